"""The shipped listing of the headline search kernels after round 15, read without a GPU (csrc/frame_bb.hip).

Round 15 rewrote the blob walk of match()'s two pair passes for the layouts fixed at compile time: the camera's sixteen slots are
read as eight 16-byte words whatever the count, a float32 pre-test (the wide variant's, tests/test_wide_pretest_bound_cpu.py)
drops the clear misses -- two fused multiply-adds and a compare per slot, no branch, no wait per blob --, and the exact double
distance is computed in one short loop for the blobs that pass.  For frame_bb_kernel<true, 1, 8, 16, 48> -- the instantiation
bench.py's 8 x 16 workload takes -- and its per-camera-K twin, the disassembly of lib/libmocap_core.so (llvm-objdump, through
tests/isa_barriers.py) is held at or below a ceiling in
  * static instructions,
  * the instructions of the segment between two s_barrier that holds the pair code: the one with the most float32 fused
    multiply-adds (the pre-test's 32; every other segment of the kernel computes in double),
  * the s_waitcnt of that segment that wait for the LDS / scalar-memory counter (lgkmcnt): a walk that waits per blob again adds
    sixteen.
A ceiling is the figure of the listing round 15 shipped, rounded up by 2 %, as in tests/test_code_objects_row_words_cpu.py.
(The walk's straight-line pre-test is LONGER than the four copies of the per-blob body it replaces, 1 214 against 1 182
instructions: what it takes away is executed instructions, branches and LDS round trips, not text.)
"""
import math
import os

import pytest

from test_code_objects_cpu import LIB, LLVM

# kernel (mangled-name fragment) -> the shipped listing's figures
#                                                          instructions  pair segment  lgkmcnt waits in it
SHIPPED = {
    "frame_bb_kernelILb1ELi1ELi8ELi16ELi48E":              (6960,        1214,         43),    # parent: 6 944, 1 182, 43
    "frame_bb_calib_kernelILb1ELi1ELi8ELi16ELi48E":        (8720,        1209,         42),    # parent: 8 709, 1 182, 43
}
FIELDS = ("instructions", "pair_segment", "lgkmcnt_waits_in_the_pair_segment")
_FMA32 = ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32")
MIN_FMA32 = 16   # a segment with fewer is not the pre-test's


def pair_figures(insts):
    """[(addr, mnemonic, operands, branch target)] of one kernel -> the three figures.  Segments end with their s_barrier."""
    segs = [[0, 0, 0]]   # [instructions, float32 fused multiply-adds, waits for lgkmcnt]
    for _, mn, ops, _ in insts:
        segs[-1][0] += 1
        segs[-1][1] += 1 if mn.startswith(_FMA32) else 0
        segs[-1][2] += 1 if mn == "s_waitcnt" and "lgkmcnt" in ops else 0
        if mn == "s_barrier":
            segs.append([0, 0, 0])
    n, fma, waits = max(segs, key=lambda s: s[1])
    assert fma >= MIN_FMA32, ("no segment holds the float32 pre-test", [s[1] for s in segs])
    return {"instructions": len(insts), "pair_segment": n, "lgkmcnt_waits_in_the_pair_segment": waits}


def test_figures_on_a_hand_written_listing():
    """The counting itself: three segments, the middle one has the float32 multiply-adds (in their e32 / e64 / packed spellings);
    waits outside it do not count, nor do waits for another counter inside it."""
    listing = [("s_waitcnt", "lgkmcnt(0)"), ("v_fma_f64", ""), ("s_barrier", "")]
    listing += [("v_fma_f32", "")] * 6 + [("v_fmac_f32_e32", "")] * 6 + [("v_pk_fma_f32", "")] * 4
    listing += [("s_waitcnt", "vmcnt(0)"), ("s_waitcnt", "vmcnt(0) lgkmcnt(1)"), ("s_waitcnt", "lgkmcnt(0)"), ("v_fma_f64", ""), ("s_barrier", "")]
    listing += [("s_waitcnt", "lgkmcnt(0)"), ("v_fma_f32", ""), ("s_endpgm", "")]
    insts = [(4 * i, mn, ops, None) for i, (mn, ops) in enumerate(listing)]
    assert pair_figures(insts) == {"instructions": 27, "pair_segment": 21, "lgkmcnt_waits_in_the_pair_segment": 2}


def test_a_listing_without_the_pre_test_is_refused():
    insts = [(4 * i, mn, "", None) for i, mn in enumerate(["v_fma_f32"] * 3 + ["s_barrier", "v_fma_f64", "s_endpgm"])]
    with pytest.raises(AssertionError):
        pair_figures(insts)


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("library or LLVM tools not present")
    import isa_barriers as ib
    return ib.disassemble(LIB, str(tmp_path_factory.mktemp("pair_walk")))


@pytest.mark.parametrize("kernel", list(SHIPPED))
def test_pair_walk_figures_stay_below_their_ceilings(listings, kernel):
    names = [k for k in listings if kernel in k]
    assert len(names) == 1, (kernel, names)
    got = pair_figures(listings[names[0]])
    for field, shipped in zip(FIELDS, SHIPPED[kernel]):
        ceiling = math.ceil(shipped * 1.02)
        assert got[field] <= ceiling, (kernel, field, got[field], "ceiling %d = shipped %d + 2 %%" % (ceiling, shipped), got)
