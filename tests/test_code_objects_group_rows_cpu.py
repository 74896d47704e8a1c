"""The shipped listing of the headline search kernels after round 13, read without a GPU (csrc/frame_bb.hip).

Round 13 made a group's byte per camera the blob's row of the per-blob table (fixed layouts) and listed the provisional roots
once per frame.  For frame_bb_kernel<true, 1, 8, 16, 48> -- the instantiation bench.py's 8 x 16 workload takes -- and its
per-camera-K twin, the disassembly of lib/libmocap_core.so (llvm-objdump, through tests/isa_barriers.py) is held at or below a
ceiling in
  * static instructions (the list took the cameras' walks out of the matching: about 270 instructions of either kernel),
  * the instructions of one evaluation round: the segment between two s_barrier with the most FP64 instructions (the rows took
    the extract / compare / select / shift-add chains per camera out of the table sums: 29 of 1 548 in the identical-K kernel).
A ceiling is the figure of the listing round 13 shipped, rounded up by 2 %, as in tests/test_code_objects_eval_path_cpu.py.
"""
import math
import os
import re

import pytest

from test_code_objects_cpu import LIB, LLVM

# kernel (mangled-name fragment) -> the shipped listing's figures
#                                                          instructions  evaluation round
SHIPPED = {
    "frame_bb_kernelILb1ELi1ELi8ELi16ELi48E":              (6824,        1519),    # parent: 7 174, 1 548
    "frame_bb_calib_kernelILb1ELi1ELi8ELi16ELi48E":        (8584,        2090),    # parent: 8 872, 2 103
}
FIELDS = ("instructions", "evaluation_round")
_FP64 = re.compile(r"^v_\w+_f64")


def round_figures(insts):
    """[(addr, mnemonic, operands, branch target)] of one kernel -> the two figures.  Segments end with their s_barrier."""
    segs = [[0, 0]]   # [instructions, FP64 instructions]
    for _, mn, _, _ in insts:
        segs[-1][0] += 1
        segs[-1][1] += 1 if _FP64.match(mn) else 0
        if mn == "s_barrier":
            segs.append([0, 0])
    n, _ = max(segs, key=lambda s: s[1])
    return {"instructions": len(insts), "evaluation_round": n}


def test_figures_on_a_hand_written_listing():
    """The counting itself: three segments, the middle one has the most FP64 instructions (conversions to f64 count, f32 does not)."""
    listing = ["v_add_f64", "s_barrier", "v_fma_f64", "v_mov_b32_e32", "v_cvt_f64_f32_e32", "v_mul_f64", "ds_read_b128", "s_barrier",
               "v_add_f32_e32", "v_add_f32_e32", "v_add_f32_e32", "v_add_f32_e32", "v_add_f32_e32", "v_add_f32_e32", "v_add_f64", "s_endpgm"]
    insts = [(4 * i, mn, "", None) for i, mn in enumerate(listing)]
    assert round_figures(insts) == {"instructions": 16, "evaluation_round": 6}


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("library or LLVM tools not present")
    import isa_barriers as ib
    return ib.disassemble(LIB, str(tmp_path_factory.mktemp("group_rows")))


@pytest.mark.parametrize("kernel", list(SHIPPED))
def test_instruction_counts_stay_below_their_ceilings(listings, kernel):
    names = [k for k in listings if kernel in k]
    assert len(names) == 1, (kernel, names)
    got = round_figures(listings[names[0]])
    for field, shipped in zip(FIELDS, SHIPPED[kernel]):
        ceiling = math.ceil(shipped * 1.02)
        assert got[field] <= ceiling, (kernel, field, got[field], "ceiling %d = shipped %d + 2 %%" % (ceiling, shipped), got)
