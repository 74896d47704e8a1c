"""The shipped listing of the headline search kernels, read without a GPU: what the compiler adds around the arithmetic of the
evaluation path (csrc/frame_bb.hip, csrc/mocap_device.hpp) stays where round 11 left it.

For frame_bb_kernel<true, 1, 8, 16, 48> -- the instantiation bench.py's 8 x 16 workload takes -- and its per-camera-K twin, the
disassembly of lib/libmocap_core.so (llvm-objdump, through tests/isa_barriers.py) is held at or below a ceiling in
  * static instructions,
  * v_mov (the zero-fill cascades in front of exec-mask regions: score_point's partial sums),
  * lane moves (v_readlane / v_writelane: scalar registers spilled to vector lanes),
  * s_waitcnt with a vmcnt operand inside the frame loop (waits for global memory on paths that only touch LDS: the barriers
    of the search's rounds, the LDS reads behind the frame's global_load_lds prefetch).
A ceiling is the figure of the listing round 11 shipped, rounded up by 2 %.  The kernel is bound by instruction issue
(DESIGN.md 3.1), so a regression here is time; it shows in this test before anybody measures it.
"""
import math
import os

import pytest

from test_code_objects_cpu import LIB, LLVM

# kernel (mangled-name fragment) -> the shipped listing's figures
#                                                          instructions  v_mov  lane moves  vmcnt waits in the frame loop
SHIPPED = {
    "frame_bb_kernelILb1ELi1ELi8ELi16ELi48E":              (7174,        529,   172,        16),    # parent: 7 195, 573, 172, 30
    "frame_bb_calib_kernelILb1ELi1ELi8ELi16ELi48E":        (8872,        576,   199,        45),    # parent: 8 897, 636, 233, 61
}
FIELDS = ("instructions", "v_mov", "lane_moves", "vmcnt_waits_in_frame_loop")


def listing_figures(insts):
    """[(addr, mnemonic, operands, branch target)] of one kernel -> the four figures.  The frame loop is the backward branch
    with the widest span (the persistent loop over the frames encloses every other loop of the kernel)."""
    back = [(a - tgt, tgt, a) for a, _, _, tgt in insts if tgt is not None and tgt < a]
    assert back, "no loop in the kernel"
    _, lo, hi = max(back)
    return {
        "instructions": len(insts),
        "v_mov": sum(1 for i in insts if i[1].startswith("v_mov_")),
        "lane_moves": sum(1 for i in insts if i[1].startswith(("v_readlane", "v_writelane"))),
        "vmcnt_waits_in_frame_loop": sum(1 for a, mn, ops, _ in insts if lo <= a <= hi and mn == "s_waitcnt" and "vmcnt" in ops),
    }


def test_figures_on_a_hand_written_listing():
    """The counting itself: a frame loop around an inner loop, one wait inside and one outside the frame loop."""
    listing = [("s_waitcnt", "vmcnt(0)", None), ("v_mov_b32_e32", "v1, 0", None), ("v_writelane_b32", "v2, s0, 1", None),
               ("s_waitcnt", "vmcnt(0) lgkmcnt(0)", None), ("v_mov_b64_e32", "v[2:3], 0", None), ("s_cbranch_scc1", "-2", 3),
               ("v_readlane_b32", "s0, v2, 1", None), ("s_waitcnt", "lgkmcnt(0)", None), ("s_cbranch_vccnz", "-8", 1),
               ("s_endpgm", "", None)]
    insts = [(4 * i, mn, ops, None if t is None else 4 * t) for i, (mn, ops, t) in enumerate(listing)]
    assert listing_figures(insts) == {"instructions": 10, "v_mov": 2, "lane_moves": 2, "vmcnt_waits_in_frame_loop": 1}


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("library or LLVM tools not present")
    import isa_barriers as ib
    return ib.disassemble(LIB, str(tmp_path_factory.mktemp("eval_path")))


@pytest.mark.parametrize("kernel", list(SHIPPED))
def test_evaluation_path_figures_stay_below_their_ceilings(listings, kernel):
    names = [k for k in listings if kernel in k]
    assert len(names) == 1, (kernel, names)
    got = listing_figures(listings[names[0]])
    for field, shipped in zip(FIELDS, SHIPPED[kernel]):
        ceiling = math.ceil(shipped * 1.02)
        assert got[field] <= ceiling, (kernel, field, got[field], "ceiling %d = shipped %d + 2 %%" % (ceiling, shipped), got)
