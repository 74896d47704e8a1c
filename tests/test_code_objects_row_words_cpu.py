"""The shipped listing of the headline search kernels after round 14, read without a GPU (csrc/frame_bb.hip).

Round 14 reads a root's rows of `act` and `nh` as one 64-bit word each in the search's decodes (fetch_candidate, block_pk) and
in phase C, and lets the pair loop keep the closest hit while it walks a camera's blobs.  For frame_bb_kernel<true, 1, 8, 16, 48>
-- the instantiation bench.py's 8 x 16 workload takes -- and its per-camera-K twin, the disassembly of lib/libmocap_core.so
(llvm-objdump, through tests/isa_barriers.py) is held at or below a ceiling in
  * static instructions (phase C from registers and the walk's running minimum ADD instructions, 120 and 125: what they take
    away is dependent LDS round trips on the frame's serial path, not issue),
  * the instructions of one evaluation round: the segment between two s_barrier with the most FP64 instructions,
  * the byte-wide LDS reads (ds_read_u8) of that round: the record's root sizes and one `hits` byte per digit -- a digit's camera
    and hit count are no longer among them (5 before).
A ceiling is the figure of the listing round 14 shipped, rounded up by 2 %, as in tests/test_code_objects_group_rows_cpu.py.
"""
import math
import os

import pytest

from test_code_objects_cpu import LIB, LLVM
from test_code_objects_group_rows_cpu import _FP64

# kernel (mangled-name fragment) -> the shipped listing's figures
#                                                          instructions  evaluation round  ds_read_u8 in the round
SHIPPED = {
    "frame_bb_kernelILb1ELi1ELi8ELi16ELi48E":              (6944,        1526,             3),    # parent: 6 824, 1 519, 5
    "frame_bb_calib_kernelILb1ELi1ELi8ELi16ELi48E":        (8709,        2091,             3),    # parent: 8 584, 2 090, 5
}
FIELDS = ("instructions", "evaluation_round", "byte_reads_in_the_round")


def round_figures(insts):
    """[(addr, mnemonic, operands, branch target)] of one kernel -> the three figures.  Segments end with their s_barrier."""
    segs = [[0, 0, 0]]   # [instructions, FP64 instructions, ds_read_u8]
    for _, mn, _, _ in insts:
        segs[-1][0] += 1
        segs[-1][1] += 1 if _FP64.match(mn) else 0
        segs[-1][2] += 1 if mn == "ds_read_u8" else 0
        if mn == "s_barrier":
            segs.append([0, 0, 0])
    n, _, u8 = max(segs, key=lambda s: s[1])
    return {"instructions": len(insts), "evaluation_round": n, "byte_reads_in_the_round": u8}


def test_figures_on_a_hand_written_listing():
    """The counting itself: three segments, the middle one has the most FP64 instructions; byte reads outside it do not count,
    nor do wider or signed reads inside it."""
    listing = ["ds_read_u8", "v_add_f64", "s_barrier", "v_fma_f64", "ds_read_u8", "ds_read_u8", "ds_read_b64", "ds_read_i8", "v_mul_f64", "s_barrier",
               "ds_read_u8", "ds_read_u8", "ds_read_u8", "v_add_f64", "s_endpgm"]
    insts = [(4 * i, mn, "", None) for i, mn in enumerate(listing)]
    assert round_figures(insts) == {"instructions": 15, "evaluation_round": 7, "byte_reads_in_the_round": 2}


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("library or LLVM tools not present")
    import isa_barriers as ib
    return ib.disassemble(LIB, str(tmp_path_factory.mktemp("row_words")))


@pytest.mark.parametrize("kernel", list(SHIPPED))
def test_row_word_figures_stay_below_their_ceilings(listings, kernel):
    names = [k for k in listings if kernel in k]
    assert len(names) == 1, (kernel, names)
    got = round_figures(listings[names[0]])
    for field, shipped in zip(FIELDS, SHIPPED[kernel]):
        ceiling = math.ceil(shipped * 1.02)
        assert got[field] <= ceiling, (kernel, field, got[field], "ceiling %d = shipped %d + 2 %%" % (ceiling, shipped), got)
