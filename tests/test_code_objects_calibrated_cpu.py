"""The per-camera-K search kernels (csrc/frame_bb.hip, frame_bb_calib_kernel) inside lib/libmocap_core.so, read without a
GPU like tests/test_code_objects_cpu.py reads the identical-K ones: every instantiation the launch can pick is there for
gfx950, its VGPR count allows the workgroups per CU its LDS layout is planned for (five for the 8 x 16 layout with 48 root
slots, four elsewhere), and spills and scratch stay at the figures DESIGN.md 3.1 records for them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "low-cost-mocap_amd", "lib", "libmocap_core.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("library or LLVM tools not present")
    d = tmp_path_factory.mktemp("co_calib")
    shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
    objs = [f for f in os.listdir(d) if "amdgcn" in f]
    assert objs and all(f.endswith("gfx950") for f in objs), objs
    out = {}
    for f in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=d, check=True, capture_output=True,
                               text=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            out[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                         for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return out


# <F32R, CW, CT, ML, RL> -> (VGPR ceiling of the planned occupancy: 512 / workgroups per CU in granules of 8,
#                            spilled VGPRs, bytes of scratch: DESIGN.md 3.1, "per-camera intrinsics")
BUDGET = {
    "Li1ELi8ELi16ELi48E": (96, 5, 24),     # five workgroups per CU
    "Li1ELi8ELi16ELi64E": (128, 0, 0),
    "Li1ELi8ELi0ELi0E": (128, 0, 0),
    "Li1ELi0ELi0ELi0E": (128, 0, 0),       # runtime layout, CW = 1
    "Li2ELi0ELi0ELi0E": (128, 0, 24),      # runtime layout, CW = 2
}


@pytest.mark.parametrize("f32r", ["Lb1E", "Lb0E"])
@pytest.mark.parametrize("inst", sorted(BUDGET))
def test_calibrated_search_kernels_are_there_and_inside_their_budget(kernels, f32r, inst):
    hits = [k for k in kernels if "frame_bb_calib_kernelI" + f32r + inst in k]
    assert len(hits) == 1, (f32r, inst, hits)
    k = kernels[hits[0]]
    vgprs, spills, scratch = BUDGET[inst]
    assert k["vgpr_count"] <= vgprs, k
    assert k["vgpr_spill_count"] <= spills and k["private_segment_fixed_size"] <= scratch, k
    assert k["group_segment_fixed_size"] == 0, k          # LDS is dynamic: sized by frame_bb_lds_bytes for the launch


def test_identical_k_kernels_keep_their_symbols(kernels):
    """The variant has a __global__ name of its own: the identical-K instantiations are found by the names they had."""
    assert len([k for k in kernels if "frame_bb_kernelI" in k]) == 10
    assert len([k for k in kernels if "frame_bb_calib_kernelI" in k]) == 10
