"""The per-camera-K heavy-root kernels (csrc/heavy_bb.hip: heavy_bb_calib_kernel, heavy_enum_calib_kernel) and the wide
instantiations that export heavy roots on such rigs (csrc/frame_kernel.hip, UNIFORM_K = false, HEAVY = true) inside
lib/libmocap_core.so, read without a GPU like tests/test_code_objects_calibrated_cpu.py reads the per-camera-K search kernels:
each one the launch can pick is there for gfx950 for both F32R settings, its VGPR count allows the occupancy its launch bounds
plan for, spills and scratch stay at the figures DESIGN.md 3.8 records, and the identical-K kernels keep their symbols."""
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
    d = tmp_path_factory.mktemp("co_heavy_calib")
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
                         for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
                                   "max_flat_workgroup_size")}
    return out


def _one(kernels, stem):
    hits = [k for k in kernels if stem in k]
    assert len(hits) == 1, (stem, hits)
    return kernels[hits[0]]


# F32R -> (spilled VGPRs, bytes of scratch) as compiled ("per-camera intrinsics")
SEARCH = {"Lb1E": (55, 192), "Lb0E": (65, 192)}


@pytest.mark.parametrize("f32r", sorted(SEARCH))
def test_calibrated_heavy_search_kernel(kernels, f32r):
    """1 024 lanes = 16 waves, one workgroup per CU = 4 waves per SIMD: at most 512 / 4 = 128 VGPRs."""
    k = _one(kernels, "heavy_bb_calib_kernelI" + f32r)
    spills, scratch = SEARCH[f32r]
    assert k["max_flat_workgroup_size"] == 1024 and k["vgpr_count"] <= 128, k
    assert k["vgpr_spill_count"] <= spills and k["private_segment_fixed_size"] <= scratch, k
    # (static LDS: the identical-K kernel's plus the position table, 64 bytes)
    assert k["group_segment_fixed_size"] == _one(kernels, "heavy_bb_kernelI" + f32r)["group_segment_fixed_size"] + 64, k


@pytest.mark.parametrize("f32r", ["Lb1E", "Lb0E"])
def test_calibrated_heavy_enumeration_kernel(kernels, f32r):
    """256 lanes, three workgroups per CU planned (the launch's grid: 3 per CU) = 3 waves per SIMD: at most 168 VGPRs
    (512 / 3 in granules of 8), nothing spilled -- the identical-K kernel's figures."""
    k = _one(kernels, "heavy_enum_calib_kernelI" + f32r)
    assert k["max_flat_workgroup_size"] == 256 and k["vgpr_count"] <= 168, k
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == _one(kernels, "heavy_enum_kernelI" + f32r)["group_segment_fixed_size"] + 64, k
    assert 3 * k["group_segment_fixed_size"] <= 160 * 1024


@pytest.mark.parametrize("f32r", ["Lb1E", "Lb0E"])
@pytest.mark.parametrize("lanes", [512, 1024])
def test_wide_instantiation_that_exports_heavy_roots_with_per_camera_k(kernels, lanes, f32r):
    """frame_kernel<T, UNIFORM_K = false, F32R, WIDE = true, MODE_ALL, HEAVY = true>: 16 waves per CU either way (one frame of
    1 024 lanes or two of 512), 128 VGPRs; 40 spilled registers and 160 bytes of scratch as compiled (the identical-K exporting
    instantiation: 26-28 and 144)."""
    k = _one(kernels, "frame_kernelILi%dELb0E%sLb1ELi3ELb1E" % (lanes, f32r))
    assert k["max_flat_workgroup_size"] == lanes and k["vgpr_count"] <= 128, k
    assert k["vgpr_spill_count"] <= 40 and k["private_segment_fixed_size"] <= 160, k
    assert k["group_segment_fixed_size"] == 0, k          # LDS is dynamic: sized by frame_lds_bytes for the launch
    # the export lives in instantiations of its own: the ones the first pass takes on these rigs are as they were
    first = _one(kernels, "frame_kernelILi%dELb0E%sLb1ELi3ELb0E" % (lanes, f32r))
    assert first["vgpr_spill_count"] < k["vgpr_spill_count"], (first, k)


def test_identical_k_heavy_kernels_keep_their_symbols(kernels):
    """The variants have __global__ names of their own: the identical-K instantiations are found by the names they had, two
    (F32R on / off) of each."""
    assert len([k for k in kernels if "heavy_bb_kernelI" in k]) == 2
    assert len([k for k in kernels if "heavy_enum_kernelI" in k]) == 2
    assert len([k for k in kernels if "heavy_bb_calib_kernelI" in k]) == 2
    assert len([k for k in kernels if "heavy_enum_calib_kernelI" in k]) == 2
    # the exporting wide instantiations: 512 / 1 024 lanes x F32R, identical K and per-camera K
    assert len([k for k in kernels if re.search(r"frame_kernelILi(512|1024)ELb1ELb[01]ELb1ELi3ELb1E", k)]) == 4
    assert len([k for k in kernels if re.search(r"frame_kernelILi(512|1024)ELb0ELb[01]ELb1ELi3ELb1E", k)]) == 4
