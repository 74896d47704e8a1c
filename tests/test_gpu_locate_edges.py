"""GPU: both object searches of csrc/post_kernels.hip (one lane per frame, one wave per frame) on the constructed frames of
tests/locate_cases.py -- the decision edges of the reference's locate_objects (helpers.py:424-480), shared and skipped points,
members across the wave search's 64-point chunks, dense clutter, non-finite points, out-of-range counts -- and at the grid limits
of both kernels; the carry of the compaction's scan of block totals.

Every frame is compared with the restatement (oracle.mocap_oracle.locate_objects, one frame at a time): n_obj, lead and droneIndex
exact, pos and error bit for bit, heading to 1e-12 absolute.  The frames recorded in tests/golden/locate_edges.npz are also compared
with what the reference's own function returned (error to rtol 1e-14: np.mean is a library call upstream).  Outputs are pre-filled
with a sentinel: slots at or beyond min(n_obj, O_max) keep it, and so does a guard frame behind the last one."""
import os

import numpy as np
import pytest

import locate_cases as lc
from conftest import load_golden

pytestmark = pytest.mark.gpu

SENT, ISENT = -7777.25, -77
FLOATS, INTS = ("pos", "heading", "error"), ("droneIndex", "lead", "n_obj")


def locate(core, xyz, err, n_pts, O_max, which=None):
    """mocap_locate_objects_dev on sentinel-filled outputs of F + 1 frames; which = "lane" / "wave" forces a search, None leaves
    the choice to the library.  Returns host arrays, the guard frame included."""
    import torch
    dev = torch.device("cuda", 0)
    F, K = err.shape
    d_in = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xyz, err, np.asarray(n_pts, dtype=np.int32))]
    shapes = {"pos": (F + 1, O_max, 3), "heading": (F + 1, O_max), "error": (F + 1, O_max), "droneIndex": (F + 1, O_max),
              "lead": (F + 1, O_max), "n_obj": (F + 1,)}
    d = {k: torch.full(s, SENT if k in FLOATS else ISENT, dtype=torch.float64 if k in FLOATS else torch.int32, device=dev)
         for k, s in shapes.items()}
    torch.cuda.synchronize()
    assert "MOCAP_LOCATE_KERNEL" not in os.environ
    if which:
        os.environ["MOCAP_LOCATE_KERNEL"] = which
    try:
        core.locate_objects_dev(F, K, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), O_max, d["pos"].data_ptr(),
                                d["heading"].data_ptr(), d["error"].data_ptr(), d["droneIndex"].data_ptr(), d["n_obj"].data_ptr(),
                                d["lead"].data_ptr())
        core.synchronize()
    finally:
        if which:
            del os.environ["MOCAP_LOCATE_KERNEL"]
    return {k: v.cpu().numpy() for k, v in d.items()}


def fit(a, O_max, fill):
    """The statement's per-object array cut or padded to O_max object slots."""
    out = np.full((a.shape[0], O_max) + a.shape[2:], fill, dtype=a.dtype)
    m = min(O_max, a.shape[1])
    out[:, :m] = a[:, :m]
    return out


def same_bits(a, b):
    """Bit for bit; two NaNs count as the same whatever their payload."""
    ab, bb = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
    return bool(((ab == bb) | (np.isnan(a) & np.isnan(b))).all())


def check(got, want, O_max, tag):
    """got: locate()'s arrays (F + 1 frames); want: the statement's (F frames, any number of object slots)."""
    F = want["n_obj"].shape[0]
    for k in FLOATS + INTS:                                          # the guard behind the last frame
        assert (got[k][F] == (SENT if k in FLOATS else ISENT)).all(), (tag, k, "guard frame written")
    assert np.array_equal(got["n_obj"][:F], want["n_obj"]), (tag, np.flatnonzero(got["n_obj"][:F] != want["n_obj"])[:8])
    have = np.arange(O_max)[None, :] < np.minimum(want["n_obj"], O_max)[:, None]
    for k in ("lead", "droneIndex"):
        w = fit(want[k], O_max, ISENT)
        w[~have] = ISENT
        assert np.array_equal(got[k][:F], w), (tag, k, np.argwhere(got[k][:F] != w)[:8])
    for k in ("pos", "error"):
        w = fit(want[k], O_max, SENT)
        w[~have] = SENT
        assert same_bits(got[k][:F], w), (tag, k)
    assert (got["heading"][:F][~have] == SENT).all(), (tag, "heading beyond n_obj")
    dh = np.abs(got["heading"][:F][have] - fit(want["heading"], O_max, SENT)[have])
    assert not have.any() or dh.max() <= 1e-12, (tag, "heading", dh.max())       # (an inexact atan2 at +-pi/2 shows as pi here)


def check_golden(got, fam, idx, O_max, tag):
    g = load_golden("locate_edges")
    n = g[fam + "_ref_nobj"]
    assert np.array_equal(got["n_obj"][idx], n), tag
    O = min(O_max, g[fam + "_ref_drone"].shape[1])
    have = np.arange(O)[None, :] < n[:, None]
    assert np.array_equal(got["droneIndex"][idx][:, :O][have], g[fam + "_ref_drone"][:, :O][have]), tag
    assert np.array_equal(got["pos"][idx][:, :O][have], g[fam + "_ref_pos"][:, :O][have]), tag
    np.testing.assert_allclose(got["error"][idx][:, :O][have], g[fam + "_ref_error"][:, :O][have], rtol=1e-14, atol=0)
    np.testing.assert_allclose(got["heading"][idx][:, :O][have], g[fam + "_ref_heading"][:, :O][have], rtol=0, atol=1e-12)


def both_searches(core, xyz, err, n_pts, want, O_max, tag):
    out = {}
    for which in ("lane", "wave"):
        out[which] = locate(core, xyz, err, n_pts, O_max, which)
        check(out[which], want, O_max, (tag, which))
    for k in FLOATS:                                                  # the two are one function: heading included
        assert same_bits(out["lane"][k], out["wave"][k]), (tag, k, "lane != wave")
    for k in INTS:
        assert np.array_equal(out["lane"][k], out["wave"][k]), (tag, k, "lane != wave")
    return out


@pytest.mark.parametrize("fam", lc.CONSTRUCTED + ("dense",))
def test_both_searches_on_constructed_frames(core, fam):
    cs = lc.case_set(fam)
    st = lc.statement(cs)
    O_max = st["lead"].shape[1]                                       # the fullest frame's count: nothing is dropped
    print(fam, "frames", len(cs["labels"]), "objects", int(st["n_obj"].sum()), "O_max", O_max)
    out = both_searches(core, cs["xyz"], cs["err"], cs["n_pts"], st, O_max, fam)
    idx = dict((name, i) for name, _, i in lc.recorded())[fam]
    for which in ("lane", "wave"):
        check_golden(out[which], fam, idx, O_max, (fam, which))


@pytest.mark.parametrize("O_max", [1, 12, 256])
def test_capacity_keeps_the_count_and_the_first_objects(core, O_max):
    """n_obj is the full count whatever O_max is; the first O_max objects are the statement's first O_max."""
    cs = lc.case_set("dense")
    st = lc.statement(cs)
    assert st["n_obj"].min() > 12 and st["n_obj"].max() < 256       # 1 and 12 drop objects in every frame, 256 in none
    out = both_searches(core, cs["xyz"], cs["err"], cs["n_pts"], st, O_max, ("dense", O_max))
    check_golden(out["wave"], "dense", lc.dense_recorded(cs), O_max, ("dense", O_max))


GRID_O_MAX = 12


@pytest.mark.parametrize("which,F", [("wave", 4095), ("wave", 4096), ("wave", 4097), ("wave", 8193), ("lane", 1), ("lane", 63),
                                     ("lane", 65), (None, 16383), (None, 16384)])
def test_grid_limits_on_the_tiled_bank(core, which, F):
    """The wave search launches at most 4 096 workgroups and walks further frames in that stride with ONE LDS copy: in the tiling
    a 3-point triangle and a frame with its count out of range follow the dense 256-point frame in the same workgroup.  With no
    environment variable the library takes the wave search below 16 384 frames and the lane search from there on."""
    xyz, err, n_pts, want = lc.tiled(lc.case_set("grid_bank"), F)
    got = locate(core, xyz, err, n_pts, GRID_O_MAX, which)
    check(got, want, GRID_O_MAX, (which, F))


def test_lane_search_beyond_its_grid(core):
    """16 384 x 64 + 65 frames: the lane search's grid covers 16 384 x 64, the last 65 frames are second turns of their lanes.
    Triangles and empties only (K_max 4, O_max 2)."""
    F = 16384 * 64 + 65
    xyz, err, n_pts, want = lc.tiled(lc.case_set("small_bank"), F)
    assert want["n_obj"][-65:].sum() > 20 and want["n_obj"].max() == 2
    got = locate(core, xyz, err, n_pts, 2, "lane")
    check(got, want, 2, ("lane", F))


def test_compaction_scan_carries_across_passes(core):
    """mocap_compact_tracks_dev over 1 024 x 1 024 + 1 025 frames: 1 026 scan blocks, so the scan of the block totals runs a second
    pass of 1 024 and carries the first pass's sum into it.  Whole blocks of empty frames (the last of the first pass and the first
    of the second among them), out-of-range counts, a last block of one frame; offsets, total and every record byte against
    mocap_core.dist.compact_tracks_reference, nothing written behind the last record."""
    import torch
    from mocap_core import dist as mdist, synth
    F, K, C = 1024 * 1024 + 1025, 2, 1
    rig = synth.ring_rig(2)
    core.set_cameras(rig["K"][:C], rig["R"][:C], rig["t"][:C])
    rng = np.random.default_rng(1026)
    n_out = rng.integers(-1, 4, F).astype(np.int32)                   # -1 and 3 (> K): no valid slot
    for b in (0, 3, 500, 1023, 1024):
        n_out[b * 1024:(b + 1) * 1024] = 0
    assert (F + 1023) // 1024 == 1026 and F % 1024 == 1 and n_out[-1024:].any()
    n_out[-1] = 2                                                     # the one frame of the last block
    xyz, err = rng.normal(size=(F, K, 3)), rng.random((F, K))
    corr = rng.integers(-1, 16, (F, K, C)).astype(np.int16)
    rec_ref, off_ref = mdist.compact_tracks_reference(n_out, xyz, err, corr)
    total_ref = int(off_ref[-1])
    assert off_ref[1024 * 1024] > 0 and total_ref > off_ref[1024 * 1024]     # records on both sides of the carry
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(a).to(dev) for a in (n_out, xyz, err, corr)]
    stride = mdist.track_record_bytes(C)
    cap = total_ref + 4096
    d_off = torch.full((F + 1,), -1, dtype=torch.int64, device=dev)
    d_rec = torch.full((cap, stride), 0xAB, dtype=torch.uint8, device=dev)
    total = torch.zeros(1, dtype=torch.int64).pin_memory()
    torch.cuda.synchronize()
    core.compact_tracks_dev(F, K, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d_off.data_ptr(),
                            d_rec.data_ptr(), cap, total.data_ptr())
    core.synchronize()
    assert int(total[0]) == total_ref
    off = d_off.cpu().numpy()
    assert np.array_equal(off, off_ref), np.flatnonzero(off != off_ref)[:8]
    rec = d_rec.cpu().numpy()
    assert np.array_equal(rec[:total_ref], rec_ref)
    assert (rec[total_ref:] == 0xAB).all()                            # nothing written past the last record
