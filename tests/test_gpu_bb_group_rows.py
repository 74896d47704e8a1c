"""GPU: the search kernels' fixed layouts (8 cameras x 16 blobs, 48 or 64 root slots) after round 13 (csrc/frame_bb.hip).

Round 13 changed what two pieces of the frame's state ARE, neither of which may show in a result:
  * a group's byte per camera is the blob's row c * 16 + k of the per-blob table (rows 0 .. 127; 128, the table's record of
    zeros, = the camera is open or absent) where it was the blob index (0xFF = absent): the hit lists, pkbase, the queued
    records and the winner's record carry rows, the table sums and the observation fetch take the byte as it is, phase E
    turns it back into the blob index;
  * the provisional roots -- the blobs of cameras 1 .. 7 the camera-0 roots leave unclaimed -- are listed once per frame
    behind stage 0's barrier (one byte each, (camera, blob) order); stage 1's pair decode and B1's lane set-up look their
    root up in the list instead of walking the cameras and the set bits of the unclaimed masks.
The runtime layouts (any other M_max or camera count, two-word groups) keep blob-index bytes and the walks.

What can go wrong: the highest row (127: blob 15 of camera 7) or the row of zeros mistaken for one another or cut by a mask, a
camera that is absent in the middle or at the end of a group, groups that start at a later camera, a byte decoded with the
wrong camera, a list that is empty, has no pairs, is exactly one wave long or longer, staging rows that do not fit.  Every
case compares every bit of n_out, status, corr, xyz and err (mocap_core.devcheck.compare_bitwise) and n_cand with the
exhaustive walk on a second context; the hand-built cases assert on the CPU, with the oracle's matching, that their frames are
at the edge they are named for.

Streams: seed 1, gate 5 px, G_cap 2^20 (the walk alone flags under 1 % of these streams' frames: asserted in _walk).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from mocap_core import synth
from test_gpu_bb_eval_path import GATE, KERNELS, RIGS, ROOT, _frames_with_n_prov, _search_equals, _to_dev, _walk, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

C, M = 8, 16
F_STREAM = 4096   # more than three buffer swaps per resident workgroup (256 CUs x 5 workgroups = 1 280 at the most)


@functools.lru_cache(maxsize=None)
def _rig(rig_name, cams=C):
    return RIGS[rig_name](cams)


@functools.lru_cache(maxsize=None)
def _stream(rig_name, F, markers, dropout=0.05, m_max=M):
    blobs, counts, _ = synth.make_blob_stream(_rig(rig_name), F, markers, seed=1, dropout=dropout, m_max=m_max)
    blobs.setflags(write=False)
    counts.setflags(write=False)
    return blobs, counts


@functools.lru_cache(maxsize=None)
def _ftab(rig_name):
    from oracle import mocap_oracle as mo
    rig = _rig(rig_name)
    return mo.fundamental_table(rig["K"], rig["R"], rig["t"])


def _match(rig_name, blobs_f, counts_f):
    from oracle import mocap_oracle as mo
    return mo.match_frame(blobs_f.astype(np.float64), counts_f, _ftab(rig_name), gate_px=GATE)


# ------------------------------------------------------------------------------------------------ 1. the bench's streams

@pytest.mark.parametrize("f32", [True, False], ids=["float32 rounding", "no float32 rounding"])
@pytest.mark.parametrize("K_max", [48, 64])
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_streams_equal_the_walk(gpu, rig_name, K_max, f32):
    dev, _ = gpu
    rig = _rig(rig_name)
    blobs, counts = _stream(rig_name, F_STREAM, M)
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, C, M, K_max, d_b, d_c, min_points=F_STREAM, f32=f32)
    _search_equals(gpu, rig, ref, M, d_b, d_c, KERNELS[rig_name] % 1, f32=f32)


# ------------------------------------------------------------------------------------------------ 2. rows at their edges

def _all_hits(hr):
    return [h for h in hr if h]


def _case(name, rig_name):
    """-> blobs, counts [F][8][16], frames to assert on, predicate on a frame's (roots, hits, counts)."""
    if name == "row 127":
        # every camera holds 16 blobs and a root's only hit in camera 7 is blob 15: each of its candidates, the winner
        # included, carries row 127
        b, c = _stream(rig_name, 96, M, dropout=0.0)
        full = np.flatnonzero((c == M).all(axis=1))
        keep = [f for f in full[:24] if any(hr[7] == [15] and len(_all_hits(hr)) >= 2 for hr in _match(rig_name, b[f], c[f])[1])]
        assert len(keep) >= 2, (len(full), len(keep))
        b, c = b[keep], c[keep]
        return b, c, range(len(keep)), lambda roots, hits, cnt: (cnt == M).all() and any(hr[7] == [15] for hr in hits)
    b, c = (a.copy() for a in _stream(rig_name, 96, 12))
    if name == "a camera absent in the middle, the last camera absent":
        c[:48, 4] = 0
        c[48:, 7] = 0
        return b, c, (0, 1, 48, 49), lambda roots, hits, cnt: any(
            rc == 0 and not hr[4 if cnt[4] == 0 else 7] and len(_all_hits(hr)) >= 3 for (rc, _), hr in zip(roots, hits))
    if name == "roots created at camera 3 and at camera 6":
        c[:48, :3] = 0
        c[48:, :6] = 0
        return b, c, (0, 1, 48, 49), lambda roots, hits, cnt: bool(roots) and roots[0][0] == (3 if cnt[5] else 6) and any(
            rc == (3 if cnt[5] else 6) and _all_hits(hr) for (rc, _), hr in zip(roots, hits))
    if name == "a two-view root":
        keep = np.zeros(C, dtype=bool)
        keep[[0, 7]] = True
        c[:, ~keep] = 0
        return b, c, (0, 1, 2, 3), lambda roots, hits, cnt: any(rc == 0 and len(_all_hits(hr)) == 1 and hr[7] for (rc, _), hr in zip(roots, hits))
    assert name == "camera 1 the only multi-hit camera"
    # clean frames of two well separated markers, plus in camera 1 a copy of root 0's closest blob one pixel away: two hits there, one everywhere else
    b2, c2, _ = synth.make_blob_stream(_rig(rig_name), 64, 2, seed=1, m_max=M, dropout=0.0, min_sep=0.6)
    got_b, got_c = [], []
    for f in range(b2.shape[0]):
        if c2[f, 0] < 1 or c2[f, 1] < 1 or c2[f, 1] >= M:
            continue
        _, hits = _match(rig_name, b2[f], c2[f])
        if not hits or not hits[0][1]:
            continue
        bf, cf = b2[f].copy(), c2[f].copy()
        bf[1, cf[1]] = bf[1, hits[0][1][0]] + np.float32(1.0)
        cf[1] += 1
        roots, hits = _match(rig_name, bf, cf)
        if any(rc == 0 and len(hr[1]) > 1 and all(len(hr[i]) <= 1 for i in range(2, C)) and len(_all_hits(hr)) >= 2 for (rc, _), hr in zip(roots, hits)):
            got_b.append(bf)
            got_c.append(cf)
    assert len(got_b) >= 8, len(got_b)
    return np.stack(got_b), np.stack(got_c), range(len(got_b)), lambda roots, hits, cnt: any(
        rc == 0 and len(hr[1]) > 1 and all(len(hr[i]) <= 1 for i in range(2, C)) for (rc, _), hr in zip(roots, hits))


ROW_CASES = ["row 127", "a camera absent in the middle, the last camera absent", "roots created at camera 3 and at camera 6", "a two-view root",
             "camera 1 the only multi-hit camera"]


@pytest.mark.parametrize("rig_name", list(RIGS))
@pytest.mark.parametrize("name", ROW_CASES)
def test_rows_at_their_edges(gpu, name, rig_name):
    dev, _ = gpu
    rig = _rig(rig_name)
    blobs, counts, frames, want = _case(name, rig_name)
    for f in frames:
        roots, hits = _match(rig_name, blobs[f], counts[f])
        assert want(roots, hits, counts[f]), (name, f)
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, C, M, 48, d_b, d_c, min_points=blobs.shape[0] // 2)
    if name == "row 127":   # ... and the walk's rows say so: a kept point with blob 15 of camera 7
        n_out, corr = ref.n_out.cpu().numpy(), ref.corr.cpu().numpy()
        assert any((corr[f, :n_out[f], 7] == 15).any() for f in range(corr.shape[0]))
    for K_max in (48, 64):
        r = ref if K_max == 48 else _walk(gpu, rig, C, M, K_max, d_b, d_c, min_points=blobs.shape[0] // 2)
        _search_equals(gpu, rig, r, M, d_b, d_c, KERNELS[rig_name] % 1)


# ------------------------------------------------------------------------------------------------ 3. the list of provisional roots

def provisional_per_camera(rig_name, blobs_f, counts_f):
    """Per camera 1 .. C-1 the blobs no camera-0 root claims (helpers.py:391 by value): the kernel's list, camera by camera."""
    from oracle import mocap_oracle as mo
    Ftab = _ftab(rig_name)
    out = [0] * C
    for i in range(1, C):
        n_i = int(counts_f[i])
        if n_i == 0:
            continue
        px, py = blobs_f[i, :n_i, 0].astype(np.float64), blobs_f[i, :n_i, 1].astype(np.float64)
        claimed = np.zeros(n_i, dtype=bool)
        for rb in range(int(counts_f[0])):
            a, b, c = mo.epiline(Ftab[0, i], blobs_f[0, rb])
            d = np.abs(a * px + b * py + c) / np.sqrt(a ** 2 + b ** 2)
            idx = [k for k in range(n_i) if d[k] < GATE]
            if idx:
                k0 = min(idx, key=lambda k: (d[k], k))
                claimed |= (px == px[k0]) & (py == py[k0])
        out[i] = int((~claimed).sum())
    return out


# 8 x 16: 200 bytes of staging rows per provisional root; 8 000 bytes of scratch at 48 slots hold 40 of them, 8 960 bytes at 64
# slots hold 44 -- 40 / 41 and 44 / 45 are where the staging rows stop fitting; 64 is a full wave of provisional roots and 65
# one more (both lists are built, both frames take the chain over the cameras)
PROV_CASES = {"no provisional root": (48, 0), "provisional roots in the last camera only: no pairs": (48, 1), "exactly 64 provisional roots": (48, 64),
              "65 provisional roots: the chain": (48, 65), "40: the staging rows just fit 48 slots": (48, 40), "41: they do not fit 48 slots": (48, 41),
              "44: the staging rows just fit 64 slots": (64, 44), "45: they do not fit 64 slots": (64, 45)}


@pytest.mark.parametrize("rig_name", list(RIGS))
@pytest.mark.parametrize("name", list(PROV_CASES))
def test_the_list_of_provisional_roots_at_its_edges(gpu, name, rig_name):
    dev, _ = gpu
    K_max, target = PROV_CASES[name]
    rig = _rig(rig_name)
    blobs, counts = _frames_with_n_prov(rig, C, M, target)
    per = [provisional_per_camera(rig_name, blobs[f], counts[f]) for f in range(blobs.shape[0])]
    assert all(sum(n) == target for n in per), (name, per)
    if target == 1:
        keep = [f for f, n in enumerate(per) if n[C - 1] == 1]
        assert len(keep) >= 2, (name, per)
        blobs, counts = blobs[keep], counts[keep]
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, C, M, K_max, d_b, d_c, min_points=blobs.shape[0])
    _search_equals(gpu, rig, ref, M, d_b, d_c, KERNELS[rig_name] % 1)


# ------------------------------------------------------------------------------------------------ 4. the layouts that did not change

@pytest.mark.parametrize("cams,m_max,cw", [(8, 12, 1), (6, 16, 1), (9, 8, 2)], ids=["8 x 12", "6 x 16", "9 x 8: two-word groups"])
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_runtime_layouts_keep_their_bytes(gpu, rig_name, cams, m_max, cw):
    dev, _ = gpu
    rig = _rig(rig_name, cams)
    blobs, counts, _ = synth.make_blob_stream(rig, 500, min(m_max, 12), seed=1, m_max=m_max)
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, cams, m_max, 48, d_b, d_c, min_points=250)
    _search_equals(gpu, rig, ref, m_max, d_b, d_c, KERNELS[rig_name] % cw)


# ------------------------------------------------------------------------------------------------ 5. the measuring build

_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [%(root)r, %(pkg)r]
import torch
from mocap_core import capi, synth
core = capi.MocapCore(0)
dev = torch.device("cuda:0")
rig = synth.ring_rig(8)
F, C, M, K, EXTRA = %(frames)d, 8, 16, 48, 11
blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
core.set_cameras(rig["K"], rig["R"], rig["t"])
d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
xyz = torch.full((F, K, 3), float("nan"), dtype=torch.float64, device=dev); err = torch.full((F, K), float("nan"), dtype=torch.float64, device=dev)
corr = torch.full((F, K, C), -2, dtype=torch.int16, device=dev); n_out = torch.zeros(F, dtype=torch.int32, device=dev)
status = torch.zeros(F + EXTRA, dtype=torch.int32, device=dev)          # + the measuring build's counters (unused by the product library)
n_cand = torch.zeros(F, dtype=torch.int32, device=dev)
core.match_triangulate_dev(F, M, d_b.data_ptr(), d_c.data_ptr(), 5.0, K, 1 << 20, xyz.data_ptr(), err.data_ptr(),
                           corr.data_ptr(), n_out.data_ptr(), status.data_ptr(), n_cand.data_ptr())
core.synchronize()
assert core.last_frame_kernel().startswith("frame_bb_kernel")
np.savez(%(out)r, xyz=xyz.cpu().numpy().view(np.uint64), err=err.cpu().numpy().view(np.uint64), corr=corr.cpu().numpy(),
         n_out=n_out.cpu().numpy(), status=status.cpu().numpy(), n_cand=n_cand.cpu().numpy())
"""


def test_measuring_build_equals_the_product_library(tmp_path):
    """lib/libmocap_core_phaseclocks.so (csrc/frame_bb.hip with -DMOCAP_BB_PHASE_CLOCKS) and the product library on one batch
    of 4 096 frames of the bench's stream, each in a process of its own into buffers filled alike: every byte of xyz, err,
    corr, n_out, status and n_cand is the same (the untouched tails included), and the measuring build's eleven counters
    behind the status array all counted."""
    libdir = os.path.join(ROOT, "low-cost-mocap_amd", "lib")
    got = {}
    for name in ("libmocap_core.so", "libmocap_core_phaseclocks.so"):
        lib = os.path.join(libdir, name)
        assert os.path.exists(lib), "build it with `make -C low-cost-mocap_amd all` (__graft_entry__.build does)"
        out = str(tmp_path / (name + ".npz"))
        code = _CHILD % {"root": ROOT, "pkg": os.path.join(ROOT, "low-cost-mocap_amd"), "frames": F_STREAM, "out": out}
        env = dict(os.environ, MOCAP_CORE_LIB=lib)
        for k in ("MOCAP_BB_PL", "MOCAP_BB_PL_MIN", "MOCAP_BB_NB_MAX", "MOCAP_BB_FIXED_LAYOUT"):
            env.pop(k, None)
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        got[name] = dict(np.load(out))
    prod, meas = got["libmocap_core.so"], got["libmocap_core_phaseclocks.so"]
    assert int(prod["n_out"].sum()) >= F_STREAM
    for field in ("xyz", "err", "corr", "n_out", "n_cand"):
        assert np.array_equal(prod[field], meas[field]), field
    assert np.array_equal(prod["status"][:F_STREAM], meas["status"][:F_STREAM])
    assert (prod["status"][F_STREAM:] == 0).all() and (meas["status"][F_STREAM:] > 0).all(), meas["status"][F_STREAM:]
