"""GPU: the pair walk of the search kernels' fixed layouts (8 cameras x 16 blobs, 48 or 64 root slots) after round 15
(csrc/frame_bb.hip, match(), stages 0 and 1).

Round 15 changed HOW a (root, camera) pair finds its hits, which may not show in a result:
  * all sixteen slots of the camera are read, whatever its count; the count is applied to the candidate mask afterwards;
  * with the float32 roundings on, a slot reaches the exact decision of helpers.py:373,375 only if it passes the wide variant's
    float32 pre-test |fmaf(a, x, fmaf(b, y, c))| <= thr, thr = RU(gate den (1 + 1e-12) + E (1 + 1e-6)),
    E = 2.5 2^-24 (2 omax + |c|), omax = the largest coordinate of the frame under the counts;
  * the candidates are decided in ascending index by all lanes at once; strict < fills the hit mask and keeps the closest hit.

What can go wrong: a slot at or beyond the count that reaches the hit mask, the claim or the minimum (NaN, infinities, huge
values, the coordinates of a perfect hit); a count of 0, 1, 15 or 16; a blob at the gate dropped or kept on the wrong side of
the strict <; a blob the pre-test drops although its exact distance is inside the gate (|t32| next to thr, large coordinates
with a small gate); an omax taken from too few slots; equal coordinates in two slots (the claim by value), different blobs at
equal distance (the tie rule), hit lists of three and more, roots created at later cameras (stage 1), frames that take the
old chain.  Every case compares every bit of n_out, status, corr, xyz and err (mocap_core.devcheck.compare_bitwise) and n_cand
with the exhaustive walk on a second context, on both slot layouts, both rigs, with and without the float32 roundings, and
asserts the kernel that ran; the hand-built cases assert on the CPU, with the oracle's matching, that their frames are at the
edge they are named for.

Batches are a few hundred frames of 8 x 16; streams: seed 1, G_cap 2^20.
"""
import functools

import numpy as np
import pytest

import test_gpu_bb_eval_path as ep
from mocap_core import synth
from test_gpu_bb_eval_path import GATE, KERNELS, RIGS, _frames_with_n_prov, _search_equals, _to_dev, _walk, gpu  # noqa: F401
from test_gpu_bb_row_words import (C, LAYOUTS, M, _check, _clean, _equal_distance_frames, _ftab, _match, _rig, _steps, _stream,
                                   _with_copies)

pytestmark = pytest.mark.gpu

F_STREAM = 384
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 1. a seeded random stream

@pytest.mark.parametrize("K_max,f32", LAYOUTS)
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_random_stream_equals_the_walk(gpu, rig_name, K_max, f32):
    blobs, counts = _stream(rig_name, F_STREAM, M)
    _check(gpu, rig_name, blobs, counts, layouts=[(K_max, f32)], min_points=F_STREAM)


# ------------------------------------------------------------------------------------------------ 2. slots beyond the count, the counts' edges

def _first_root_hit(rig_name, bf, cf, cam):
    """The blob of camera `cam` that is the closest hit of the frame's first root, or None."""
    roots, hits = _match(rig_name, bf, cf)
    return hits[0][cam][0] if roots and hits[0][cam] else None


@functools.lru_cache(maxsize=None)
def _poisoned(rig_name):
    """256 frames of twelve markers whose slots at and beyond every camera's count hold, in turn, NaN, +inf, -inf, 1e30, the
    coordinates of a perfect hit (the closest hit of the frame's first root in that camera, copied) and a mix of them; every
    eighth frame has cameras cut down to 0, 1 and 15 blobs, and camera 5 of every frame of sixteen markers is full."""
    b12, c12 = (a.copy() for a in _stream(rig_name, 192, 12))
    b16, c16 = (a.copy() for a in _stream(rig_name, 64, M, dropout=0.0))
    blobs, counts = np.concatenate([b12, b16]), np.concatenate([c12, c16])
    fills = [np.nan, np.inf, -np.inf, 1e30, "hit", "mix"]
    n_hit = 0
    for f in range(blobs.shape[0]):
        if f % 8 == 3:
            counts[f, 2], counts[f, 4], counts[f, 6] = 0, min(counts[f, 4], 1), min(counts[f, 6], 15)
        fill = fills[f % len(fills)]
        for c in range(C):
            n = int(counts[f, c])
            if fill == "hit" or fill == "mix":
                k = _first_root_hit(rig_name, blobs[f], counts[f], c) if c and f < 48 else None
                good = blobs[f, c, k].copy() if k is not None else np.float32([1e30, -1e30])
                n_hit += k is not None
                blobs[f, c, n:] = good
                if fill == "mix":
                    blobs[f, c, n + 1::4] = np.nan
                    blobs[f, c, n + 2::4] = np.inf
                    blobs[f, c, n + 3::4, 0] = -np.inf
            else:
                blobs[f, c, n:] = fill
    assert n_hit >= 20                                                      # slots beyond a count that WOULD be hits
    assert {0, 1, 15, 16} <= set(np.unique(counts[:, 1:]).tolist())
    assert (counts[192:, 5] == M).all()
    blobs.setflags(write=False)
    counts.setflags(write=False)
    return blobs, counts


@pytest.mark.parametrize("K_max,f32", LAYOUTS)
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_slots_beyond_the_count_and_counts_of_0_1_15_16(gpu, rig_name, K_max, f32):
    blobs, counts = _poisoned(rig_name)
    _check(gpu, rig_name, blobs, counts, layouts=[(K_max, f32)], min_points=blobs.shape[0])


# ------------------------------------------------------------------------------------------------ 3. the gate and the pre-test's threshold

def _line_and_distances(rig_name, bf, root, cam, n):
    """The oracle's float32 line of `root` in camera `cam` and the distances of the camera's first n blobs (helpers.py:373)."""
    from oracle import mocap_oracle as mo
    a, b, c = mo.epiline(_ftab(rig_name)[root[0], cam], bf[root[0], root[1]])
    px, py = bf[cam, :n, 0].astype(np.float64), bf[cam, :n, 1].astype(np.float64)
    return (a, b, c), np.abs(a * px + b * py + c) / np.sqrt(a ** 2 + b ** 2)


def _single_hit_frame(rig_name, stage):
    """A clean frame (cameras before `stage` emptied) whose first root created at camera `stage` has one hit in camera stage + 1
    -> blobs, counts, root, the hit's index."""
    b0, c0 = _clean(rig_name)
    for f in range(b0.shape[0]):
        bf, cf = b0[f].copy(), c0[f].copy()
        cf[:stage] = 0
        roots, hits = _match(rig_name, bf, cf)
        mine = [r for r, (rc, _) in enumerate(roots) if rc == stage]
        if mine and len(hits[mine[0]][stage + 1]) == 1 and all(len(hits[mine[0]][c]) == 1 for c in range(stage + 1, C)):
            return bf, cf, roots[mine[0]], hits[mine[0]][stage + 1][0]
    raise AssertionError("no such frame")


@pytest.mark.parametrize("rig_name", list(RIGS))
@pytest.mark.parametrize("stage", [0, 1])
def test_a_blob_within_two_ulps_of_the_gate(gpu, rig_name, stage, monkeypatch):
    """The gate set to a hit's exact distance d moved by -2 .. +2 ulps: strict < keeps the blob for gate > d only.  The same few
    frames (the edge frame among clean ones) under five gates, all layouts."""
    from oracle import mocap_oracle as mo
    bf, cf, root, k = _single_hit_frame(rig_name, stage)
    cam = stage + 1
    _, d = _line_and_distances(rig_name, bf, root, cam, int(cf[cam]))
    b0, c0 = _clean(rig_name)
    blobs, counts = np.concatenate([np.stack([bf] * 4), b0[:28]]), np.concatenate([np.stack([cf] * 4), c0[:28]])
    for ulps in (-2, -1, 0, 1, 2):
        gate = float(d[k])
        for _ in range(abs(ulps)):
            gate = float(np.nextafter(gate, np.inf if ulps > 0 else 0.0))
        roots, hits = mo.match_frame(bf.astype(np.float64), cf, _ftab(rig_name), gate_px=gate)
        assert (k in hits[roots.index(root)][cam]) == (ulps > 0), (ulps, gate, d[k])
        monkeypatch.setattr(ep, "GATE", gate)
        _check(gpu, rig_name, blobs, counts, min_points=1)


def _fma32(a, x, c):
    """float32(a x + c) for float32 a, x, c: the product is exact in double (the sum's double rounding is far below what the
    assertions below resolve)."""
    return np.float32(np.float64(a) * np.float64(x) + np.float64(c))


@functools.lru_cache(maxsize=None)
def _threshold_frames(rig_name, stage):
    """Clean frames in which camera stage + 1 holds sixteen blobs next to the gate of the first root's line: the foot of the
    root's own hit moved along the line's normal to the distance GATE, then one coordinate stepped through sixteen neighbouring
    float32 values -- distances a few 1e-5 px apart on either side of the gate and, beyond it, on either side of the pre-test's
    threshold (E is a few 1e-4 px here).  -> blobs, counts, per frame (|t32| - thr) / E and d - GATE of the sixteen blobs."""
    b0, c0 = _clean(rig_name)
    cam = stage + 1
    got_b, got_c, rel, dd = [], [], [], []
    for f in range(b0.shape[0]):
        bf, cf = b0[f].copy(), c0[f].copy()
        cf[:stage] = 0
        roots, hits = _match(rig_name, bf, cf)
        mine = [r for r, (rc, _) in enumerate(roots) if rc == stage]
        if not mine or len(hits[mine[0]][cam]) != 1:
            continue
        root = roots[mine[0]]
        (a, b, c), _ = _line_and_distances(rig_name, bf, root, cam, int(cf[cam]))
        den = np.sqrt(a ** 2 + b ** 2)
        hit = bf[cam, hits[mine[0]][cam][0]].astype(np.float64)
        s = (a * hit[0] + b * hit[1] + c) / den
        side = 1.0 if s >= 0 else -1.0
        p = hit + (side * GATE - s) * np.array([a, b]) / den                 # at the distance GATE, on the hit's side of the line
        ax = 0 if abs(a) >= abs(b) else 1                                    # the coordinate the distance is most sensitive to
        q0 = np.float32(p)
        pts = []
        for j in range(-8, 8):
            q = q0.copy()
            for _ in range(abs(j)):
                q[ax] = np.nextafter(q[ax], np.float32(np.inf if j > 0 else -np.inf))
            pts.append(q)
        bf[cam, :M] = np.stack(pts)
        cf[cam] = M
        omax = max(float(np.abs(bf[i, :cf[i]]).max()) for i in range(C) if cf[i])
        E = 2.5 * U24 * (2.0 * omax + abs(c))
        thr = GATE * den * (1 + 1e-12) + E * (1 + 1e-6)
        a32, b32, c32 = np.float32(a), np.float32(b), np.float32(c)
        t32 = np.array([abs(float(_fma32(a32, q[0], _fma32(b32, q[1], c32)))) for q in pts])
        _, d = _line_and_distances(rig_name, bf, root, cam, M)
        roots2, hits2 = _match(rig_name, bf, cf)
        if root not in roots2:
            continue
        assert sorted(hits2[roots2.index(root)][cam]) == [k for k in range(M) if d[k] < GATE]
        got_b.append(bf)
        got_c.append(cf)
        rel.append((t32 - thr) / E)
        dd.append(d - GATE)
        if len(got_b) == 12:
            break
    assert len(got_b) >= 4
    return np.stack(got_b), np.stack(got_c), np.array(rel), np.array(dd)


@pytest.mark.parametrize("rig_name", list(RIGS))
@pytest.mark.parametrize("stage", [0, 1])
def test_blobs_next_to_the_gate_and_to_the_pre_test_threshold(gpu, rig_name, stage):
    blobs, counts, rel, dd = _threshold_frames(rig_name, stage)
    assert (dd < 0).any() and (dd >= 0).any() and np.abs(dd).min() < 5e-5      # hits and misses a few float32 steps from the gate
    assert ((rel > -1) & (rel <= 0)).any() and ((rel > 0) & (rel < 1)).any()  # |t32| within E of thr, on either side
    assert ((rel <= 0) & (dd >= 0)).any()                                     # blobs the pre-test passes and the exact test drops
    _check(gpu, rig_name, blobs, counts, min_points=1)


# ------------------------------------------------------------------------------------------------ 4. claims, ties, long lists, later roots, the old chain

@functools.lru_cache(maxsize=None)
def _hand_built(rig_name):
    """One batch: equal coordinates in two slots, different blobs at equal distance (as the closest hit and behind it), hit lists
    of 3 and 5, each for a camera-0 root (stage 0) and a root created at camera 1 (stage 1); a camera with sixteen hits; frames
    whose camera 0 sees nothing (six markers: 42 provisional roots, more than the 48-slot layout stages -- the old chain);
    frames with 65 provisional roots (the old chain on every layout); roots created at cameras 3 and 6."""
    parts = []
    for stage in (0, 1):
        parts.append(_with_copies(rig_name, [stage + 1], [(np.float32(0.0), np.float32(0.0))], root_cam=stage, want=4)[:2])
        parts.append(_with_copies(rig_name, [stage + 1], _steps(2, 0.5), root_cam=stage, want=4)[:2])
        parts.append(_with_copies(rig_name, [stage + 1], _steps(4, 0.5), root_cam=stage, want=4)[:2])
        parts.append(_equal_distance_frames(rig_name, 0.0, stage)[:2])
        parts.append(_equal_distance_frames(rig_name, 3.0, stage)[:2])
    parts.append(_with_copies(rig_name, [4], _steps(15), want=4)[:2])
    b6, c6, _ = synth.make_blob_stream(_rig(rig_name), 8, 6, seed=1, m_max=M, dropout=0.0)
    c6 = c6.copy()
    c6[:, 0] = 0
    assert (c6[:, 1:].sum(axis=1) > 40).all()
    for f in range(2):
        roots, _ = _match(rig_name, b6[f], c6[f])
        assert ep.n_provisional(_ftab(rig_name), b6[f], c6[f]) == int(c6[f].sum()) and 0 < len(roots) <= 48   # every blob is provisional
    parts.append((b6, c6))
    parts.append(_frames_with_n_prov(_rig(rig_name), C, M, 65))
    b12, c12 = (a.copy() for a in _stream(rig_name, 64, 12))
    c12[0::2, :3] = 0
    c12[1::2, :6] = 0
    for f in range(4):
        roots, hits = _match(rig_name, b12[f], c12[f])
        first = 3 if f % 2 == 0 else 6
        assert roots and roots[0][0] == first and any(rc == first and any(hr) for (rc, _), hr in zip(roots, hits)), f
    parts.append((b12, c12))
    blobs, counts = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    blobs.setflags(write=False)
    counts.setflags(write=False)
    return blobs, counts


@pytest.mark.parametrize("K_max,f32", LAYOUTS)
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_claims_ties_long_lists_later_roots_and_the_old_chain(gpu, rig_name, K_max, f32):
    blobs, counts = _hand_built(rig_name)
    _check(gpu, rig_name, blobs, counts, layouts=[(K_max, f32)], min_points=blobs.shape[0] // 2)


# ------------------------------------------------------------------------------------------------ 5. large coordinates, small gate

@pytest.mark.parametrize("K_max,f32", LAYOUTS)
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_coordinates_up_to_16000_px_with_a_half_pixel_gate(gpu, rig_name, K_max, f32, monkeypatch):
    """The 16 k-pixel sensor of the stress rig on eight cameras, gate 0.5 px, no pixel truncation (a marker's blobs lie within the
    noise of its lines): omax is large, E is 1 % of the gate's width and the float32 test passes blobs the exact one drops."""
    dev, _ = gpu
    kw = dict(K=synth.STRESS_K, image_size=(16000, 16000))
    rig = synth.ring_rig(C, **kw) if rig_name == "identical K" else synth.calibrated_ring_rig(C, 1, **kw)
    blobs, counts, _ = synth.make_blob_stream(rig, 256, 12, seed=1, m_max=M, noise_px=0.15, truncate=False)
    assert float(np.nanmax(blobs)) > 12000.0
    monkeypatch.setattr(ep, "GATE", 0.5)
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, C, M, K_max, d_b, d_c, min_points=128, f32=f32)
    _search_equals(gpu, rig, ref, M, d_b, d_c, KERNELS[rig_name] % 1, f32=f32)
