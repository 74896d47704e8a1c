"""The marker tracker's reference (tests/marker_track_reference.py) on its own, no GPU: hand-computed frames, the two statements
of the association against each other, chunk invariance, and the seven symbols of the "marker tracker" section."""
import os
import re

import numpy as np
import pytest

import marker_track_reference as mt
from conftest import ROOT

SYMBOLS = ["mocap_set_marker_tracker", "mocap_reset_marker_tracker", "mocap_track_markers", "mocap_track_markers_dev",
           "mocap_get_marker_tracks", "mocap_track_frame_ids", "mocap_track_frame_ids_dev"]
PLANTED = [(20, 32, 3, 1), (40, 64, 3, 11), (5, 8, 1, 12)]      # (markers, K_max, clutter per frame, seed)
CROWDED = [(64, 64, 64, 3), (30, 32, 20, 4), (12, 16, 64, 5)]   # (points, K_max, T_max, seed)


def _frame(*pts, K=4):
    xyz = np.full((K, 3), 1e6)
    xyz[:len(pts)] = pts
    return xyz, len(pts)


def test_hand_computed_frames_birth_match_coast_retire_reuse():
    tr = mt.Tracker(gate=0.05, max_missed=1, vel_alpha=0.5, T_max=3)
    # frame 0: two births, in point order
    i, h, n, s = tr.step(10.0, *_frame([0.0, 0.0, 0.0], [1.0, 0.0, 0.0]))
    assert i.tolist() == [0, 1, -1, -1] and h.tolist() == [1, 1, 0, 0] and (n, s) == (2, 0) and tr.next_id == 2
    # frame 1 (dt = 0.5): both matched, in swapped order; v = 0 + 0.5 * ((x - p) / 0.5 - 0)
    i, h, n, s = tr.step(10.5, *_frame([1.0, 0.01, 0.0], [0.02, 0.0, 0.0]))
    assert i.tolist() == [1, 0, -1, -1] and h.tolist() == [2, 2, 0, 0] and (n, s) == (2, 0)
    assert tr.v[0].tolist() == [0.5 * (0.02 / 0.5), 0.0, 0.0] and tr.v[1].tolist() == [0.0, 0.5 * (0.01 / 0.5), 0.0]
    assert tr.p[0].tolist() == [0.02, 0.0, 0.0] and tr.t_seen.tolist()[:2] == [10.5, 10.5]
    # frame 2 (dt = 0.5): track 0 is predicted at 0.02 + 0.02 * 0.5 = 0.03; the point at 0.07 is inside the gate of the
    # prediction (0.04) and would be outside the gate of the last position (0.05 is not < 0.05).  Track 1 coasts.
    i, h, n, s = tr.step(11.0, *_frame([0.07, 0.0, 0.0]))
    assert i.tolist() == [0, -1, -1, -1] and h.tolist() == [3, 0, 0, 0] and (n, s) == (2, 0)
    assert tr.missed.tolist()[:2] == [0, 1] and tr.t_seen[1] == 10.5 and tr.p[1].tolist() == [1.0, 0.01, 0.0]
    u = (0.07 - 0.02) / 0.5
    assert tr.v[0, 0] == 0.02 + 0.5 * (u - 0.02)
    # frame 3: track 1 unseen a second time: missed 2 > max_missed 1, retired; its slot is free for THIS frame's birth, which
    # takes the lowest free slot (1, not 2) and the next id
    i, h, n, s = tr.step(11.5, *_frame([5.0, 5.0, 5.0]))
    assert i.tolist() == [2, -1, -1, -1] and h.tolist() == [1, 0, 0, 0] and (n, s) == (2, 0)     # track 0 coasts (missed 1)
    assert tr.slots().tolist() == [0, 1] and tr.id.tolist()[:2] == [0, 2] and tr.v[1].tolist() == [0.0, 0.0, 0.0]
    # frame 4: track 0 is retired (missed 2 > 1), so slots 0 and 2 are free for three unmatched points: the third finds none
    i, h, n, s = tr.step(12.0, *_frame([5.0, 5.0, 5.0], [7.0, 7.0, 7.0], [8.0, 8.0, 8.0], [9.0, 9.0, 9.0]))
    assert i.tolist() == [2, 3, 4, -1] and h.tolist() == [2, 1, 1, 0] and (n, s) == (3, mt.ST_FULL) and tr.next_id == 5
    assert tr.id.tolist() == [3, 2, 4]          # slot 0 (retired this frame) before slot 2
    # a non-finite time stamp: nothing but the status
    before = {k: v.copy() for k, v in tr.tracks().items()}
    i, h, n, s = tr.step(float("nan"), *_frame([5.0, 5.0, 5.0]))
    assert i.tolist() == [-1] * 4 and not h.any() and (n, s) == (0, mt.ST_BAD_TIME)
    assert all(before[k].tobytes() == v.tobytes() for k, v in tr.tracks().items())


def _both(t, xyz, n_pts, **kw):
    a, b = mt.Tracker(**kw), mt.Tracker(associate=mt.associate_rounds, **kw)
    return a, a.run(t, xyz, n_pts), b, b.run(t, xyz, n_pts)


def _same(oa, ob, a, b):
    for k in oa:
        assert np.array_equal(oa[k], ob[k]), k
    ta, tb = a.tracks(), b.tracks()
    for k in ta:
        assert ta[k].tobytes() == tb[k].tobytes(), k
    assert a.next_id == b.next_id


@pytest.mark.parametrize("case", PLANTED)
def test_rounds_equal_the_sorted_list_on_the_planted_scenes(case):
    markers, K_max, clutter, seed = case
    t, xyz, n_pts, truth = mt.planted_scene(markers, K_max, clutter, seed)
    a, oa, b, ob = _both(t, xyz, n_pts, **mt.DEFAULTS)
    _same(oa, ob, a, b)
    assert mt.id_switches(oa["id"], truth) == 0 and not (oa["mk_status"] & mt.ST_FULL).any()
    assert max(b.rounds) >= 1


@pytest.mark.parametrize("case", CROWDED)
def test_rounds_equal_the_sorted_list_where_many_rounds_are_needed(case):
    points, K_max, T_max, seed = case
    t, xyz, n_pts = mt.crowded_scene(points, K_max, seed)
    a, oa, b, ob = _both(t, xyz, n_pts, gate=0.05, max_missed=2, vel_alpha=0.5, T_max=T_max)
    _same(oa, ob, a, b)
    assert max(b.rounds) >= 3


def test_crossing_swaps_without_velocity_and_not_with_it():
    t, xyz, n_pts = mt.crossing_scene()
    for alpha, last in ((0.0, [1, 0]), (0.5, [0, 1]), (1.0, [0, 1])):
        a, oa, b, ob = _both(t, xyz, n_pts, gate=0.05, max_missed=5, vel_alpha=alpha, T_max=64)
        _same(oa, ob, a, b)
        assert oa["id"][0].tolist() == [0, 1] and oa["id"][-1].tolist() == last, alpha
        assert (oa["n_tracks"] == 2).all()


def test_chunk_invariance():
    t, xyz, n_pts, _ = mt.planted_scene(20, 32, 3, 1)
    whole = mt.Tracker(**mt.DEFAULTS)
    ow = whole.run(t, xyz, n_pts)
    cut = mt.Tracker(**mt.DEFAULTS)
    parts, f = [], 0
    for L in (1, 7, 64, len(t)):
        parts.append(cut.run(t[f:f + L], xyz[f:f + L], n_pts[f:f + L]))
        f += L
    for k in ow:
        assert np.array_equal(np.concatenate([p[k] for p in parts]), ow[k]), k
    for k, v in whole.tracks().items():
        assert cut.tracks()[k].tobytes() == v.tobytes(), k


def test_validate():
    assert mt.validate(**mt.DEFAULTS) is None
    for kw in (dict(gate=0.0), dict(gate=float("inf")), dict(gate=float("nan")), dict(max_missed=-1), dict(vel_alpha=-0.1),
               dict(vel_alpha=1.5), dict(vel_alpha=float("nan")), dict(T_max=65), dict(T_max=0)):
        assert mt.validate(**{**mt.DEFAULTS, **kw}) is not None, kw


def test_the_seven_symbols_are_declared_and_bound():
    from mocap_core import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mocap_core.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mocap_[a-z_0-9]+)\s*\(", text))
    lib = capi.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in capi.SIGNATURES, name
        assert getattr(lib, name) is not None
    # the binding takes as many arguments as the declaration lists
    for name in SYMBOLS:
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(capi.SIGNATURES[name][1]) == len(args.split(",")), name
    assert (capi.MT_ST_FULL, capi.MT_ST_BAD_TIME, capi.MT_MAX_TRACKS, capi.MT_MAX_POINTS) == (mt.ST_FULL, mt.ST_BAD_TIME, 64, 64)
    for name, value in (("MOCAP_MT_ST_FULL", 1), ("MOCAP_MT_ST_BAD_TIME", 2)):
        assert re.search(name + r"\s*=\s*%d\b" % value, text), name
