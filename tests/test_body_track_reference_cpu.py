"""The body tracker's reference (tests/body_track_reference.py) on its own, no GPU: the seven symbols of the "body tracker"
section, chunk invariance, what the tracker is for (a symmetric body keeps its labelling, a body with two visible markers
coasts and is retired, three of five markers are enough) and the margins every scene of the GPU tests must keep."""
import os
import re
import subprocess

import numpy as np
import pytest

import body_track_reference as br
from conftest import ROOT

SYMBOLS = ["mocap_set_body_tracker", "mocap_reset_body_tracker", "mocap_track_bodies", "mocap_track_bodies_dev",
           "mocap_get_body_tracks", "mocap_track_frame_bodies_tracked", "mocap_track_frame_bodies_tracked_dev"]
OUT_KEYS = ("tracked", "source", "n_used", "assign", "R", "t", "rms", "hits", "missed", "status")


def test_the_seven_symbols_are_declared_exported_and_bound():
    from mocap_core import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mocap_core.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mocap_[a-z_0-9]+)\s*\(", text))
    lib = capi.load_library()
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert name in declared, name
        assert name in capi.SIGNATURES, name
        assert getattr(lib, name) is not None
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(capi.SIGNATURES[name][1]) == len(args.split(",")), name     # as many arguments as the declaration lists
    assert (capi.BT_SRC_NONE, capi.BT_SRC_GUIDED, capi.BT_SRC_SEARCH, capi.BT_SRC_COAST) == \
        (br.SRC_NONE, br.SRC_GUIDED, br.SRC_SEARCH, br.SRC_COAST) == (0, 1, 2, 3)
    assert capi.BT_ST_BAD_TIME == br.ST_BAD_TIME == 1
    for name, value in (("MOCAP_BT_SRC_NONE", 0), ("MOCAP_BT_SRC_GUIDED", 1), ("MOCAP_BT_SRC_SEARCH", 2), ("MOCAP_BT_SRC_COAST", 3),
                        ("MOCAP_BT_ST_BAD_TIME", 1)):
        assert re.search(name + r"\s*=\s*%d\b" % value, text), name
    for method in ("set_body_tracker", "reset_body_tracker", "track_bodies", "track_bodies_dev", "get_body_tracks",
                   "track_frame_bodies_tracked", "track_frame_bodies_tracked_dev"):
        assert callable(getattr(capi.MocapCore, method)), method
    from mocap_core import helpers
    for fn in ("set_body_tracker", "track_bodies", "track_frame_bodies_tracked"):
        assert callable(getattr(helpers, fn)), fn


def _same(a, b):
    for k in OUT_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", ["planted1", "occlusion"])
def test_the_reference_is_chunk_invariant(name):
    s = br.scene(name)
    F = len(s["t"])
    for cuts in ([1, F - 1], [F // 2, F - F // 2], [1] * F):
        trk = br.Tracker(s["bodies"], br.TOL, br.MAX_RMS, *s["settings"])
        parts, f = [], 0
        for L in cuts:
            parts.append(trk.run(s["t"][f:f + L], s["xyz"][f:f + L], s["n_pts"][f:f + L]))
            f += L
        _same({k: np.concatenate([p[k] for p in parts]) for k in OUT_KEYS}, s["ref"])
        st = trk.state()
        for k, v in s["ref_state"].items():
            assert st[k].tobytes() == v.tobytes(), k


def test_the_search_flips_on_a_symmetric_body_and_the_tracker_does_not():
    s = br.scene("symmetric")
    F, truth = 120, s["truth"]["assign"]
    assert (s["n_pts"] == 15).all() and (truth[:, 0, :5] >= 0).all()           # all five markers visible, ten clutter points
    found, assign = br.search_labels(s["xyz"], s["n_pts"], s["bodies"], br.TOL, br.MAX_RMS)
    lab = [br.labelling(assign[f, 0], truth[f, 0], 5) if found[f, 0] else None for f in range(F)]
    flips = sum(lab[f] is not None and lab[f - 1] is not None and lab[f] != lab[f - 1] for f in range(1, F))
    print(f"per-frame search: found in {int(found.sum())} of {F} frames, labelling changed between two found frames {flips} times")
    assert flips >= 20
    r = s["ref"]
    assert r["tracked"][:, 0].all() and r["source"][0, 0] == br.SRC_SEARCH and (r["source"][1:, 0] == br.SRC_GUIDED).all()
    assert (r["n_used"][:, 0] == 5).all()
    tl = {br.labelling(r["assign"][f, 0], truth[f, 0], 5) for f in range(F)}
    assert len(tl) == 1 and -1 not in next(iter(tl)), tl                        # one labelling, all of the body's own points
    assert r["hits"][:, 0].tolist() == list(range(1, F + 1))


def test_two_visible_markers_coast_for_max_missed_frames_and_then_nothing():
    s = br.scene("occlusion")
    r, mm = s["ref"], s["settings"][1]
    assert mm == 5
    src = r["source"][:, 0].tolist()
    assert src[0] == br.SRC_SEARCH and set(src[1:20]) == {br.SRC_GUIDED}
    assert src[20:25] == [br.SRC_COAST] * 5 and r["missed"][20:25, 0].tolist() == [1, 2, 3, 4, 5]
    assert src[25:29] == [br.SRC_NONE] * 4 and not r["tracked"][25:29, 0].any()
    assert src[29] == br.SRC_SEARCH and r["hits"][29, 0] == 1 and set(src[30:]) == {br.SRC_GUIDED}
    # a coasting frame carries the held orientation, the extrapolated position and no markers
    assert (r["assign"][20:25, 0] == -1).all() and not r["n_used"][20:25, 0].any() and not r["rms"][20:25, 0].any()
    assert all(r["R"][f, 0].tobytes() == r["R"][19, 0].tobytes() for f in range(20, 25))
    step = np.diff(r["t"][19:25, 0], axis=0)
    assert np.abs(step - step[0]).max() < 1e-12 and np.abs(step[0]).max() > 1e-3      # p + v dt: equal steps at 60 Hz
    # everything beyond the body's own slot and the retired frames is zero
    for k in OUT_KEYS[:-1]:
        assert not r[k][25:29].any(), k


def test_three_of_five_markers_are_guided():
    rng = np.random.default_rng(11)
    body = br.make_body(rng, 5)
    vis = np.ones((12, 1, 8), dtype=bool)
    vis[4:, 0, [1, 3]] = False
    t, xyz, n_pts, truth = br.path_scene(rng, [body], 12, 16, 6, br._PATHS[:1], visible=vis)
    trk = br.Tracker([body], br.TOL, br.MAX_RMS, 0.03, 10, 0.5)
    r = trk.run(t, xyz, n_pts)
    assert br.posable_table(body)[0b10101]
    assert (r["source"][4:, 0] == br.SRC_GUIDED).all() and (r["n_used"][4:, 0] == 3).all()
    assert (r["assign"][4:, 0, [1, 3]] == -1).all()
    for f in range(4, 12):
        assert br.labelling(r["assign"][f, 0], truth["assign"][f, 0], 5) == (0, -1, 2, -1, 4)


@pytest.mark.parametrize("name", br.SCENES)
def test_every_scene_of_the_gpu_tests_keeps_its_margins(name):
    """No d2 within 1e-9 relative of g2, no two pair keys of one association within 1e-9 relative, no rms within 1e-9 relative
    of max_rms: an assignment cannot turn on the last bits in which the device's Horn / Jacobi pose and the reference's SVD pose
    differ."""
    s = br.scene(name)
    print(name, s["margin"])
    assert s["margins_ok"], s["margin"]
    assert all(v > br.MARGIN for v in s["margin"].values())


def test_what_each_gpu_scene_is_there_for():
    r = br.scene("planted1")["ref"]
    assert (r["source"] == br.SRC_COAST).any() and (r["n_used"][r["source"] == br.SRC_GUIDED] < 5).any()    # hidden markers
    r = br.scene("planted3")["ref"]
    assert r["tracked"].all() and {br.SRC_GUIDED, br.SRC_SEARCH} <= set(r["source"].ravel().tolist())
    s = br.scene("identical")
    r, truth = s["ref"], s["truth"]["assign"]
    for b in range(2):       # each copy keeps its own points through the pass
        assert {br.labelling(r["assign"][f, b], truth[f, b], 5) for f in range(90)} == {(0, 1, 2, 3, 4)}
    assert (br.scene("full64")["n_pts"] == 64).all()
    r = br.scene("eight")["ref"]
    assert r["tracked"].shape == (12, 8) and r["tracked"].all()
