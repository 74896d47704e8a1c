"""GPU: the heavy-root search and its enumeration (csrc/heavy_bb.hip: heavy_bb_calib_kernel, heavy_enum_calib_kernel) on rigs
with one plain intrinsic matrix PER CAMERA, as a calibration gives them -- what tests/test_gpu_wide_adversarial.py checks on
the identical-K stress rig, on synth.calibrated_stress_rig:
  * two markers behind each other as seen from camera 0 (2^60 groups per root): solved by the re-submit;
  * search = enumeration bit for bit where the enumeration is feasible, through the default frontier, a frontier of 64 nodes
    (in-place fall-back) and a frontier of one node without fall-back (heavy_enum_calib_kernel); the bounded variant;
  * the re-submit against the C oracle;
  * the position rule (helpers.py:305-307: a view takes the intrinsics of its camera's POSITION among the cameras the group
    sees): hand-made frames whose heavy roots have lower cameras without a hit and roots created after camera 0."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDE = ("frame_kernel<512, wide>", "frame_kernel<1024, wide>")


def _with_env(env, fn):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def test_two_markers_behind_each_other_on_the_calibrated_rig(core):
    """The construction of test_gpu_wide_adversarial.py::test_two_markers_behind_each_other_as_seen_from_camera_0 on the
    calibrated stress rig: marker B on camera 0's ray through marker A, two hits per camera, 2^60 groups per root.  The
    re-submit solves all four frames: both roots of the pair carry ONE marker's blobs in all 63 other cameras and that
    marker's position to 5e-5 (the existing test's tolerance on the same construction)."""
    from mocap_core import capi, synth
    rig = synth.calibrated_stress_rig(64)
    assert not np.array_equal(rig["K"][0], rig["K"][1])

    def behind(w):
        w = w.copy()
        for f in range(w.shape[0]):
            a0 = w[f, 0] @ rig["R0"].T + rig["centre"]                 # marker 0 in camera-0 coordinates (camera 0 at the origin)
            w[f, 1] = (a0 * (1.15 + 0.05 * f) - rig["centre"]) @ rig["R0"]   # marker 1 further out on the same ray
        return w

    blobs, counts, truth = synth.make_blob_stream(rig, 4, 256, seed=5, noise_px=0.02, dropout=0.0, half_extent=1.5, min_sep=0.05,
                                                  truncate=False, world=behind)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    plain = core.match_triangulate(blobs, counts, gate_px=synth.STRESS_GATE_PX, K_max=384, G_cap=1 << 24)
    assert core.last_frame_kernel() in WIDE, core.last_frame_kernel()
    assert (plain["status"] & capi.ST_CAND_OVERFLOW).all()
    auto = core.match_triangulate_auto(blobs, counts, gate_px=synth.STRESS_GATE_PX, K_max=384, G_cap=1 << 20)
    print("status", auto["status"].tolist(), "resubmitted", auto["resubmitted"], "n_out", auto["n_out"].tolist())
    assert auto["resubmitted"] == 4 and not auto["status"].any(), auto["status"]
    X0 = truth["points_cam0"]
    for f in range(4):
        n = int(auto["n_out"][f])
        assert n >= 250
        found = 0
        for k in range(n):
            k0 = auto["corr"][f, k, 0]
            if k0 < 0 or int(truth["ident"][f, 0, k0]) not in (0, 1):
                continue                                              # (the two camera-0 roots of the pair are what is tested)
            ids = {int(truth["ident"][f, c, auto["corr"][f, k, c]]) for c in range(1, 64) if auto["corr"][f, k, c] >= 0}
            assert len(ids) == 1 and ids <= {0, 1}, (f, k, ids)        # one marker's blobs, never a mixture
            assert (auto["corr"][f, k] >= 0).sum() == 64
            mk = ids.pop()
            print("frame", f, "root", k, "marker", mk, "|xyz - truth|", np.abs(auto["xyz"][f, k] - X0[f, mk]).max())
            np.testing.assert_allclose(auto["xyz"][f, k], X0[f, mk], atol=5e-5)
            found += 1
        assert found == 2


def test_heavy_root_search_equals_the_enumeration_on_the_calibrated_rig(core):
    """heavy_bb_calib_kernel / heavy_enum_calib_kernel against the enumeration, root by root, where the enumeration is feasible
    (the legs of test_gpu_wide_adversarial.py::test_heavy_root_search_equals_the_enumeration).  Seed 77: the first of 77, 78, ...
    for which the C oracle alone (G_cap = 2^20) finishes at least 20 of the 24 frames -- it finishes 24 of 24."""
    from mocap_core import capi, synth
    rig = synth.calibrated_stress_rig(64)
    blobs, counts, _ = synth.make_stress_stream(rig, 24, 256, seed=77)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    plain = core.match_triangulate(blobs, counts, gate_px=synth.STRESS_GATE_PX, K_max=384, G_cap=1 << 20)
    assert core.last_frame_kernel() in WIDE, core.last_frame_kernel()
    ok = plain["status"] == 0
    print("plain call finishes", int(ok.sum()), "of 24")
    assert ok.sum() >= 20
    valid = (np.arange(384)[None, :] < plain["n_out"][:, None]) & ok[:, None]

    def resubmit():
        return core.match_triangulate_auto(blobs, counts, gate_px=synth.STRESS_GATE_PX, K_max=384, G_cap=1)

    legs = ({}, {"MOCAP_HEAVY_NCAP": "64"}, {"MOCAP_HEAVY_NCAP": "1", "MOCAP_HEAVY_ENUM_CAP": "0"})
    for leg in legs:
        auto = _with_env(dict(leg, MOCAP_RESUBMIT_G_CAP="8"), resubmit)
        print(leg, "resubmitted", auto["resubmitted"], "flagged", int((auto["status"] != 0).sum()),
              "frames with fewer candidates", int((auto["n_cand"][ok] < plain["n_cand"][ok]).sum()))
        assert auto["resubmitted"] >= 20 and not auto["status"][ok].any(), leg
        assert np.array_equal(auto["n_out"][ok], plain["n_out"][ok]), leg
        assert np.array_equal(auto["corr"][valid], plain["corr"][valid]), leg
        assert np.array_equal(auto["xyz"][valid], plain["xyz"][valid]) and np.array_equal(auto["err"][valid], plain["err"][valid]), leg
        assert (auto["n_cand"][ok] < plain["n_cand"][ok]).any(), leg        # the search did run: its roots count one candidate each
    # MOCAP_OPT_BOUNDED_RESUBMIT with the third leg's settings: the forced give-ups are NOT enumerated, their frames stay flagged
    # (candidate overflow + FINAL, not INTRACTABLE: fewer than 2^24 groups) without a point; every frame that is returned is exact
    try:
        core.set_options(bounded_resubmit=True)
        bounded = _with_env(dict(legs[2], MOCAP_RESUBMIT_G_CAP="8"), resubmit)
    finally:
        core.set_options(bounded_resubmit=False)
    left = bounded["status"] != 0
    print("bounded: frames left flagged", int(left.sum()), "status", sorted(set(bounded["status"][left].tolist())))
    want = capi.ST_CAND_OVERFLOW | capi.ST_FINAL
    assert left.any() and (bounded["status"][left] & (want | capi.ST_INTRACTABLE) == want).all()
    assert not bounded["n_out"][left].any()
    done = ok & ~left
    v3 = (np.arange(384)[None, :] < plain["n_out"][:, None]) & done[:, None]
    assert np.array_equal(bounded["n_out"][done], plain["n_out"][done])
    assert np.array_equal(bounded["corr"][v3], plain["corr"][v3])
    assert np.array_equal(bounded["xyz"][v3], plain["xyz"][v3]) and np.array_equal(bounded["err"][v3], plain["err"][v3])


def test_resubmit_on_the_calibrated_rig_vs_c_oracle(core):
    """The frames of the oracle comparison in test_candidate_cap_overflow_at_the_stress_shape_is_resubmitted (12 frames, seed 31)
    on the calibrated rig: correspondences exact, points to rtol 1e-9 / atol 1e-12 (that comparison's figures).  Roots above
    4 096 groups go through the search here."""
    from mocap_core import capi, synth
    from oracle import c_oracle
    rig = synth.calibrated_stress_rig(64)
    blobs, counts, _ = synth.make_stress_stream(rig, 12, 256, seed=31)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    tight = core.match_triangulate(blobs, counts, gate_px=synth.STRESS_GATE_PX, K_max=384, G_cap=2)
    assert core.last_frame_kernel() in WIDE
    assert (tight["status"] & capi.ST_CAND_OVERFLOW).all() and not tight["n_out"].any()
    auto = core.match_triangulate_auto(blobs, counts, gate_px=synth.STRESS_GATE_PX, K_max=384, G_cap=2)
    ref = c_oracle.COracle(rig["K"], rig["R"], rig["t"]).match_triangulate(blobs, counts, gate_px=synth.STRESS_GATE_PX, K_max=384,
                                                                           G_cap=1 << 20)
    ok = ref["status"] == 0         # (a frame with a root of more than 2^20 groups is left to the core alone: minutes on the CPU)
    print("oracle finishes", int(ok.sum()), "of 12; status", auto["status"].tolist())
    assert auto["resubmitted"] == 12 and ok.sum() >= 10 and not auto["status"][ok].any()
    assert np.array_equal(auto["n_out"][ok], ref["n_out"][ok])
    assert (auto["n_cand"][ok] <= ref["n_cand"][ok]).all()
    valid = (np.arange(384)[None, :] < ref["n_out"][:, None]) & ok[:, None]
    assert np.array_equal(auto["corr"][valid], ref["corr"][valid])
    print("max |xyz - oracle|", np.abs(auto["xyz"][valid] - ref["xyz"][valid]).max())
    np.testing.assert_allclose(auto["xyz"][valid], ref["xyz"][valid], rtol=1e-9, atol=1e-12)


def position_rule_frames():
    """(rig, blobs, counts, truth): six hand-made frames of 8 calibrated cameras x 6 markers.  Marker 1 lies behind marker 0 as
    seen from camera cb (two hits in every later camera for either root: a heavy root once the candidate cap is 1), and both
    markers' blobs are taken out of some cameras:
      frame  cb  removed from   what the pair's roots look like
        0    0   --             camera-0 roots, every camera seen: position = camera
        1    0   1, 2           camera-0 roots, cameras 1 and 2 without a hit: position = camera - 2 from camera 3 on
        2    0   4              ... a gap in the middle
        3    2   0, 1           roots created at camera 2: position = camera - 2
        4    2   0, 1, 4        ... with a gap behind the root's camera
        5    1   0, 3, 6        roots created at camera 1, two gaps"""
    from mocap_core import synth
    rig = synth.calibrated_ring_rig(8, seed=3)
    plan = [(0, ()), (0, (1, 2)), (0, (4,)), (2, (0, 1)), (2, (0, 1, 4)), (1, (0, 3, 6))]

    def behind(w):
        w = w.copy()
        for f, (cb, _) in enumerate(plan):
            a0 = w[f, 0] @ rig["R0"].T + rig["centre"]                       # marker 0 in camera-0 coordinates
            o = -rig["R"][cb].T @ rig["t"][cb]                               # centre of camera cb in camera-0 coordinates
            w[f, 1] = (o + 1.2 * (a0 - o) - rig["centre"]) @ rig["R0"]       # marker 1 further out on camera cb's ray
        return w

    blobs, counts, truth = synth.make_blob_stream(rig, len(plan), 6, seed=11, noise_px=0.05, dropout=0.0, half_extent=0.6, min_sep=0.25,
                                                  truncate=False, world=behind)
    ident = truth["ident"].copy()
    for f, (_, gone) in enumerate(plan):
        for cam in gone:
            for mk in (0, 1):
                k = int(np.nonzero(ident[f, cam] == mk)[0][0])
                n = int(counts[f, cam])
                blobs[f, cam, k:n - 1] = blobs[f, cam, k + 1:n]
                ident[f, cam, k:n - 1] = ident[f, cam, k + 1:n]
                blobs[f, cam, n - 1] = np.nan
                ident[f, cam, n - 1] = -1
                counts[f, cam] = n - 1
    return rig, blobs, counts, {"points_cam0": truth["points_cam0"], "ident": ident, "plan": plan}


def check_position_rule_frames(rig, blobs, counts, truth, ref):
    """The frames are what their table says (on the oracle's result: no GPU needed): per frame the pair's two roots start at
    camera cb, see no removed camera, and had a choice (more candidates than points)."""
    for f, (cb, gone) in enumerate(truth["plan"]):
        n = int(ref["n_out"][f])
        assert ref["status"][f] == 0 and ref["n_cand"][f] >= n + 2 * (2 ** (7 - cb - len([g for g in gone if g > cb])) - 1), (f, ref["n_cand"][f], n)
        pair = 0
        for k in range(n):
            row = ref["corr"][f, k]
            first = int(np.nonzero(row >= 0)[0][0])
            if first != cb or int(truth["ident"][f, first, row[first]]) not in (0, 1):
                continue                    # (a blob of the pair no root claimed becomes a root of its own at a later camera)
            pair += 1
            # no blob of the pair in a removed camera (another marker's blob may sit inside the gate there by chance) ...
            assert all(row[g] < 0 or int(truth["ident"][f, g, row[g]]) not in (0, 1) for g in gone), (f, k, row)
            # ... so that, except in frame 0, cameras of the group sit at a position below their number
            shifted = any(row[c] >= 0 and int((row[:c] >= 0).sum()) < c for c in range(8))
            assert shifted == (f != 0), (f, k, row)
        assert pair == 2, (f, pair)


def test_position_rule_lower_cameras_without_a_hit(core):
    """Heavy roots whose position differs from the camera number, and roots created after camera 0, through the search
    (MOCAP_RESUBMIT_G_CAP=1, forced wide: every root with a choice is exported): the C oracle's correspondences and the plain
    call's bits."""
    from oracle import c_oracle
    rig, blobs, counts, truth = position_rule_frames()
    ref = c_oracle.COracle(rig["K"], rig["R"], rig["t"]).match_triangulate(blobs, counts, gate_px=5.0, K_max=48, G_cap=1 << 20)
    check_position_rule_frames(rig, blobs, counts, truth, ref)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    plain = core.match_triangulate(blobs, counts, gate_px=5.0, K_max=48, G_cap=1 << 20)
    assert not plain["status"].any() and np.array_equal(plain["n_out"], ref["n_out"])
    valid = np.arange(48)[None, :] < ref["n_out"][:, None]
    assert np.array_equal(plain["corr"][valid], ref["corr"][valid])
    for leg in ({}, {"MOCAP_HEAVY_NCAP": "1", "MOCAP_HEAVY_ENUM_CAP": "0"}):         # the search; the enumeration kernel
        try:
            core.set_frame_limits(hit_cap=32, force_wide=True)
            auto = _with_env(dict(leg, MOCAP_RESUBMIT_G_CAP="1"),
                             lambda: core.match_triangulate_auto(blobs, counts, gate_px=5.0, K_max=48, G_cap=1))
            assert core.last_frame_kernel() in WIDE, core.last_frame_kernel()
        finally:
            core.set_frame_limits(hit_cap=32, force_wide=False)
        print(leg, "resubmitted", auto["resubmitted"], "status", auto["status"].tolist(), "n_cand", auto["n_cand"].tolist(), "plain", plain["n_cand"].tolist())
        assert auto["resubmitted"] == len(blobs) and not auto["status"].any(), leg
        assert np.array_equal(auto["n_out"], ref["n_out"]), leg
        assert (auto["n_cand"] < plain["n_cand"]).all(), leg                 # every frame had roots that went to the search
        assert np.array_equal(auto["corr"][valid], ref["corr"][valid]), leg
        assert np.array_equal(auto["xyz"][valid], plain["xyz"][valid]) and np.array_equal(auto["err"][valid], plain["err"][valid]), leg
        np.testing.assert_allclose(auto["xyz"][valid], ref["xyz"][valid], rtol=1e-9, atol=1e-12)
