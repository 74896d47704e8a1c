"""Camera resection on the device (include/mocap_core.h, "camera resection"; csrc/resect.hip) against the plain statement of the
contract (tests/resection_reference.py): the candidate table of the search, the full two-round solve against the 50-digit minimiser,
the evaluate-only mode, the two outcomes without a pose, the bits from call to call, the device-pointer form, and the two helpers
(camera_health, reseat_camera) on a ring rig with one camera knocked.

The margin of 16 on every comparison with a 50-digit value is the project's rule: the device may be 16 times as far
from the exact value as the plain-double statement of the same arithmetic is."""
import math

import numpy as np
import pytest

import resection_reference as rr

pytestmark = pytest.mark.gpu
np.seterr(all="ignore")

NAMES = list(rr.CASES)
MARGIN = 16.0


@pytest.fixture(scope="module")
def rcore(core):
    """A context of this module's own."""
    from mocap_core import capi
    c = capi.MocapCore(core.device_id)
    yield c
    c.close()


def _args(c):
    return dict(prior=c["prior"], threshold_px=rr.THRESHOLD, n_hyp=c["n_hyp"], seed=rr.SEED)


_solved = {}


def _solve(rcore, name):
    """The device's full solve of a case, once."""
    if name not in _solved:
        c = rr.case(name)
        _solved[name] = rcore.resect_camera(c["X"], c["obs"], c["K"], min_inliers=c["min_inliers"], max_iter=rr.MAX_ITER, **_args(c))
    return _solved[name]


# ------------------------------------------------------------------------------------------------------------------- probe
@pytest.mark.parametrize("name", NAMES)
def test_candidate_table(rcore, name):
    c = rr.case(name)
    ref, k4 = c["table"], rr.k4_of(c["K"])
    dev = rcore.resect_hypotheses(c["X"], c["obs"], c["K"], **_args(c))
    H = ref["poses"].shape[0]
    assert dev["poses"].shape == (H, 4, 12)
    assert np.array_equal(dev["sample"], ref["sample"])                      # the sampler, exactly
    if c["prior"] is not None:                                               # hypothesis 0 is the prior itself
        assert dev["n_sol"][0] == 1 and np.array_equal(dev["poses"][0, 0], rr.pose_of(*c["prior"])) and (dev["sample"][0] == -1).all()
    rows, idx = ref["rows"], ref["idx"]
    worst = {"ref": [0.0, 0.0], "dev": [0.0, 0.0]}
    for h in range(H):
        if ref["sample"][h, 0] < 0:
            continue
        pick = [int(np.nonzero(idx == i)[0][0]) for i in ref["sample"][h]]
        for who, tab in (("ref", ref), ("dev", dev)):
            for s in range(int(tab["n_sol"][h])):
                assert np.isfinite(tab["poses"][h, s]).all()
                px, orth = rr.mp_sample_error(list(tab["poses"][h, s]), k4, rows[pick])
                worst[who] = [max(worst[who][0], px), max(worst[who][1], orth)]
            assert np.isnan(tab["poses"][h, int(tab["n_sol"][h]):]).all()
        # every well-conditioned solution of the statement is among the device's
        for s in range(int(ref["n_sol"][h])):
            if min(ref["cond"][h][s]) > 1e-6:
                d = [np.abs(dev["poses"][h, k] - ref["poses"][h, s]).max() for k in range(int(dev["n_sol"][h]))]
                assert d and min(d) < 1e-6, (h, s, d)
    print(f"\n{name}: sample reprojection at 50 digits, statement {worst['ref'][0]:.3e} px / device {worst['dev'][0]:.3e} px; "
          f"|R^T R - I| statement {worst['ref'][1]:.3e} / device {worst['dev'][1]:.3e}")
    assert worst["dev"][0] <= MARGIN * worst["ref"][0] and worst["dev"][1] <= MARGIN * worst["ref"][1]
    # the counts: the statement's scoring of the device's OWN poses, bit for bit (IEEE +, -, x, / and comparisons only)
    assert np.array_equal(dev["counts"], rr.score_poses(dev["poses"], dev["n_sol"], c["K"], c["X"], c["obs"], rr.THRESHOLD))
    # the winner: the stated rule over the device's counts
    info = _solve(rcore, name)[3]
    assert (info["winner_hypothesis"], info["winner_solution"], info["winner_inliers"]) == rr.winner(dev["counts"], dev["n_sol"])
    assert info["no_solution"] == int((dev["n_sol"] == 0).sum()) and info["valid"] == len(idx)


# -------------------------------------------------------------------------------------------------------------- full solve
@pytest.mark.parametrize("name", NAMES)
def test_full_solve(rcore, name):
    c = rr.case(name)
    k4, rows, idx = rr.k4_of(c["K"]), c["table"]["rows"], c["table"]["idx"]
    R, t, mask, info = _solve(rcore, name)
    pose = rr.pose_of(R, t)
    assert info["status"] == rr.OK and info["accepted"] >= 1
    want = np.zeros(len(mask), dtype=bool)
    want[idx[rr.classify(pose, k4, rows, rr.THRESHOLD)]] = True
    assert np.array_equal(mask, want)                   # the classification at the device's final pose
    assert np.array_equal(mask, c["mask"])              # ... which is the planted mask
    assert info["inliers"] == int(mask.sum())
    # against the 50-digit minimiser over that mask (the statement ends on the same mask: test_resection_reference_cpu.py)
    assert np.array_equal(c["solve"][2], mask)
    Rm, tm, cost_min, (ref_dR, ref_dt) = rr.minimiser(name)
    dR, dt = rr.mp_distance(pose, Rm, tm)
    print(f"\n{name}: distance to the 50-digit minimiser, statement dR {ref_dR:.3e} dt {ref_dt:.3e} / device dR {dR:.3e} dt {dt:.3e}; "
          f"{info['accepted']} steps, {info['linearisations']} linearisations, rms {info['rms_winner']:.4g} -> {info['rms_final']:.4g} px")
    assert dR <= MARGIN * ref_dR and dt <= MARGIN * ref_dt
    if name == "exact6":
        assert np.abs(R - c["R"]).max() < 1e-9 and np.linalg.norm(t - c["t"]) < 1e-9
    else:                                               # a minimum cannot be higher than the planted pose's cost
        assert rr.mp_cost(pose, k4, rows, mask[idx]) <= rr.mp_cost(rr.pose_of(c["R"], c["t"]), k4, rows, mask[idx])
        assert info["rms_final"] < info["rms_winner"]
    assert math.isclose(info["rms_final"], math.sqrt(rr.cost_over(pose, k4, rows, mask[idx]) / mask.sum()), rel_tol=1e-12, abs_tol=1e-18)
    if c["prior"] is not None:
        assert info["rms_prior"] > info["rms_final"]
        assert math.isclose(info["rms_prior"], math.sqrt(rr.cost_over(rr.pose_of(*c["prior"]), k4, rows, mask[idx]) / mask.sum()), rel_tol=1e-12)
    else:
        assert math.isnan(info["rms_prior"])


def test_two_calls_give_the_same_bytes_and_the_device_form_equals_the_host_form(rcore):
    import torch
    c = rr.case("noisy1031")
    first = _solve(rcore, "noisy1031")
    again = rcore.resect_camera(c["X"], c["obs"], c["K"], min_inliers=c["min_inliers"], max_iter=rr.MAX_ITER, **_args(c))
    d_X = torch.from_numpy(np.ascontiguousarray(c["X"])).to("cuda:%d" % rcore.device_id)
    d_obs = torch.from_numpy(np.ascontiguousarray(c["obs"])).to("cuda:%d" % rcore.device_id)
    torch.cuda.synchronize()
    dev = rcore.resect_camera_dev(len(c["X"]), d_X.data_ptr(), d_obs.data_ptr(), c["K"], min_inliers=c["min_inliers"], max_iter=rr.MAX_ITER,
                                  **_args(c))
    for other in (again, dev):
        assert first[0].tobytes() == other[0].tobytes() and first[1].tobytes() == other[1].tobytes()
        assert np.array_equal(first[2], other[2])
        assert np.array([first[3][k] for k in rr.INFO_KEYS]).tobytes() == np.array([other[3][k] for k in rr.INFO_KEYS]).tobytes()
    t1 = rcore.resect_hypotheses(c["X"], c["obs"], c["K"], **_args(c))
    t2 = rcore.resect_hypotheses(c["X"], c["obs"], c["K"], **_args(c))
    assert all(t1[k].tobytes() == t2[k].tobytes() for k in t1)


def test_evaluate_only_returns_the_priors_bits(rcore):
    c = rr.case("prior257")
    k4, rows, idx = rr.k4_of(c["K"]), c["table"]["rows"], c["table"]["idx"]
    for thr in (2.0, 30.0):
        R, t, mask, info = rcore.resect_camera(c["X"], c["obs"], c["K"], prior=c["prior"], threshold_px=thr, n_hyp=0, min_inliers=4, max_iter=0)
        _, _, rmask, rinfo = rr.resect(c["X"], c["obs"], c["K"], c["prior"], thr, 0, 0, 4, 0)
        assert R.tobytes() == np.ascontiguousarray(c["prior"][0]).tobytes() and t.tobytes() == np.ascontiguousarray(c["prior"][1]).tobytes()
        assert np.array_equal(mask, rmask) and info["accepted"] == 0 and info["linearisations"] == 0
        for k in ("valid", "winner_inliers", "winner_hypothesis", "winner_solution", "no_solution", "inliers", "status"):
            assert info[k] == rinfo[k], k
        if rinfo["inliers"]:
            assert info["rms_prior"] == info["rms_final"] == info["rms_winner"]
            assert math.isclose(info["rms_final"], rinfo["rms_final"], rel_tol=1e-12)
    # a search without refinement: the winner comes back as it is
    R, t, _, info = rcore.resect_camera(c["X"], c["obs"], c["K"], min_inliers=c["min_inliers"], max_iter=0, **_args(c))
    tab = rcore.resect_hypotheses(c["X"], c["obs"], c["K"], **_args(c))
    assert rr.pose_of(R, t) == tab["poses"][info["winner_hypothesis"], info["winner_solution"]].tolist() and info["accepted"] == 0


def test_too_few_and_no_model(rcore):
    c = rr.planted_case(40, outliers=0.2, noise=0.3, prior_off=(3.0, 0.03), seed=5)
    X = c["X"].copy()
    X[3:] = np.nan
    R, t, mask, info = rcore.resect_camera(X, c["obs"], c["K"], threshold_px=2.0, n_hyp=16, seed=1, min_inliers=4, max_iter=10)
    assert info["status"] == rr.TOO_FEW and info["valid"] == 3 and np.isnan(R).all() and np.isnan(t).all() and not mask.any()
    R, t, mask, info = rcore.resect_camera(X, c["obs"], c["K"], prior=c["prior"], threshold_px=2.0, n_hyp=16, seed=1, min_inliers=4, max_iter=10)
    assert info["status"] == rr.TOO_FEW and np.array_equal(R, c["prior"][0]) and np.array_equal(t, c["prior"][1]) and info["accepted"] == 0
    rng = np.random.default_rng(11)
    scrambled = np.stack([rng.uniform(0, 320, 67), rng.uniform(0, 240, 67)], axis=1)
    big = rr.planted_case(67, seed=5)
    R, t, mask, info = rcore.resect_camera(big["X"], scrambled, big["K"], threshold_px=2.0, n_hyp=64, seed=1, min_inliers=8, max_iter=10)
    assert info["status"] == rr.NO_MODEL and info["winner_inliers"] < 8 and np.isnan(R).all() and info["accepted"] == 0 and not mask.any()


def test_refusals_leave_every_output_untouched(rcore):
    from mocap_core import capi
    c = rr.planted_case(8)
    X, obs, K = np.ascontiguousarray(c["X"]), np.ascontiguousarray(c["obs"]), np.ascontiguousarray(c["K"]).reshape(9)
    skew = K.copy()
    skew[1] = 0.5
    pR, pt = np.ascontiguousarray(c["R"]).reshape(9), np.ascontiguousarray(c["t"])
    p = lambda a: None if a is None else a.ctypes.data     # noqa: E731
    base = dict(N=8, X=X, obs=obs, K=K, pR=None, pt=None, thr=2.0, n_hyp=16, min_inliers=4, max_iter=5, R=True, t=True)
    for kw in (dict(N=0), dict(N=rr.MAX_POINTS + 1), dict(n_hyp=-1), dict(n_hyp=rr.MAX_HYP + 1), dict(min_inliers=3), dict(max_iter=-1),
               dict(K=skew), dict(thr=0.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(n_hyp=0), dict(pR=pR), dict(pt=pt),
               dict(X=None), dict(obs=None), dict(K=None), dict(R=False), dict(t=False)):
        a = dict(base)
        a.update(kw)
        R, t, mask, info = np.full(9, 7.0), np.full(3, 7.0), np.full(8, 7, dtype=np.uint8), np.full(rr.INFO, 7.0)
        rc = rcore.lib.mocap_resect_camera(rcore._h, a["N"], p(a["X"]), p(a["obs"]), p(a["K"]), p(a["pR"]), p(a["pt"]), a["thr"], a["n_hyp"], 3,
                                           a["min_inliers"], a["max_iter"], p(R) if a["R"] else None, p(t) if a["t"] else None, p(mask),
                                           p(info))
        assert rc == capi.MOCAP_E_ARG, kw
        assert (R == 7.0).all() and (t == 7.0).all() and (mask == 7).all() and (info == 7.0).all(), kw


# ----------------------------------------------------------------------------------------------------------------- helpers
def _knocked_rig(camera):
    """synth.ring_rig(4) whose camera `camera` was turned by 3 degrees and moved 30 mm after the calibration: the capture comes from
    the rig as it stands now, the poses handed to the helpers are the calibration's."""
    from mocap_core import synth
    rig = synth.ring_rig(4)
    rng = np.random.default_rng(40 + camera)
    axis, shift = rng.normal(size=3), rng.normal(size=3)
    step = list(axis / np.linalg.norm(axis) * math.radians(3.0)) + list(shift / np.linalg.norm(shift) * 0.03)
    moved = rr.apply_step(rr.pose_of(rig["R"][camera], rig["t"][camera]), step)
    now = dict(rig, R=rig["R"].copy(), t=rig["t"].copy())
    now["R"][camera], now["t"][camera] = np.array(moved[:9]).reshape(3, 3), np.array(moved[9:])
    obs, _ = synth.make_ba_observations(now, 160, seed=9, noise_px=0.3, dropout=0.05)
    return rig, now, obs


@pytest.fixture()
def seam(core):
    from mocap_core import helpers
    saved = dict(helpers._state)
    yield helpers
    helpers._state.update(saved)


def _pose_error(pose, R, t):
    return float(np.abs(np.asarray(pose["R"]) - R).max()), float(np.linalg.norm(np.asarray(pose["t"]).reshape(3) - t))


def _gate(helpers, obs, poses, camera, report):
    """The minimiser comparison of test_full_solve on that camera's data: points built without it, its own views."""
    _, X, o, K, prior = helpers._resection_inputs(obs, poses, camera)
    Rr, tr, rmask, _ = rr.resect(X, o, K, prior, 2.0, 256, 0, 6, 20)
    rows, idx = rr.valid_rows(X, o)
    _, _, dmask, _ = helpers.get_core().resect_camera(X, o, K, prior=(report["R"], report["t"]), threshold_px=2.0, n_hyp=0, min_inliers=4,
                                                      max_iter=0)
    assert np.array_equal(dmask, rmask)
    Rm, tm, _ = rr.mp_minimise(rr.pose_of(Rr, tr), rr.k4_of(K), rows, rmask[idx])
    ref = rr.mp_distance(rr.pose_of(Rr, tr), Rm, tm)
    dev = rr.mp_distance(rr.pose_of(report["R"], report["t"]), Rm, tm)
    print(f"camera {camera}: distance to the 50-digit minimiser, statement dR {ref[0]:.3e} dt {ref[1]:.3e} / device dR {dev[0]:.3e} dt {dev[1]:.3e}")
    assert dev[0] <= MARGIN * ref[0] and dev[1] <= MARGIN * ref[1]


def test_camera_health_finds_the_knocked_camera_and_reseat_brings_it_back(seam):
    from mocap_core import capi, synth
    rig, now, obs = _knocked_rig(2)
    seam.set_camera_params([{"intrinsic_matrix": K.tolist()} for K in rig["K"]])
    poses = synth.rig_to_pose_dicts(rig)
    health = seam.camera_health(obs, poses)
    print("\ncamera_health:", [(round(h["rms"], 3), round(h["inlier_share"], 3), h["views"]) for h in health])
    assert len(health) == 4 and max(range(4), key=lambda c: health[c]["rms"]) == 2
    assert health[2]["inlier_share"] == min(h["inlier_share"] for h in health) and all(h["views"] > 100 for h in health)
    new, report = seam.reseat_camera(obs, poses, 2)
    before, after = _pose_error(poses[2], now["R"][2], now["t"][2]), _pose_error(new[2], now["R"][2], now["t"][2])
    print(f"camera 2: pose error |dR| {before[0]:.3e} |dt| {before[1]:.3e} before, |dR| {after[0]:.3e} |dt| {after[1]:.3e} after; "
          f"rms {report['rms_prior']:.3f} -> {report['rms_final']:.3f} px over {report['inliers']} of {report['valid']} views")
    assert report["status"] == capi.RESECT_OK and report["camera"] == 2 and "to_world_right" not in report
    assert after[0] < before[0] / 20 and after[1] < before[1] / 5 and report["rms_final"] < report["rms_prior"]
    for c in (0, 1, 3):
        assert np.array_equal(new[c]["R"], rig["R"][c]) and np.array_equal(new[c]["t"], rig["t"][c])
    _gate(seam, obs, poses, 2, report)
    healed = seam.camera_health(obs, new)
    assert healed[2]["rms"] < 1.0 and healed[2]["inlier_share"] > 0.95


def test_reseating_camera_0_keeps_the_gauge_and_the_world(seam):
    from mocap_core import capi, synth
    rig, now, obs = _knocked_rig(0)
    seam.set_camera_params([{"intrinsic_matrix": K.tolist()} for K in rig["K"]])
    poses = synth.rig_to_pose_dicts(rig)
    new, report = seam.reseat_camera(obs, poses, 0)
    R0, t0 = report["R"], report["t"]
    before, after = _pose_error(poses[0], now["R"][0], now["t"][0]), _pose_error({"R": R0, "t": t0}, now["R"][0], now["t"][0])
    print(f"\ncamera 0: pose error |dR| {before[0]:.3e} |dt| {before[1]:.3e} before, |dR| {after[0]:.3e} |dt| {after[1]:.3e} after")
    assert report["status"] == capi.RESECT_OK and after[0] < before[0] / 20 and after[1] < before[1] / 5
    assert np.array_equal(new[0]["R"], np.eye(3)) and not np.asarray(new[0]["t"]).any()
    _gate(seam, obs, poses, 0, report)
    # the statement's re-gauge of the same resected pose
    Rn, tn, M = rr.regauge(rig["R"], rig["t"], R0, t0)
    for c in range(4):
        assert np.abs(new[c]["R"] - Rn[c]).max() < 1e-15 and np.abs(new[c]["t"] - tn[c]).max() < 1e-15
    assert np.abs(report["to_world_right"] - M).max() < 1e-15
    # world coordinates of the capture's points do not move: points from cameras 1 .. 3, before in the old frame under W, after in the
    # new frame under W M -- once with the helper's poses and matrix, once with the statement's (its own discrepancy)
    blanked = obs.copy()
    blanked[:, 0] = np.nan
    D = np.diag([-1.0, -1.0, 1.0])
    W = np.eye(4)
    W[:3, :3] = np.array(rr.apply_step(rr.pose_of(np.eye(3), np.zeros(3)), [0.3, -0.2, 0.1, 0, 0, 0])[:9]).reshape(3, 3) * 1.7
    W[:3, 3] = [0.4, -1.0, 2.0]

    def world(Wm, pose_list):
        X = np.array([[np.nan] * 3 if r[0] is None else r for r in seam.triangulate_points_refined(blanked, pose_list)], dtype=np.float64)
        return (np.c_[X @ D, np.ones(len(X))] @ Wm.T)[:, :3]

    old = world(W, poses)
    seen = np.isfinite(old[:, 0])
    disc_dev = np.abs(world(W @ report["to_world_right"], new) - old)[seen].max()
    disc_ref = np.abs(world(W @ M, [{"R": Rn[c], "t": tn[c]} for c in range(4)]) - old)[seen].max()
    print(f"world coordinates before / after: helper {disc_dev:.3e}, statement {disc_ref:.3e} (of {int(seen.sum())} points)")
    assert seen.sum() > 100 and disc_dev <= MARGIN * disc_ref
    # The refined points are four Levenberg-Marquardt steps from a DLT start, not converged minima, so the two frames' points agree
    # only as far as those steps have converged -- but a micrometre is a thousandth of the points' own noise (0.3 px at 3 m is
    # millimetres), while a wrong re-gauge moves the world by centimetres (3 degrees at 3 m).
    assert disc_dev < 1e-6
