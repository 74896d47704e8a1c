"""Joint bundle adjustment on the device (include/mocap_core.h, "joint bundle adjustment"; csrc/ba_joint.hip) against the plain
statement of the contract (tests/ba_joint_reference.py): the linearisation entry by entry against 50-digit values, the bits from
call to call, the loop on exact data, against the reference's algorithm on a noisy rig, with outliers, and the refusals."""
import numpy as np
import pytest

import ba_joint_reference as bj

pytestmark = pytest.mark.gpu
np.seterr(all="ignore")

CAP = 1e-9   # pose error on exact data (tests/test_ba_joint_reference_cpu.py: the same cap for the reference alone)


@pytest.fixture(scope="module")
def jcore(core):
    """A context of this module's own: cameras and options set here stay here."""
    from mocap_core import capi
    c = capi.MocapCore(core.device_id)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------------ 3. linearisation
# (C, N, calibrated rig, dropout, focal flag, index of a point given as NaN or None)
SHAPES = {"2x5": (2, 5, False, 0.05, False, None), "3x67": (3, 67, True, 0.3, True, None), "4x257": (4, 257, False, 0.05, False, 100),
          "16x1031": (16, 1031, False, 0.05, True, None)}
COMBOS = [(lam, hub) for lam in (0.0, 1e-3) for hub in (0.0, 2.0)]


def _lin_input(name):
    C, N, calibrated, dropout, focal, nan_row = SHAPES[name]
    # poses 6 mrad / 15 mm off: at 2 px the Huber threshold then splits the views of every shape, some down-weighted and some not
    rig, obs, _, start = bj.planted_case(C, N, noise_px=0.3, calibrated=calibrated, dropout=dropout, rot_sigma=0.006, trans_sigma=0.015)
    X = bj.dlt_start(obs, start["R"], start["t"], rig["K"])
    if nan_row is not None:
        X[nan_row] = np.nan
    fs = 1.0 + 0.01 * np.linspace(-1.0, 1.0, C) if focal else None
    return rig, obs, start, X, fs, focal


@pytest.fixture(scope="module")
def lin_refs():
    """Every input once, with its 50-digit values and the plain-double reference's error against them; the largest such error
    over all inputs is what the device's tolerance is made of."""
    refs = {}
    for name in SHAPES:
        rig, obs, start, X, fs, focal = _lin_input(name)
        for lam, hub in COMBOS:
            args = (obs, start["R"], start["t"], rig["K"], X, fs, focal, hub, lam)
            exact = bj.linearise_mp(*args)
            plain = bj.linearise(*args)
            refs[name, lam, hub] = {"args": args, "exact": exact, "plain": plain, "err": max(bj.rel_errors(plain, exact))}
    worst = max(r["err"] for r in refs.values())
    print(f"\nplain-double reference against the 50-digit values, largest relative error over {len(refs)} inputs: {worst:.3e}")
    return refs, worst


@pytest.mark.parametrize("lam,hub", COMBOS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_linearisation_against_50_digits(jcore, lin_refs, name, lam, hub):
    refs, worst = lin_refs
    ref = refs[name, lam, hub]
    obs, R, t, K, X, fs, focal, _, _ = ref["args"]
    jcore.set_cameras(K, R, t)
    got = jcore.ba_joint_normal_eq(obs, R, t, X, fscale=fs, refine_focal=focal, huber_px=hub, lam=lam)
    again = jcore.ba_joint_normal_eq(obs, R, t, X, fscale=fs, refine_focal=focal, huber_px=hub, lam=lam)
    assert got["S"].tobytes() == again["S"].tobytes() and got["rhs"].tobytes() == again["rhs"].tobytes()
    assert np.float64(got["cost"]).tobytes() == np.float64(again["cost"]).tobytes()
    plain = ref["plain"]
    n_c = bj.n_cam_params(len(R), focal)
    assert got["S"].shape == (n_c, n_c) and np.array_equal(got["S"], got["S"].T)
    assert got["info"]["participating"] == plain["part"].sum() and got["info"]["excluded"] == len(X) - plain["part"].sum()
    assert got["info"]["down_weighted"] == plain["down"] and int(got["info"]["status"]) == plain["status"] == 0
    if hub > 0:
        assert 0 < plain["down"] < plain["seen"].sum()      # the threshold splits the views
    if SHAPES[name][5] is not None:
        assert not plain["part"][SHAPES[name][5]]
    err = max(bj.rel_errors(got, ref["exact"]))
    print(f"{name} lam={lam} huber={hub}: device {err:.3e}, plain doubles {ref['err']:.3e} (largest over all inputs {worst:.3e}), "
          f"tolerance {16 * worst:.3e}")
    assert err <= 16 * worst


# ---------------------------------------------------------------------------------------------------------- 4. exact data
@pytest.mark.parametrize("C,N", [(4, 200), (2, 67), (3, 5)])
def test_solve_recovers_planted_poses_on_exact_data(jcore, C, N):
    rig, obs, X0, start = bj.planted_case(C, N)
    jcore.set_cameras(rig["K"], start["R"], start["t"])
    R, t, _, X, info = jcore.ba_joint_solve(obs, start["R"], start["t"])
    rot, tr = bj.pose_errors(R, t, rig)
    print(f"C={C} N={N}: rotation {rot:.2e} rad, translation {tr:.2e} |t1|; {info}")
    assert rot <= CAP and tr <= CAP
    few = (~np.isnan(obs[..., 0])).sum(axis=1) < 2
    assert np.isnan(X[few]).all() and not np.isnan(X[~few]).any()
    assert info["excluded"] == few.sum() and info["participating"] == N - few.sum()
    t1 = np.linalg.norm(rig["t"][1])
    assert np.abs(X[~few] * (t1 / np.linalg.norm(t[1])) - X0[~few]).max() <= CAP * t1
    assert R[0].tobytes() == start["R"][0].tobytes() and t[0].tobytes() == start["t"][0].tobytes()
    n_in = np.linalg.norm(start["t"][1])
    assert abs(np.linalg.norm(t[1]) - n_in) <= 4 * np.spacing(n_in)
    assert info["cost"] < info["cost0"] and info["accepted"] >= 1


# --------------------------------------------------------------------------------- 5. monotone against the reference's algorithm
def test_monotone_from_the_poses_of_the_reference_algorithm(jcore):
    from mocap_core import synth
    rig, obs, _, start = bj.planted_case(8, 257, noise_px=0.3)
    jcore.set_options(f32_rounding=False)
    try:
        jcore.set_cameras(rig["K"], start["R"], start["t"])
        # the reference's algorithm, resident: x = [f0, (f_i, rotvec_i, t_i)]
        from scipy.spatial.transform import Rotation
        x0 = [rig["K"][0][0, 0]]
        for c in range(1, 8):
            x0 += [rig["K"][c][0, 0]] + Rotation.from_matrix(start["R"][c]).as_rotvec().tolist() + start["t"][c].tolist()
        x, _ = jcore.ba_solve(np.array(x0), obs, ftol=1e-2, f32_residuals=True, use_cauchy=True)
        R = np.stack([np.eye(3)] + [Rotation.from_rotvec(x[7 * i + 2:7 * i + 5]).as_matrix() for i in range(7)])
        t = np.stack([np.zeros(3)] + [x[7 * i + 5:7 * i + 8] for i in range(7)])
        jcore.set_cameras(rig["K"], R, t)
        _, err = jcore.triangulate(obs)
        views = (~np.isnan(obs[..., 0])).sum(axis=1)
        want0 = float(np.sum(2.0 * views[views >= 2] * err[views >= 2]))
        seen = []
        jcore.set_ba_progress(lambda p: seen.append(p.copy()))
        try:
            R1, t1, _, _, info = jcore.ba_joint_solve(obs, R, t)
        finally:
            jcore.set_ba_progress(None)
    finally:
        jcore.set_options(f32_rounding=True)
    e0, e1 = bj.pose_errors(R, t, rig), bj.pose_errors(R1, t1, rig)
    print(f"cost0 {info['cost0']:.6f} (sum 2 v err of mocap_triangulate {want0:.6f}) -> cost {info['cost']:.6f} in {info['accepted']} "
          f"accepted steps of {info['passes']} passes; pose error {e0[0] * 1e3:.3f} mrad / {e0[1]:.2e} -> {e1[0] * 1e3:.3f} mrad / {e1[1]:.2e}")
    assert abs(info["cost0"] - want0) <= 1e-10 * want0
    assert info["cost"] <= info["cost0"]
    assert len(seen) == info["accepted"] >= 1 and all(len(p) == 1 + 7 * 7 for p in seen)
    # every accepted step's cost: the solve cut off after k passes is the same walk (same bytes), so its info is the state after
    # pass k -- an accepted pass lowers the cost strictly, a rejected one leaves it
    prev_cost, prev_acc = info["cost0"], 0
    for k in range(1, int(info["passes"]) + 1):
        jcore.set_cameras(rig["K"], R, t)
        step = jcore.ba_joint_solve(obs, R, t, max_iter=k)[4]
        assert step["accepted"] - prev_acc in (0, 1) and step["cost0"] == info["cost0"]
        assert step["cost"] < prev_cost if step["accepted"] > prev_acc else step["cost"] == prev_cost
        prev_cost, prev_acc = step["cost"], step["accepted"]
    assert prev_cost == info["cost"] and prev_acc == info["accepted"]
    # the plain-double loop ends in the same minimum
    ref = bj.solve(obs, R, t, rig["K"])[4]
    assert abs(ref["cost"] - info["cost"]) <= 1e-6 * info["cost"]
    # the last emitted poses are the returned ones (before the gauge: the rotations)
    last = seen[-1]
    for c in range(1, 8):
        assert np.abs(Rotation.from_rotvec(last[7 * (c - 1) + 2:7 * (c - 1) + 5]).as_matrix() - R1[c]).max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------ 6. Huber
def test_huber_holds_the_poses_against_outliers(jcore):
    rig, clean, bad, moved, start = bj.outlier_case()
    jcore.set_cameras(rig["K"], start["R"], start["t"])
    c = jcore.ba_joint_solve(clean, start["R"], start["t"], max_iter=50)
    off = jcore.ba_joint_solve(bad, start["R"], start["t"], huber_px=0.0, max_iter=50)
    on = jcore.ba_joint_solve(bad, start["R"], start["t"], huber_px=2.0, max_iter=50)
    e_c, e_off, e_on = (bj.pose_errors(r[0], r[1], rig) for r in (c, off, on))
    print(f"clean data {e_c[0] * 1e3:.2f} mrad / {e_c[1]:.2e} |t1|; {moved} observations moved: Huber off {e_off[0] * 1e3:.2f} mrad / "
          f"{e_off[1]:.2e}, at 2 px {e_on[0] * 1e3:.2f} mrad / {e_on[1]:.2e}; down-weighted {on[4]['down_weighted']:.0f}")
    assert e_on[0] <= 0.25 * e_off[0] and e_on[1] <= 0.25 * e_off[1]
    assert on[4]["down_weighted"] >= moved


# ------------------------------------------------------------------------------------------------------ 7. refusals and flags
def _raw_solve(core, obs, R, t, fs=None, flags=0, huber=0.0, ftol=1e-10, max_iter=5):
    from mocap_core.capi import _p
    X = np.full((obs.shape[0], 3), 7.0)
    info = np.full(12, 7.0)
    rc = core.lib.mocap_ba_joint_solve(core._h, obs.shape[0], _p(obs), _p(R), _p(t), _p(fs), _p(X), flags, huber, ftol, max_iter, _p(info))
    return rc, X, info


def test_refusals_and_flags(jcore):
    from mocap_core import capi
    rig, obs, _, start = bj.planted_case(3, 20, noise_px=0.3)
    R, t = np.ascontiguousarray(start["R"]).reshape(3, 9).copy(), np.ascontiguousarray(start["t"]).copy()
    keep = (R.tobytes(), t.tobytes())
    jcore.set_cameras(rig["K"], start["R"], start["t"])
    # a camera without any observation: the flag, nothing written
    blind = obs.copy()
    blind[:, 2] = np.nan
    rc, X, info = _raw_solve(jcore, blind, R, t)
    assert rc == 0 and int(info[8]) & capi.BAJ_ST_CAMERA_UNSEEN and (R.tobytes(), t.tobytes()) == keep and info[1] == 0
    # refusals: outputs untouched
    for kw in (dict(flags=2), dict(huber=-1.0), dict(huber=float("nan")), dict(ftol=-1.0), dict(max_iter=0)):
        rc, X, info = _raw_solve(jcore, obs, R, t, **kw)
        assert rc == capi.MOCAP_E_ARG and (X == 7.0).all() and (info == 7.0).all() and (R.tobytes(), t.tobytes()) == keep, kw
    assert _raw_solve(jcore, obs, R, t, flags=capi.BAJ_FOCAL)[0] == capi.MOCAP_E_ARG        # the focal flag without fscale
    # a K that is not plain
    skew = rig["K"].copy()
    skew[1, 0, 1] = 0.25
    jcore.set_cameras(skew, start["R"], start["t"])
    assert _raw_solve(jcore, obs, R, t)[0] == capi.MOCAP_E_ARG
    with pytest.raises(capi.MocapError) as e:
        jcore.ba_joint_normal_eq(obs, start["R"], start["t"], np.zeros((20, 3)))
    assert e.value.code == capi.MOCAP_E_ARG
    # the focal flag with two cameras, in the library itself
    rig2, obs2, _, start2 = bj.planted_case(2, 20, noise_px=0.3)
    jcore.set_cameras(rig2["K"], start2["R"], start2["t"])
    R2, t2 = np.ascontiguousarray(start2["R"]).reshape(2, 9).copy(), np.ascontiguousarray(start2["t"]).copy()
    assert _raw_solve(jcore, obs2, R2, t2, fs=np.ones(2), flags=capi.BAJ_FOCAL)[0] == capi.MOCAP_E_ARG
    # one point with two views runs
    one = obs2[(~np.isnan(obs2[..., 0])).all(axis=1)][:1].copy()
    rc, X, info = _raw_solve(jcore, one, R2, t2)
    assert rc == 0 and info[5] == 1 and np.isfinite(X).all()
    # without cameras
    fresh = capi.MocapCore(jcore.device_id)
    try:
        assert _raw_solve(fresh, obs2, R2, t2)[0] == -3     # MOCAP_E_NOCAMS
    finally:
        fresh.close()


def test_refine_focal_recovers_a_planted_scale(jcore):
    """Exact data, four cameras, the focal lengths handed over 1 % off: the scales come back."""
    rig, obs, _, start = bj.planted_case(4, 200)
    K = rig["K"].copy()
    true = np.array([1.01, 0.99, 1.005, 0.995])
    K[:, 0, 0] /= true
    K[:, 1, 1] /= true
    jcore.set_cameras(K, start["R"], start["t"])
    R, t, s, _, info = jcore.ba_joint_solve(obs, start["R"], start["t"], refine_focal=True, max_iter=100)
    rot, tr = bj.pose_errors(R, t, rig)
    print(f"focal scales {s} (planted {true}); rotation {rot:.2e} rad, translation {tr:.2e} |t1|; {info}")
    assert np.abs(s - true).max() <= 1e-8 and rot <= 1e-8 and tr <= 1e-8


def test_the_seam_returns_the_reference_shape_and_emits(core):
    from mocap_core import helpers, synth

    class Stub:
        def __init__(self):
            self.sent = []

        def emit(self, name, payload):
            self.sent.append((name, payload))
    rig, obs, _, start = bj.planted_case(4, 60, noise_px=0.3)
    helpers.set_camera_params([{"intrinsic_matrix": rig["K"][c].tolist()} for c in range(4)])
    poses = synth.rig_to_pose_dicts(start)
    sio = Stub()
    out, info = helpers.bundle_adjustment_joint(synth.obs_to_reference_array(obs), poses, sio, huber_px=2.0, return_info=True)
    assert len(out) == 4 and all(set(p) == {"R", "t"} and np.shape(p["R"]) == (3, 3) and np.shape(p["t"]) == (3,) for p in out)
    assert np.array_equal(out[0]["R"], start["R"][0]) and np.array_equal(out[0]["t"], start["t"][0])
    assert len(sio.sent) == info["accepted"] + 1 and info["accepted"] >= 1
    assert all(name == "camera-pose" and len(p["camera_poses"]) == 4 for name, p in sio.sent)
    assert np.allclose(sio.sent[-1][1]["camera_poses"][2]["R"], out[2]["R"], atol=0, rtol=0)
    assert bj.pose_errors([p["R"] for p in out], [p["t"] for p in out], rig)[0] < bj.pose_errors(start["R"], start["t"], rig)[0]
    plain = helpers.bundle_adjustment_joint(synth.obs_to_reference_array(obs), poses, huber_px=2.0)
    assert isinstance(plain, list) and np.array_equal(plain[1]["R"], out[1]["R"])
    with_focal = helpers.bundle_adjustment_joint(synth.obs_to_reference_array(obs), poses, refine_focal=True)
    assert len(with_focal) == 2 and len(with_focal[1]) == 4
