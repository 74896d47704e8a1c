"""GPU: one linearisation of the bundle adjustment at the shapes where its two schedules (the one-launch ba_fused_kernel and
the chain ba_build_cameras -> tri_kernel -> ba_jacobian -> ba_gram -> ba_gram_reduce) and their reduction trees change path,
against tests/ba_linearise_reference.py: J to the rounding of its last operation, J^T J / J^T f inside a derived bound around
the long-double product of the very J the launch returned, the cost against the long-double sum.  Every case runs near the
minimum (residuals below 1: the unclamped Cauchy branch) and far from it (above 1: J_scale is the EPS clamp), in the float64
and the float32 flow, and the schedule a case names is read back from the library (mocap_ba_profile / info[10..11] of
mocap_ba_solve_ex), not trusted from the table.  DESIGN.md 3.4 lists which shape pins which branch."""
import numpy as np
import pytest

import ba_linearise_reference as ref

pytestmark = pytest.mark.gpu

REGIMES = {"converged": dict(rot_sigma=0.0005, trans_sigma=0.001), "far": {}}      # far: perturb_rig's defaults (0.02 rad, 0.05 m)


def _dead(C):
    return [0] + [1 + 7 * i for i in range(C - 1)]


def _x0_of(K, R, t):
    from mocap_core import helpers
    helpers.set_camera_params([{"intrinsic_matrix": k.tolist()} for k in K])
    return helpers._ba_x0([{"R": R[i], "t": t[i]} for i in range(len(R))])


def _ring_problem(C, N, calibrated, regime, seed=None):
    """Seeded rig, capture (dropout 0.1) and start poses.  The poses are drawn from 100 + C whatever the capture's seed: one
    draw per rig size, so `far` is the same distance from the minimum at every point count.  From 4 cameras on a dropout of
    0.1 leaves no point with fewer than two views, so two points (3 and N / 2) keep one view only: m < N at every shape."""
    from mocap_core import synth
    seed = 100 + C if seed is None else seed
    rig = synth.calibrated_ring_rig(C, seed=100 + C) if calibrated else synth.ring_rig(C)
    obs, _ = synth.make_ba_observations(rig, N, seed=seed, dropout=0.1)
    if N >= 8:
        for i in (3, N // 2):
            keep = obs[i, i % C].copy()
            obs[i] = np.nan
            obs[i, i % C] = keep
    init = synth.perturb_rig(rig, np.random.default_rng(100 + C), **REGIMES[regime])
    return {"C": C, "K": rig["K"], "R": init["R"], "t": init["t"], "obs": obs, "x0": _x0_of(rig["K"], init["R"], init["t"]),
            "regime": regime, "calibrated": calibrated}


def _with_m_valid(prob, m):
    """The batch cut after its m-th valid point, plus one point no camera saw: exactly m rows, m < N."""
    obs = prob["obs"]
    valid = (~np.isnan(obs).any(axis=2)).sum(axis=1) >= 2
    assert valid.sum() >= m
    end = int(np.nonzero(valid)[0][m - 1]) + 1
    prob = dict(prob)
    prob["obs"] = np.concatenate([obs[:end], np.full((1,) + obs.shape[1:], np.nan)])
    return prob


def _stereo_problem(rv, regime, seed=3):
    """Two cameras with parallel axes, R1 = rotation(rv), t1 = (-0.5, 0, 0): with rv = 0 the parameter vector has exact zeros
    (rotation vector, t_y, t_z).  x0 IS the generating rig, so `far` comes from the observations: camera 1's blobs moved
    12 px along v, which no 3-D point of a parallel pair can follow."""
    from mocap_core import synth
    from oracle import mocap_oracle
    rv = np.array(rv, dtype=np.float64)
    K = np.repeat(np.array(synth.DEFAULT_K, dtype=np.float64)[None], 2, axis=0)
    R = np.stack([np.eye(3), np.eye(3) if not rv.any() else mocap_oracle.rotvec_to_matrix(rv)])
    t = np.array([[0.0, 0.0, 0.0], [-0.5, 0.0, 0.0]])
    rig = {"K": K, "R": R, "t": t, "R0": np.eye(3), "centre": np.array([0.25, 0.0, 3.0]),
           "image_size": (int(round(2 * K[0, 0, 2])), int(round(2 * K[0, 1, 2])))}
    obs, _ = synth.make_ba_observations(rig, 70, seed=seed, dropout=0.1, half_extent=0.5)
    if regime == "far":
        obs[:, 1, 1] += 12.0
    f = K[0, 0, 0]
    x0 = np.array([f, f, rv[0], rv[1], rv[2], t[1, 0], t[1, 1], t[1, 2]])
    return {"C": 2, "K": K, "R": R, "t": t, "obs": obs, "x0": x0, "regime": regime, "calibrated": False}


def _select(monkeypatch, schedule):
    if schedule == "chain_forced":
        monkeypatch.setenv("MOCAP_BA_UNFUSED", "1")
    else:
        monkeypatch.delenv("MOCAP_BA_UNFUSED", raising=False)


# largest |error| / bound seen per schedule (printed; DESIGN.md 3.4 quotes the run).  With a handful of rows the bound is
# tight by construction (m = 1: one rounding of one product against 2 ulp), so batches of 100 rows and more are kept apart:
# that is where a bound doing no work would show.
RATIOS = {"fused": 0.0, "chain": 0.0, "fused, m >= 100": 0.0, "chain, m >= 100": 0.0}


def _host_m(obs):
    return int(((~np.isnan(obs).any(axis=2)).sum(axis=1) >= 2).sum())


def _assert_regime(prob, r0):
    """converged: every row below 1; far: at most one row in ten.  With per-camera intrinsics the reference takes K by the
    COMPACTED view index (helpers.py:306-307), so a point that lost a view is projected with a neighbour's K and sits far above
    1 even at the generating poses: there `converged` is asserted on the points every camera saw, and the rest are rows of
    the clamped branch in the same launch."""
    obs = prob["obs"]
    if prob["calibrated"] and prob["regime"] == "converged":
        full = ~np.isnan(obs).any(axis=(1, 2))
        assert full.sum() >= 10 and (r0[full] < 1.0).all()
        return
    f = r0[~np.isnan(r0)]
    if f.size == 0:
        return
    below = float((f < 1.0).mean())
    if prob["regime"] == "converged":
        assert below == 1.0, below
    else:
        assert below <= 0.10, below


def _linearise_and_check(core, monkeypatch, prob, f32, cauchy, schedules, tag, min_rows=True):
    """One (case, flow): the reference from the residual kernel's own values at SciPy's parameter sets, then every schedule in
    `schedules` ("fused", "chain_forced" = MOCAP_BA_UNFUSED, "chain" = refused by ba_fused_eligible) against it."""
    C, x0, obs = prob["C"], prob["x0"], prob["obs"]
    n, N = x0.size, obs.shape[0]
    core.set_cameras(prob["K"], prob["R"], prob["t"])
    sets, dx = ref.fd_parameter_sets(x0, ref.rel_step_for(f32))
    _select(monkeypatch, "fused")
    r_sets = core.ba_residuals(sets, obs)
    _assert_regime(prob, r_sets[0])
    lin = ref.linearise(r_sets, dx, f32, cauchy)
    m = _host_m(obs)
    assert lin["rows"].size == m
    if min_rows:
        assert m < N                                     # rows really go through the valid list
    dead = _dead(C)
    Js = {}
    for schedule in schedules:
        _select(monkeypatch, schedule)
        fused = schedule == "fused"
        prof = core.ba_profile(x0, obs, f32_residuals=f32, use_cauchy=cauchy, reps=1)
        assert (prof["fused"], prof["launches"], prof["m"]) == ((1.0, 1.0, m) if fused else (0.0, 5.0, m)), (schedule, prof)
        ne = core.ba_normal_eq(x0, obs, f32_residuals=f32, use_cauchy=cauchy, want_J=True)
        J = ne["J"]
        assert ne["m"] == m and J.shape == (m, n)
        np.testing.assert_allclose(J, lin["J"], rtol=1e-13, atol=1e-13 * np.abs(lin["J"]).max(initial=0.0))
        assert not J[:, dead].any() and not ne["JtJ"][dead].any() and not ne["JtJ"][:, dead].any() and not ne["Jtr"][dead].any()
        # the Gram matrix of the J this launch returned, the gradient with the reference's scaled residual
        G, B = ref.gram_exact(J, lin["fs"])
        err = np.abs(ne["JtJ"].astype(np.longdouble) - G[:n, :n])
        assert (err <= B[:n, :n]).all(), float((err / np.maximum(B[:n, :n], np.finfo(float).tiny)).max())
        assert np.array_equal(ne["JtJ"], ne["JtJ"].T)
        slack = B[:n, n] + 1e-13 * (np.abs(J).T @ np.abs(lin["fs"]))       # what the J tolerance admits for fs
        err_g = np.abs(ne["Jtr"].astype(np.longdouble) - G[:n, n])
        assert (err_g <= slack).all(), float((err_g / np.maximum(slack, np.finfo(float).tiny)).max())
        live = B[:n, :n] > 0
        ratio = max(float((err[live] / B[:n, :n][live]).max(initial=0.0)),
                    float((err_g[slack > 0] / slack[slack > 0]).max(initial=0.0)))
        for key in ["fused" if fused else "chain"] + (["fused, m >= 100" if fused else "chain, m >= 100"] if m >= 100 else []):
            RATIOS[key] = max(RATIOS[key], ratio)
        np.testing.assert_allclose(ne["cost"], float(lin["cost"]), rtol=2e-7 if f32 else 1e-12, atol=0)
        # the counters are back at zero and the tree adds in record order: the same call again, bit for bit
        again = core.ba_normal_eq(x0, obs, f32_residuals=f32, use_cauchy=cauchy, want_J=False)
        assert np.array_equal(again["JtJ"], ne["JtJ"]) and np.array_equal(again["Jtr"], ne["Jtr"]) and again["cost"] == ne["cost"]
        print(f"[{tag} f32={int(f32)} cauchy={int(cauchy)} {schedule}] m={m} N={N} n={n} NP={prof['NP']:.0f} error/bound={ratio:.3g} "
              f"(largest so far: {RATIOS})")
        Js[schedule] = J
    if len(Js) == 2:
        # both schedules claim the same per-point arithmetic (contraction off): the same J, bit for bit
        a, b = Js.values()
        assert np.array_equal(a, b), float(np.abs(a - b).max())
    return lin


BOTH = ("fused", "chain_forced")
# (C, N, per-camera K, schedules): the smallest shapes at which each branch exists
CASES = [
    (2, 1, False, BOTH), (2, 63, False, BOTH), (2, 64, False, BOTH), (2, 65, False, BOTH),
    (3, 130, False, BOTH),
    (3, 1024, False, BOTH), (3, 1025, False, BOTH),
    (3, 16384, False, BOTH), (3, 16449, False, BOTH),
    (9, 128, False, BOTH), (9, 128, True, BOTH),
    (13, 70, True, BOTH),
    (14, 70, True, ("chain",)),
    (19, 130, False, BOTH),
    (20, 130, False, ("chain",)),
]


def _case_id(c):
    return f"{c[0]}x{c[1]}{'Kc' if c[2] else 'K'}"


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_linearisation_at_the_shape(core, monkeypatch, case, regime):
    C, N, calibrated, schedules = case
    prob = _ring_problem(C, N, calibrated, regime, seed=CAPTURE_SEED.get((C, N), 100 + C))
    assert _host_m(prob["obs"][-1:]) == 1            # the last point is a row: N one off a chunk / a node is a live edge
    for f32 in (False, True):
        # a single point is the row itself; every other batch has dropped points inside
        _linearise_and_check(core, monkeypatch, prob, f32, True, schedules, f"{_case_id(case)} {regime}", min_rows=N > 1)


CAPTURE_SEED = {(3, 1025): 1103}      # 100 + C leaves the 1 025th point with one view


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("m", [1, 3, 4, 5, 33, 286, 8203])
def test_chain_row_padding_and_k_split(core, monkeypatch, m, regime):
    """The chain's m_pad padding rows and the K split of its Gram kernel: m = 1, 3, 4, 5 (one step, 0 to 3 padding rows), 33
    (m_pad 36: ksplit 1 with 9 steps), 286 (m_pad 288: ksplit 9, not a multiple of the reduce kernel's 8), 8 203 (m_pad 8 204:
    ksplit capped at 256 over 2 051 steps, an uneven split)."""
    prob = _with_m_valid(_ring_problem(3, int(m * 1.3) + 12, False, regime, seed=300 + m), m)
    for f32 in (False, True):
        _linearise_and_check(core, monkeypatch, prob, f32, True, ("chain_forced",), f"3 cameras m={m} {regime}")


@pytest.mark.parametrize("regime", list(REGIMES))
def test_linear_loss_once_per_schedule(core, monkeypatch, regime):
    prob = _ring_problem(3, 130, False, regime, seed=103)
    for f32 in (False, True):
        _linearise_and_check(core, monkeypatch, prob, f32, False, BOTH, f"3x130K linear {regime}")


STEREO_RV = {"zero": (0.0, 0.0, 0.0),
             "series": tuple(3.7e-4 * np.array([1.0, -2.0, 2.0]) / 3.0),
             "just_above_series": tuple(1.0000001e-3 * np.array([1.0, -2.0, 2.0]) / 3.0),
             "nearly_pi": (0.0, 0.0, np.pi - 1e-7)}


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("variant", list(STEREO_RV))
def test_stereo_exact_zeros_and_rotation_branches(core, monkeypatch, variant, regime):
    """Parameter vectors with exact zeros (the step rule at v = 0: sign +1, max(1, |v|) = 1) and rotation vectors on both
    sides of rotvec_to_matrix's 1e-3 series threshold and next to pi; the residuals at SciPy's parameter sets against the C
    oracle as well (tolerances of test_residuals_vs_c_oracle_1k_points)."""
    from oracle import c_oracle
    prob = _stereo_problem(STEREO_RV[variant], regime)
    x0 = prob["x0"]
    angle = float(np.linalg.norm(x0[2:5]))
    assert {"zero": angle == 0.0 and not x0[[6, 7]].any(), "series": 0 < angle < 1e-3, "just_above_series": 1e-3 < angle < 1.001e-3,
            "nearly_pi": 3.14 < angle < np.pi}[variant]
    for f32 in (False, True):
        _linearise_and_check(core, monkeypatch, prob, f32, True, BOTH, f"stereo {variant} {regime}")
        sets, _ = ref.fd_parameter_sets(x0, ref.rel_step_for(f32))
        r = core.ba_residuals(sets, prob["obs"])
        want = c_oracle.COracle(prob["K"], prob["R"], prob["t"]).ba_residuals(sets, prob["obs"])
        assert np.array_equal(np.isnan(r), np.isnan(want))
        ok = ~np.isnan(want)
        np.testing.assert_allclose(r[ok], want[ok], rtol=1e-3, atol=1e-12)
        assert np.median(np.abs(r[ok] - want[ok]) / want[ok]) < 1e-9


@pytest.mark.parametrize("schedule", BOTH)
def test_no_point_with_two_views(core, monkeypatch, schedule):
    """Every point seen by one camera only: no row, J^T J and J^T f all zero, cost 0."""
    prob = _ring_problem(3, 130, False, "far", seed=103)
    obs = prob["obs"].copy()
    for i in range(obs.shape[0]):
        keep = obs[i, i % 3].copy()
        obs[i] = np.nan
        obs[i, i % 3] = keep
    assert _host_m(obs) == 0 and (~np.isnan(obs)).any()
    core.set_cameras(prob["K"], prob["R"], prob["t"])
    _select(monkeypatch, schedule)
    assert core.ba_profile(prob["x0"], prob["obs"], reps=1)["fused"] == (1.0 if schedule == "fused" else 0.0)
    for f32 in (False, True):
        ne = core.ba_normal_eq(prob["x0"], obs, f32_residuals=f32, use_cauchy=True, want_J=True)
        assert ne["m"] == 0 and ne["J"].shape == (0, 15)
        assert not ne["JtJ"].any() and not ne["Jtr"].any() and ne["cost"] == 0.0


@pytest.mark.parametrize("regime", list(REGIMES))
def test_a_whole_chunk_of_dropped_points(core, monkeypatch, regime):
    """Points 64 .. 127 all dropped: a chunk of the one-launch kernel without a single valid row (its Gram partial and cost
    record are zeros that still travel through the tree)."""
    prob = _ring_problem(3, 200, False, regime, seed=104)
    prob["obs"][64:128] = np.nan
    for f32 in (False, True):
        _linearise_and_check(core, monkeypatch, prob, f32, True, BOTH, f"3x200K chunk 1 dropped {regime}")


# ---------------------------------------------------------------------------------------------------------------
# Launch-ahead at the solve level: a kernel parked on the host's mailbox, polled with one word per lane up to n = 56 and with a
# second word (lane + 64) from n = 57; the host arms it up to n = 112 and N = 2 048.
@pytest.mark.timeout(120)       # a wrong poll ends at the device watchdogs (2 s / 30 s) and the host's 20 s limit, not here
@pytest.mark.parametrize("C,N,ahead", [(8, 128, True), (9, 128, True), (16, 128, True), (17, 128, False),
                                       (3, 2048, True), (3, 2049, False)],
                         ids=["n50_one_poll_word", "n57_second_poll_word", "n106_all_128_words", "n113_host_switches_off",
                              "N2048_last_armed", "N2049_first_unarmed"])
def test_launch_ahead_hands_over_the_same_points(core, monkeypatch, C, N, ahead):
    """The same solve with the base points handed to a launched-ahead kernel through the mailbox and with every point passed by
    value (MOCAP_BA_NO_PREARM): the arithmetic does not depend on how the point reached the kernel, so x is bit-identical and
    the counts and the cost are equal.  info[10] says whether the mailbox was really used."""
    prob = _ring_problem(C, N, False, "far", seed=200 + C)
    assert prob["x0"].size == 1 + 7 * (C - 1)
    core.set_cameras(prob["K"], prob["R"], prob["t"])
    monkeypatch.delenv("MOCAP_BA_UNFUSED", raising=False)
    # 8 evaluations from this far out are the first point and 7 rejected trials (the radius starts at |x0|, which the focal
    # entries make ~ 1 000): every hand-over is exercised but x stays put, so the same pair again with 24 evaluations, where
    # a dozen steps are accepted (SciPy on the C oracle's residuals: 13 to 15) and a wrong word in any hand-over moves x.
    for budget in (8, 24):
        out = {}
        for mode in ("default", "no_prearm"):
            if mode == "no_prearm":
                monkeypatch.setenv("MOCAP_BA_NO_PREARM", "1")
            else:
                monkeypatch.delenv("MOCAP_BA_NO_PREARM", raising=False)
            out[mode] = core.ba_solve(prob["x0"], prob["obs"], ftol=0.0, xtol=0.0, gtol=0.0, max_iter=budget)
        (xa, ia), (xb, ib) = out["default"], out["no_prearm"]
        assert ia["fused"] == ib["fused"] == 1.0 and ia["relaunches"] == ib["relaunches"] == 0.0
        assert ia["nfev"] == ib["nfev"] == float(budget) and ia["njev"] == ib["njev"] and ia["iterations"] == ib["iterations"]
        assert ib["handovers"] == 0.0
        # launch-ahead on: every linearisation of the solve (the first point and one per trial) got its point by mailbox
        assert ia["handovers"] == (ia["nfev"] if ahead else 0.0)
        assert ia["cost0"] == ib["cost0"] and ia["cost"] == ib["cost"]
        assert np.array_equal(xa, xb)
        if budget == 24:
            assert ia["njev"] >= 4.0 and ia["cost"] < 0.5 * ia["cost0"] and not np.array_equal(xa, prob["x0"])


def test_solve_reports_the_chain_schedule(core, monkeypatch):
    """info[11] = 0 and no hand-over when the chain runs: refused by ba_fused_eligible (20 cameras) and switched by hand."""
    for C, forced in ((20, False), (3, True)):
        prob = _ring_problem(C, 130, False, "far", seed=200 + C)
        core.set_cameras(prob["K"], prob["R"], prob["t"])
        _select(monkeypatch, "chain_forced" if forced else "fused")
        x, info = core.ba_solve(prob["x0"], prob["obs"], ftol=0.0, xtol=0.0, gtol=0.0, max_iter=16)
        assert info["fused"] == 0.0 and info["handovers"] == 0.0 and info["relaunches"] == 0.0
        assert info["nfev"] == 16.0 and info["cost"] < info["cost0"]
