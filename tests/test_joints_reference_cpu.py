"""The statement of "joints" (tests/joints_reference.py, include/mocap_core.h) on the CPU: the stacked Jacobi against the scalar one bit
for bit; the fit against 50 digits; the five-body scene -- body 0 - ball - body 1 - hinge - body 2, body 3 rigidly attached to body 0,
body 4 flying free, swings of +-0.5 rad, 2 000 frames -- against its planted truth, noise-free and with 0.5 mm and 5 mrad of noise
(the rms length of each pose's translation error and of its rotation-error vector); the margins that keep every kind away from
rounding; Kruskal on ties, a cycle and two components.

The error bounds are four times the figures measured here over SEEDS (DESIGN.md 3.7s has the table):
    against 50 digits      lambda 3.4e-16, centres 8.9e-16 m, sep 5.5e-18 m (the scene with noise, 400 frames)
    noise-free             ball centre 4.4e-16 m, hinge centre to the planted line 5.9e-16 m, axis angle 2.7e-15 rad
    0.5 mm + 5 mrad        ball centre 5.6e-5 m, hinge centre to the planted line 4.6e-5 m, axis angle 4.8e-4 rad
    hinge angle per frame  noise-free 2.2e-15 rad at most (rms 6.7e-16); with noise 1.9e-2 rad at most (rms 6.3e-3)

Two things about this scene are not what one expects at first sight; its own geometry forces both:
  * parent is [-1, 0, 1, 1, -1], not [-1, 0, 1, -1, -1].  Body 3 is rigid with body 0, so the ball joint of (0, 1) is a point body 1
    shares with body 3 just as well: the pair (1, 3) is BALL with a residual at the noise, the contract accepts it, and Kruskal takes
    it as the third tree edge.  (0, 3) itself is FIXED and never an edge.
  * every sep is a factor 10 away from max_sep = 1 cm on the accepted side, and a factor 7 on the other.  The nearest non-joint is
    the pair (0, 2), two joints apart: its sep grows with the length L of body 1 (about 0.3 L at these swings), but so does the noise
    of the joints at body 1's ends (5 mrad at a lever of L / 2 each); the ratio of the two stays below 103 for any L, so 10 x 10
    is out of reach with this noise and L = 0.28 m gives 10 and 7.5 .. 9.  No kind or acceptance is anywhere near rounding."""
import numpy as np
import pytest

import joints_reference as jr

SEEDS = (3, 4, 5)
S3 = 3.0 ** 0.5
NOISE = (0.0005 / S3, 0.005 / S3)      # per component: 0.5 mm and 5 mrad of rms length
TOL_RANK, MAX_SEP, MIN_COMMON = 3e-4, 0.01, 30
# measured (see the docstring) x 4
MP_LAM, MP_CENTRE, MP_SEP = 4 * 3.4e-16, 4 * 8.9e-16, 4 * 5.5e-18
CLEAN = dict(ball=4 * 4.4e-16, line=4 * 5.9e-16, angle=4 * 2.7e-15)
NOISY = dict(ball=4 * 5.6e-5, line=4 * 4.6e-5, angle=4 * 4.8e-4)
ANGLE_CLEAN = dict(max=4 * 2.2e-15, rms=4 * 6.7e-16)       # the unwrapped hinge angle against the planted one, rad
ANGLE_NOISY = dict(max=4 * 1.9e-2, rms=4 * 6.3e-3)         # (each frame's own 5 mrad, and frame 0's in every frame)


def scene(seed, noisy, F=2000):
    return jr.five_body_scene(seed, F, sigma_t=NOISE[0] if noisy else 0.0, sigma_r=NOISE[1] if noisy else 0.0)


def scene_figures(out, truth):
    """-> {"ball", "line", "angle"}: the ball centre's error, the hinge centre's distance to the planted line, the axis angle; the
    worse of the two bodies' sides each."""
    ball = max(np.linalg.norm(out["centre"][0, 1] - truth["ball_a"]), np.linalg.norm(out["centre"][1, 0] - truth["ball_b"]))
    line = max(jr.line_distance(out["centre"][1, 2], truth["hinge_p1"], truth["hinge_u1"]),
               jr.line_distance(out["centre"][2, 1], truth["hinge_p2"], truth["hinge_u2"]))
    angle = max(np.arcsin(min(1.0, np.linalg.norm(np.cross(out["axis"][1, 2], truth["hinge_u1"])))),
                np.arcsin(min(1.0, np.linalg.norm(np.cross(out["axis"][2, 1], truth["hinge_u2"])))))
    return {"ball": float(ball), "line": float(line), "angle": float(angle)}


def test_stacked_jacobi_equals_the_scalar_one_and_ends_within_nine_sweeps():
    for flag, Rm, t in (scene(3, True, 300)[:3], jr.session(11, 257, 9), jr.session(12, 65, 4)):
        stats = {}
        a = jr.find_joints(flag, Rm, t, 6, TOL_RANK, MAX_SEP, stats=stats)
        b = jr.find_joints(flag, Rm, t, 6, TOL_RANK, MAX_SEP, scalar=True)
        assert jr.same(a, b)
        assert 1 <= stats["sweeps"] <= 9
    # a matrix with a NaN runs to the limit and is SINGULAR; the identity pattern of a fixed pair is exact
    M = np.eye(6)
    M[0, 3] = M[3, 0] = np.nan
    lam, V, used = jr.jacobi6_scalar(M.tolist())
    assert used == jr.SWEEPS and jr.solve_pair(lam, V, [0.0] * 6, TOL_RANK)[0] == jr.SINGULAR
    M = np.eye(6)
    M[:3, 3:] = M[3:, :3] = -np.eye(3)
    lam, V, used = jr.jacobi6_scalar(M.tolist())
    assert sorted(lam) == [0.0, 0.0, 0.0, 2.0, 2.0, 2.0] and used == 1
    kind, lam3, ca, cb, xa, xb = jr.solve_pair(lam, V, [0.3, 0.0, 0.0, -0.3, 0.0, 0.0], TOL_RANK)
    assert kind == jr.FIXED and lam3 == [0.0, 0.0, 0.0] and np.isnan(xa).all() and np.isfinite(ca + cb).all()


def test_statement_against_fifty_digits():
    flag, Rm, t, _ = scene(3, True, 400)
    out = jr.find_joints(flag, Rm, t, MIN_COMMON, TOL_RANK, MAX_SEP)
    worst = {"lam": 0.0, "centre": 0.0, "sep": 0.0}
    for a, b in ((0, 1), (1, 2), (0, 3), (0, 4)):
        mp = jr.fit_mp(flag, Rm, t, a, b, TOL_RANK)
        worst["lam"] = max(worst["lam"], np.abs(np.array(mp["lam"]) - out["lam"][a, b]).max())
        worst["centre"] = max(worst["centre"], np.abs(np.array(mp["c_a"]) - out["centre"][a, b]).max(),
                              np.abs(np.array(mp["c_b"]) - out["centre"][b, a]).max())
        if out["accepted"][a, b] or out["kind"][a, b] == jr.FIXED:     # (the free pair's sep is metres: its error is relative)
            worst["sep"] = max(worst["sep"], abs(mp["sep"] - out["sep"][a, b]))
        else:
            assert abs(mp["sep"] - out["sep"][a, b]) <= 1e-15 * mp["sep"]
    print("against 50 digits:", worst)
    assert worst["lam"] <= MP_LAM and worst["centre"] <= MP_CENTRE and worst["sep"] <= MP_SEP, worst


@pytest.mark.parametrize("noisy", [False, True])
def test_five_body_scene_against_its_planted_truth(noisy):
    worst = {"ball": 0.0, "line": 0.0, "angle": 0.0}
    for seed in SEEDS:
        flag, Rm, t, truth = scene(seed, noisy)
        out = jr.find_joints(flag, Rm, t, MIN_COMMON, TOL_RANK, MAX_SEP)
        kind, acc = out["kind"], out["accepted"]
        assert kind[0, 1] == jr.BALL and kind[1, 2] == jr.HINGE and kind[0, 3] == jr.FIXED
        assert acc[0, 1] and acc[1, 2] and not acc[0, 3] and not acc[4].any() and not acc[:, 4].any()
        assert out["parent"].tolist() == [-1, 0, 1, 1, -1] and out["n_joints"] == 3          # (the docstring: why body 3 hangs on body 1)
        assert kind[1, 3] == jr.BALL and acc[1, 3] and not acc[0, 2] and not acc[2, 3]
        assert (out["cnt"] == 2000).all()
        # the margins: no kind and no acceptance rests on rounding
        lam = out["lam"][np.triu_indices(5, 1)].ravel()
        sep = out["sep"][np.triu_indices(5, 1)]
        assert np.isfinite(lam).all() and np.isfinite(sep).all()
        assert ((lam >= 10 * TOL_RANK) | (lam <= TOL_RANK / 10)).all(), lam
        assert ((sep >= 7 * MAX_SEP) | (sep <= MAX_SEP / 10)).all(), sep
        fig = scene_figures(out, truth)
        worst = {k: max(worst[k], fig[k]) for k in worst}
    print("five bodies,", "0.5 mm + 5 mrad:" if noisy else "noise-free:", worst)
    bound = NOISY if noisy else CLEAN
    assert all(worst[k] <= bound[k] for k in worst), (worst, bound)


def hinge_angle_error(series, joints, truth, f0):
    """The unwrapped hinge angle of the scene's hinge against the planted theta - theta[f0] (the axis' sign is the fit's) -> [F]."""
    h = [i for i, j in enumerate(joints) if j["kind"] == jr.HINGE][0]
    angle = jr.unwrapped_angle(series["twist"], series["present"])[h]
    sign = np.sign(joints[h]["axis_b"] @ truth["hinge_u2"])
    return angle - sign * (truth["theta"] - truth["theta"][f0])


@pytest.mark.parametrize("noisy", [False, True])
def test_series_of_the_scene_hinge_angle_and_gap(noisy):
    worst = {"max": 0.0, "rms": 0.0}
    for seed in SEEDS:
        flag, Rm, t, truth = scene(seed, noisy)
        out = jr.find_joints(flag, Rm, t, MIN_COMMON, TOL_RANK, MAX_SEP)
        poses, joints = jr.scene_poses(flag, Rm, t), jr.scene_joints(out)
        assert [(j["a"], j["b"], j["kind"]) for j in joints] == [(0, 1, jr.BALL), (1, 2, jr.HINGE), (1, 3, jr.BALL)]
        for j in joints:
            j["q_ref"], f0 = jr.first_relative(poses["quat"], flag, j["a"], j["b"])
        series = jr.joint_series(flag, poses["quat"], Rm, t, joints)
        assert (series["present"] == 1).all() and np.isnan(series["twist"][0]).all() and np.isfinite(series["twist"][1]).all()
        assert np.abs(np.sqrt((series["quat_rel"] ** 2).sum(axis=2)) - 1.0).max() < 1e-12
        assert np.abs(series["quat_rel"][:, 0] - [1.0, 0.0, 0.0, 0.0]).max() < 1e-12                 # q_ref is frame 0's own
        assert series["gap"].max() <= (1e-13 if not noisy else MAX_SEP)
        # sep is the rms of gap over the frames
        assert np.allclose(np.sqrt((series["gap"] ** 2).mean(axis=1)), [j["sep"] for j in joints], rtol=1e-9, atol=1e-15)
        err = hinge_angle_error(series, joints, truth, f0)
        worst = {"max": max(worst["max"], float(np.abs(err).max())), "rms": max(worst["rms"], float(np.sqrt((err ** 2).mean())))}
    print("hinge angle,", "0.5 mm + 5 mrad:" if noisy else "noise-free:", worst)
    bound = ANGLE_NOISY if noisy else ANGLE_CLEAN
    assert worst["max"] <= bound["max"] and worst["rms"] <= bound["rms"], (worst, bound)


def _tables(B, edges):
    acc, sep = np.zeros((B, B), dtype=np.int32), np.full((B, B), np.nan)
    for a, b, s in edges:
        acc[a, b] = acc[b, a] = 1
        sep[a, b] = sep[b, a] = s
    return acc, sep


def test_kruskal_ties_a_cycle_and_two_components():
    # a cycle of three accepted pairs: the largest sep stays out
    parent, n = jr.kruskal(*_tables(3, [(0, 1, 0.002), (1, 2, 0.001), (0, 2, 0.003)]))
    assert parent.tolist() == [-1, 0, 1] and n == 2
    parent, n = jr.kruskal(*_tables(3, [(0, 1, 0.003), (1, 2, 0.001), (0, 2, 0.002)]))
    assert parent.tolist() == [-1, 2, 0] and n == 2
    # the same bits on all three: (a, b) decides -- (0, 1), (0, 2) enter, (1, 2) closes the cycle
    parent, n = jr.kruskal(*_tables(3, [(0, 1, 0.001), (1, 2, 0.001), (0, 2, 0.001)]))
    assert parent.tolist() == [-1, 0, 0] and n == 2
    # two components and a body of no pair; the root is the lowest body whatever the edges' order
    parent, n = jr.kruskal(*_tables(7, [(3, 5, 0.001), (1, 3, 0.002), (0, 6, 0.004), (2, 6, 0.003)]))
    assert parent.tolist() == [-1, -1, 6, 1, -1, 3, 0] and n == 4
    # +0.0 and an infinite sep order as their bits do
    parent, n = jr.kruskal(*_tables(3, [(0, 1, np.inf), (1, 2, 0.0), (0, 2, 1e300)]))
    assert parent.tolist() == [-1, 2, 0] and n == 2
    parent, n = jr.kruskal(*_tables(4, []))
    assert parent.tolist() == [-1] * 4 and n == 0
