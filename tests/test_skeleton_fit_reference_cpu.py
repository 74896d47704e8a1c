"""The statement of "skeleton fit" (tests/skeleton_fit_reference.py) on the CPU: the lanes against the same text in Python floats,
bit for bit; the tree elimination's step against a dense solve of the assembled system; the analytic blocks against central
differences of the residuals; the cost never above the start's; a frame without an active joint left where Horn's fit put it; the
accuracy on the five-body scene beside "joint poses"' own; and every refused rule.  The scene and the statement's result are
computed once and shared (the GPU tests import them from here)."""
import functools

import numpy as np

import body_session_reference as bsr
import joint_pose_reference as jp
import skeleton_fit_reference as sk
import test_joint_pose_reference_cpu as jcpu

INF, NAN = float("inf"), float("nan")
AXIS_LEN, W_JOINT, ITERS = 0.1, 1.0, 8


@functools.lru_cache(maxsize=None)
def scene(w_joint=W_JOINT):
    """The five-body scene with 0.5 mm of noise, no mislabelled samples, max_rms = inf, after "joint poses"' stage
    -> (t, traj, bodies, joints, truth, stage 1's poses, the jointed poses, the fit); read-only for every user."""
    t, traj, bodies, joints, truth, poses, pj, _ = jcpu.scene(sigma=0.0005, outliers=0.0, max_rms=INF)
    fit = sk.fit_skeleton(traj, bodies, pj["flag"], pj["quat"], pj["t_pose"], joints, AXIS_LEN, w_joint, ITERS)
    for a in fit.values():
        a.setflags(write=False)
    return t, traj, bodies, joints, truth, poses, pj, fit


def tree(seed, F, parent, sigma=0.0005, **kw):
    """A tree session after stage 1 and "joint poses" -> traj, bodies, joints, the jointed poses"""
    traj, bodies, joints, _ = jp.tree_session(seed, F, parent, sigma=sigma, **kw)
    p = bsr.pose_rows(traj, bodies, INF)
    return traj, bodies, joints, jp.pose_joints(traj, bodies, p["flag"], p["quat"], p["R"], p["t_pose"], joints)


def fit(traj, bodies, pj, joints, axis_len=AXIS_LEN, w_joint=W_JOINT, iters=ITERS, **kw):
    return sk.fit_skeleton(traj, bodies, pj["flag"], pj["quat"], pj["t_pose"], joints, axis_len, w_joint, iters, **kw)


# ---------------------------------------------------------------- lanes = scalar
def test_lanes_equal_the_scalar_statement_bit_for_bit():
    traj, bodies, joints, pj = tree(11, 60, [-1, 0, 1, 1, 3])
    assert sk.same(fit(traj, bodies, pj, joints, iters=4, scalar=True), fit(traj, bodies, pj, joints, iters=4))
    # NaN and huge values in a marker and in a start pose, a weight at either end, two components
    traj, bodies, joints, pj = tree(12, 56, [-1, 0, -1, 2, 3])
    pj = {k: v.copy() for k, v in pj.items()}
    f = np.arange(56)
    row = bodies[1][0][0]
    traj[row, f % 11 == 2, 1] = np.nan
    traj[row, f % 11 == 4, 0] = 1e200
    traj[row, f % 11 == 6, 2] = -1e200
    pj["t_pose"][0, f % 7 == 5, 2] = 1e200
    pj["t_pose"][3, f % 7 == 6, 0] = -1e200
    pj["quat"][0, f % 13 == 1, 2] = np.nan
    for w in (1e-6, 1e6):
        lanes = fit(traj, bodies, pj, joints, w_joint=w, iters=3)
        assert sk.same(fit(traj, bodies, pj, joints, w_joint=w, iters=3, scalar=True), lanes)
    bad = ~np.isfinite(lanes["cost0"])                          # a start cost that is not finite: the frame is left as it came
    assert bad.sum() > 10 and (lanes["steps"][bad] == 0).all() and (lanes["steps"][~bad] > 0).any()


# ---------------------------------------------------------------- the solve
def _scalar_frames(traj, bodies, pj, joints, w_joint=W_JOINT):
    return sk.frames_of(traj, bodies, pj["flag"], pj["quat"], pj["t_pose"], joints, AXIS_LEN, w_joint, scalar=True)


def test_tree_elimination_equals_a_dense_solve():
    """A chain of 5, a star and two components, their trees cut by the bodies "joint poses" could not pose: the step of the
    elimination against numpy.linalg.solve on the assembled 6A x 6A system, relative to the step's largest entry.  1e-9: both
    solve a system whose condition (lam = 1e-3 on the diagonal) is below 1e6 in double precision; the measured maximum is printed."""
    worst, cuts, sizes = 0.0, 0, set()
    for seed, parent in ((21, [-1, 0, 1, 2, 3]), (22, [-1, 0, 0, 0, 0, 0]), (23, [-1, 0, 1, -1, 3, 3])):
        traj, bodies, joints, pj = tree(seed, 40, parent, shares={0: 0.1, 1: 0.15, 2: 0.1})
        for fr, q, t in _scalar_frames(traj, bodies, pj, joints):
            if not any(fr.act):
                continue
            _, _, H, g, C = sk.terms(fr, q, t, 1e-3)
            delta, piv = sk.step(fr, H, g, C)
            ids, A, rhs = sk.dense_system(fr, H, g, C)
            assert piv
            x = -np.linalg.solve(A, rhs)
            mine = np.array([delta[b] for b in ids]).reshape(-1)
            worst = max(worst, np.abs(x - mine).max() / np.abs(x).max())
            cuts += any(not fr.act[b] and any(fr.act[c] for c in range(fr.B) if fr.tb["parent"][c] == b) for b in range(fr.B))
            sizes.add(len(ids))
    print(f"tree elimination against the dense solve: {worst:.2e} of the step's largest entry; {cuts} frames with a cut tree")
    assert worst < 1e-9 and cuts > 10 and {2, 3, 4, 5, 6} <= sizes


def _residuals(fr, q, t):
    """The stacked residual vector of a scalar frame, written independently of the statement: sqrt(w) r per point."""
    out = []
    R = [np.array(bsr.quat_to_R(*q[b])).reshape(3, 3) for b in range(fr.B)]
    for b in range(fr.B):
        if fr.act[b]:
            out += [R[b] @ np.array(fr.Q[b][m]) + np.array(t[b]) - np.array(fr.P[b][m]) for m in range(len(fr.Q[b])) if fr.pres[b][m]]
    for c in range(fr.B):
        for (j, x, hinge, up, c_y, ax_y, c_x, ax_x) in fr.tb["dirs"][c]:
            if not up or not (fr.act[c] and fr.act[x]):
                continue
            wc, wx = R[c] @ np.array(c_y) + np.array(t[c]), R[x] @ np.array(c_x) + np.array(t[x])
            out.append(np.sqrt(fr.w) * (wc - wx))
            if hinge:
                out.append(np.sqrt(fr.w) * ((wc + fr.len * (R[c] @ np.array(ax_y))) - (wx + fr.len * (R[x] @ np.array(ax_x)))))
    return np.concatenate(out)


def test_blocks_equal_central_differences_of_the_residuals():
    """J^T J and J^T r with J from central differences (h = 1e-6) of the residual vector along the statement's own update: the
    update's rotation differs from the exponential map at the third order of h, the difference quotient's error is of order h^2
    = 1e-12 and its rounding of order 1e-16 / h = 1e-10 per entry of J, whose entries are of order 1: 1e-8 of the largest entry of
    J^T J.  J^T r sums those errors times residuals of 1e-3 m into a gradient that has cancelled to some 1e-5 of its terms near the
    optimum, where the same absolute error weighs a hundred times more: 1e-6.  The measured maxima are printed."""
    traj, bodies, joints, pj = tree(24, 12, [-1, 0, 1, 1, 3], shares={0: 0.1})
    h, worst_H, worst_g, n = 1e-6, 0.0, 0.0, 0
    for w in (1.0, 7.0):
        for fr, q, t in _scalar_frames(traj, bodies, pj, joints, w)[:6]:
            _, _, H, g, C = sk.terms(fr, q, t, 0.0)
            ids, A, rhs = sk.dense_system(fr, H, g, C)
            r0 = _residuals(fr, q, t)
            J = np.zeros((r0.size, 6 * len(ids)))
            for n_b, b in enumerate(ids):
                for e in range(6):
                    side = []
                    for s in (h, -h):
                        d = [0.0] * 6
                        d[e] = s
                        qq, tt = [list(v) for v in q], [list(v) for v in t]
                        qq[b], tt[b] = sk._update(sk.Scalar, q[b], t[b], d)
                        side.append(_residuals(fr, qq, tt))
                    J[:, 6 * n_b + e] = (side[0] - side[1]) / (2 * h)
            worst_H = max(worst_H, np.abs(J.T @ J - A).max() / np.abs(A).max())
            worst_g = max(worst_g, np.abs(J.T @ r0 - rhs).max() / max(np.abs(rhs).max(), 1e-300))
            n += len(ids) >= 4
    print(f"blocks against central differences: H {worst_H:.2e}, g {worst_g:.2e} of the largest entry")
    assert worst_H < 1e-8 and worst_g < 1e-6 and n >= 6


def test_cost_never_above_the_start_and_the_books():
    _, _, _, joints, _, _, pj, o = scene()
    assert (o["cost"] <= o["cost0"]).all() and (o["cost"][o["steps"] > 0] < o["cost0"][o["steps"] > 0]).all()
    assert np.array_equal(o["cost"][o["steps"] == 0], o["cost0"][o["steps"] == 0]) and (o["steps"] <= ITERS).all() and (o["steps"] > 0).mean() > 0.9
    on = (pj["flag"] == jp.POSED) | (pj["flag"] == jp.JOINTED)
    assert np.array_equal(o["n_act"], sum((on[j["a"]] & on[j["b"]]).astype(np.int32) for j in joints))
    assert np.isfinite(o["quat"][on]).all() and np.isnan(o["quat"][~on]).all() and np.isnan(o["R"][~on]).all() and np.isnan(o["rms_s"][~on]).all()
    assert np.abs(np.linalg.norm(o["quat"][on], axis=1) - 1.0).max() < 1e-15 * 4
    for b in range(len(on)):                                   # one hemisphere along the carrying frames
        q = o["quat"][b][on[b]]
        assert (np.einsum("fi,fi->f", q[1:], q[:-1]) >= 0).all()


# measured (printed below): the largest marker displacement between Horn's pose and the fit's, metres, with every joint inactive:
# rounding of coordinates near 1 m
NO_JOINT_MOVE_M = 7.0e-16


def test_without_an_active_joint_the_fit_stays_at_horns_optimum():
    traj, bodies, joints, pj = tree(25, 200, [-1, 0, 1, 2, 3], shares={})
    pj = {k: v.copy() for k, v in pj.items()}
    pj["flag"][1::2] = jp.FEW                                   # every second body of the chain inactive: no joint has both its bodies
    o = fit(traj, bodies, pj, joints)
    assert (o["n_act"] == 0).all() and (o["cost"] <= o["cost0"]).all()
    move = 0.0
    for b in (0, 2, 4):
        q = np.asarray(bodies[b][1])
        d = (np.einsum("fij,mj->fmi", o["R"][b], q) + o["t_pose"][b][:, None]) - (np.einsum("fij,mj->fmi", pj["R"][b], q) + pj["t_pose"][b][:, None])
        move = max(move, np.linalg.norm(d, axis=2).max())
    print(f"no active joint: the fit moves a marker by at most {move:.2e} m from Horn's pose")
    assert move < 4 * NO_JOINT_MOVE_M and np.isnan(o["quat"][1::2]).all()


# ---------------------------------------------------------------- accuracy
# measured on the scene (printed below), w_joint = 1: the rms over frames of the markers' rms displacement between the
# pose and the planted one, before (the jointed poses: 2.17 mm is 3.7t's own figure) and after the fit, and the rms joint gap
JOINTED_BEFORE_MM, JOINTED_AFTER_MM, POSED_BEFORE_MM, POSED_AFTER_MM, GAP_BEFORE_MM, GAP_AFTER_MM = 2.17, 1.11, 0.616, 0.518, 2.05, 0.350


def _errors(bodies, joints, truth, flag, R, t):
    on = (flag == jp.POSED) | (flag == jp.JOINTED)
    per = {jp.JOINTED: [], jp.POSED: []}
    for b in range(4):
        for kind in per:
            at = flag[b] == kind
            per[kind].append(jcpu._marker_error(bodies[b][1], R[b][at], t[b][at], truth["R"][b][at], truth["t"][b][at]))
    gap = []
    for jt in joints:
        a, b = jt["a"], jt["b"]
        at = on[a] & on[b]
        gap.append(np.linalg.norm((np.einsum("fij,j->fi", R[a][at], np.asarray(jt["c_a"])) + t[a][at]) -
                                  (np.einsum("fij,j->fi", R[b][at], np.asarray(jt["c_b"])) + t[b][at]), axis=1))
    rms = lambda v: 1e3 * float(np.sqrt((np.concatenate(v) ** 2).mean()))
    return rms(per[jp.JOINTED]), rms(per[jp.POSED]), rms(gap)


def test_accuracy_beside_joint_poses_own():
    _, traj, bodies, joints, truth, _, pj, o = scene()
    jb, pb, gb = _errors(bodies, joints, truth, pj["flag"], pj["R"], pj["t_pose"])
    ja, pa, ga = _errors(bodies, joints, truth, pj["flag"], o["R"], o["t_pose"])
    print(f"w_joint = 1: JOINTED {jb:.3f} -> {ja:.3f} mm, POSED {pb:.3f} -> {pa:.3f} mm, joint gap {gb:.3f} -> {ga:.3f} mm")
    for w in (0.1, 10.0, 100.0):
        ow = fit(traj, bodies, pj, joints, w_joint=w)
        print(f"w_joint = {w:g}: JOINTED {{:.3f}} mm, POSED {{:.3f}} mm, joint gap {{:.3f}} mm".format(*_errors(bodies, joints, truth, pj["flag"], ow["R"], ow["t_pose"])))
    assert jb < 4 * JOINTED_BEFORE_MM and pb < 4 * POSED_BEFORE_MM and gb < 4 * GAP_BEFORE_MM
    assert ja < 4 * JOINTED_AFTER_MM and pa < 4 * POSED_AFTER_MM and ga < 4 * GAP_AFTER_MM
    assert ja < jb and pa < pb and ga < gb                      # the fit is better than 3.7t's stage on every figure


# ---------------------------------------------------------------- refusals
def test_validate_names_every_refused_rule():
    _, _, _, joints, _, _, _, _ = scene()
    ok = dict(B=5, joints=joints, axis_len=0.1, w_joint=1.0, iters=8)
    assert sk.validate(**ok) is None and sk.validate(**dict(ok, iters=1)) is None and sk.validate(**dict(ok, iters=16, w_joint=5e-324)) is None

    def with_joint(i, **kw):
        return [dict(j, **kw) if n == i else j for n, j in enumerate(joints)]

    bad = [dict(ok, B=1), dict(ok, B=65), dict(ok, joints=[]), dict(ok, joints=joints + [dict(joints[0], a=2, b=4), dict(joints[0], a=3, b=4)]),
           dict(ok, axis_len=0.0), dict(ok, axis_len=NAN), dict(ok, axis_len=INF), dict(ok, w_joint=0.0), dict(ok, w_joint=NAN),
           dict(ok, w_joint=INF), dict(ok, w_joint=-1.0), dict(ok, iters=0), dict(ok, iters=17), dict(ok, joints=with_joint(0, kind=2)),
           dict(ok, joints=with_joint(0, a=5)), dict(ok, joints=with_joint(0, a=1)), dict(ok, joints=with_joint(2, a=2, b=0)),
           dict(ok, joints=with_joint(2, a=1, b=0)), dict(ok, joints=with_joint(0, c_a=[0.0, NAN, 0.0])),
           dict(ok, joints=with_joint(1, axis_a=[0.0, 0.0, 1.001])), dict(ok, joints=with_joint(1, axis_b=[0.0, INF, 1.0]))]
    assert all(sk.validate(**b) is not None for b in bad)
    assert sk.validate(**dict(ok, joints=with_joint(0, axis_a=[NAN] * 3))) is None       # a BALL's axes are not read
