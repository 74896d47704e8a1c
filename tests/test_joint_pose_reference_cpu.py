"""The statement of "joint poses" (tests/joint_pose_reference.py) on the CPU: the lanes against the same tries in Python floats, bit
for bit; a JOINTED pose against the planted one, noise-free to rounding and with 0.5 mm of marker noise against stage 1's own error;
and the condition that keeps tests/test_gpu_joint_pose.py from passing vacuously: the scene holds every class of try the contract
names.  The scene, its poses and the statement's result are computed once and shared (the GPU tests import them from here)."""
import functools

import numpy as np

import body_session_reference as bsr
import joint_pose_reference as jp

INF = float("inf")
SEED, F_SCENE, MAX_RMS, AXIS_LEN, ROUNDS = 3, 1500, 0.005, 0.1, 4


@functools.lru_cache(maxsize=None)
def scene(sigma=0.0, outliers=0.02, max_rms=MAX_RMS):
    """-> (t, traj, bodies, joints, truth, stage 1's poses, the statement's result, its trace); read-only for every user."""
    t, traj, bodies, joints, truth = jp.five_body_session(SEED, F=F_SCENE, sigma=sigma, outliers=outliers)
    poses = bsr.pose_rows(traj, bodies, max_rms)
    trace = {}
    ref = jp.pose_joints(traj, bodies, poses["flag"], poses["quat"], poses["R"], poses["t_pose"], joints, AXIS_LEN, max_rms, ROUNDS, trace=trace)
    for a in (t, traj, *poses.values(), *ref.values()):
        a.setflags(write=False)
    return t, traj, bodies, joints, truth, poses, ref, trace


def test_lanes_equal_the_scalar_tries_bit_for_bit():
    _, traj, bodies, joints, _, poses, ref, _ = scene()
    sc = jp.pose_joints(traj, bodies, poses["flag"], poses["quat"], poses["R"], poses["t_pose"], joints, AXIS_LEN, MAX_RMS, ROUNDS, scalar=True)
    assert jp.same(sc, ref)
    # and on a tree with NaN and huge values inside an anchor's pose
    traj, bodies, joints, _ = jp.tree_session(11, 300, [-1, 0, 1, 1, 3])
    p = {k: v.copy() for k, v in bsr.pose_rows(traj, bodies, INF).items()}
    f = np.arange(300)
    p["R"][0, f % 7 == 3, 1, 1] = np.nan
    p["t_pose"][0, f % 7 == 5, 2] = 1e200
    args = (traj, bodies, p["flag"], p["quat"], p["R"], p["t_pose"], joints, AXIS_LEN, INF, ROUNDS)
    assert jp.same(jp.pose_joints(*args, scalar=True), jp.pose_joints(*args))


def test_the_scene_holds_every_class_of_try():
    _, _, _, joints, _, poses, ref, tr = scene()
    assert jp.validate(5, joints, AXIS_LEN, MAX_RMS, ROUNDS) is None
    assert tr[(jp.BALL, 2, "ok")] > 0                                     # BALL with k = 2 succeeding
    assert tr[(jp.BALL, 1, "impossible")] > 0 and (jp.BALL, 1, "ok") not in tr and (jp.BALL, 1, "rms") not in tr
    assert tr[(jp.HINGE, 1, "ok")] > 0                                    # HINGE with k = 1 succeeding
    assert tr[(jp.HINGE, 1, "impossible")] > 0                            # ... and with its marker on the axis
    assert tr["rescued"] > 0                                              # a DEGENERATE set rescued
    assert tr[(jp.BALL, 2, "rms")] > 0 and tr[(jp.HINGE, 1, "rms")] > 0   # tries failing on max_rms
    assert tr[("hops", 2)] > 0 and tr[("hops", 3)] > 0
    assert tr["contested"] > 0                                            # two joints open in one round: the lower index wins
    flag, fj = poses["flag"], ref["flag"]
    assert (flag == jp.RMS).any() and np.array_equal(fj[flag == jp.RMS], flag[flag == jp.RMS])       # RMS frames left alone
    assert np.isnan(ref["R"][flag == jp.RMS]).all() and (ref["hops"][flag == jp.RMS] == -1).all()
    hidden = (flag == jp.FEW) | (flag == jp.DEGENERATE)
    share = (fj[hidden] == jp.JOINTED).mean()
    print(f"recovered {int((fj[hidden] == jp.JOINTED).sum())} of {int(hidden.sum())} FEW/DEGENERATE frames ({100 * share:.1f} %)")
    assert share > 0.25
    # the books: hops, via and the doubles agree with the flags
    j = fj == jp.JOINTED
    assert (ref["hops"][j] >= 1).all() and (ref["via"][j] >= 0).all() and np.isfinite(ref["quat"][j]).all() and (ref["rms_j"][j] <= MAX_RMS).all()
    assert (ref["hops"][flag == jp.POSED] == 0).all() and np.isnan(ref["rms_j"][~j]).all()
    rest = ~j & (flag != jp.POSED)
    assert (ref["hops"][rest] == -1).all() and (ref["via"][~j] == -1).all() and np.isnan(ref["quat"][rest]).all()
    # a jointed pose comes from a body one hop nearer
    for b, f in np.argwhere(j)[:200]:
        jt = joints[ref["via"][b, f]]
        x = jt["b"] if jt["a"] == b else jt["a"]
        assert ref["hops"][x, f] == ref["hops"][b, f] - 1


def _angle(Ra, Rb):
    c = (np.trace(np.einsum("nij,nkj->nik", Ra, Rb), axis1=1, axis2=2) - 1.0) / 2.0
    return np.arccos(np.clip(c, -1.0, 1.0))


def _marker_error(q, R, t, Rt, tt):
    """Per frame the rms distance between the body's markers under the two poses."""
    q = np.asarray(q)
    d = (np.einsum("nij,mj->nmi", R, q) + t[:, None]) - (np.einsum("nij,mj->nmi", Rt, q) + tt[:, None])
    return np.sqrt((d ** 2).sum(axis=2).mean(axis=1))


def test_a_jointed_pose_equals_the_planted_one_without_noise():
    _, _, _, _, truth, _, ref, _ = scene()
    clean = ~truth["outlier"].any(axis=0)                       # (a frame with a mislabelled sample has no planted answer)
    j = (ref["flag"] == jp.JOINTED) & clean[None, :]
    assert j.sum() > 400 and all(((ref["hops"] == h) & j).any() for h in (1, 2, 3))
    # 1e-11: the fits are exact up to rounding (the measured maxima are 8e-13 in R and 3e-14 m in t, three hops deep)
    assert np.abs(ref["R"][j] - truth["R"][j]).max() < 1e-11 and np.abs(ref["t_pose"][j] - truth["t"][j]).max() < 1e-11


# measured on this scene with 0.5 mm of marker noise, no outliers, max_rms = inf (printed below): the rms over frames
# of the markers' rms displacement between the fitted and the planted pose
STAGE1_FULL_MM, JOINTED_MM, JOINTED_RAD = 0.567, 2.17, 0.0230


def test_accuracy_with_half_a_millimetre_of_noise():
    _, _, bodies, _, truth, poses, ref, _ = scene(sigma=0.0005, outliers=0.0, max_rms=INF)
    full, jointed, angles = [], [], []
    for b in range(4):
        q = bodies[b][1]
        own = (poses["flag"][b] == jp.POSED) & (poses["n_used"][b] == len(q))
        j = ref["flag"][b] == jp.JOINTED
        full.append(_marker_error(q, poses["R"][b][own], poses["t_pose"][b][own], truth["R"][b][own], truth["t"][b][own]))
        jointed.append(_marker_error(q, ref["R"][b][j], ref["t_pose"][b][j], truth["R"][b][j], truth["t"][b][j]))
        angles.append(_angle(ref["R"][b][j], truth["R"][b][j]))
    full, jointed, angles = (np.sqrt((np.concatenate(v) ** 2).mean()) for v in (full, jointed, angles))
    print(f"stage 1, fully seen: {1e3 * full:.3f} mm; jointed: {1e3 * jointed:.3f} mm, {angles:.4f} rad; ratio {jointed / full:.2f}")
    assert 1e3 * full < 4 * STAGE1_FULL_MM and 1e3 * jointed < 4 * JOINTED_MM and angles < 4 * JOINTED_RAD
    assert jointed < 4 * (JOINTED_MM / STAGE1_FULL_MM) * full      # against stage 1's own error on the same bodies


def test_validate_names_every_refused_rule():
    _, _, _, joints, _, _, _, _ = scene()
    ok = dict(B=5, joints=joints, axis_len=0.1, max_rms=INF, max_rounds=4)
    assert jp.validate(**ok) is None

    def with_joint(i, **kw):
        return [dict(j, **kw) if n == i else j for n, j in enumerate(joints)]

    bad = [dict(ok, B=1), dict(ok, B=65), dict(ok, joints=[]), dict(ok, joints=joints + [dict(joints[0], a=2, b=4), dict(joints[0], a=3, b=4)]),
           dict(ok, axis_len=0.0), dict(ok, axis_len=float("nan")), dict(ok, axis_len=INF), dict(ok, max_rms=0.0), dict(ok, max_rms=float("nan")),
           dict(ok, max_rounds=0), dict(ok, max_rounds=17), dict(ok, joints=with_joint(0, kind=2)), dict(ok, joints=with_joint(0, a=5)),
           dict(ok, joints=with_joint(0, a=1)), dict(ok, joints=with_joint(2, a=2, b=0)), dict(ok, joints=with_joint(2, a=1, b=0)),
           dict(ok, joints=with_joint(0, c_a=[0.0, float("nan"), 0.0])), dict(ok, joints=with_joint(1, axis_a=[0.0, 0.0, 1.001])),
           dict(ok, joints=with_joint(1, axis_b=[0.0, INF, 1.0]))]
    assert all(jp.validate(**b) is not None for b in bad)
    assert jp.validate(**dict(ok, joints=with_joint(0, axis_a=[float("nan")] * 3))) is None       # a BALL's axes are not read
