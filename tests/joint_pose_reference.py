"""The "joint poses" contract of include/mocap_core.h in plain Python and NumPy, in the order the header writes.

    validate(B, joints, axis_len, max_rms, max_rounds)   None, or the reason the core returns MOCAP_E_ARG for (the joints and the three
                                                         parameters; the bodies and the session are body_session_reference.validate's)
    dir_mask(Q, virtual)                                 a directed joint's table: [2^N] bools over the present subsets
    pose_joints(traj, bodies, flag, quat, Rm, t_pose, joints, axis_len, max_rms, max_rounds)
                                                         THE statement, lanes over frames -> {"flag", "hops", "via", "quat", "R",
                                                         "t_pose", "rms_j"}; scalar=True: every try in Python floats
                                                         (body_session_reference.pose_sample), asserted equal bit for bit in
                                                         tests/test_joint_pose_reference_cpu.py; the device is compared with the lanes
    tree_session(seed, F, parent, ...)                   a session of bodies hung on each other by planted ball joints and hinges
    five_body_session(seed, F, ...)                      joints_reference.five_body_scene's poses with 4-5 markers per body, marker
                                                         dropout that leaves bodies at 0, 1, 2 and 3-collinear visible markers, and the
                                                         planted joints

The fit and the sign walk are body_session_reference's (_fit_lanes, sign_walk, pose_sample); the spanning rule is
rigid_body_reference's.  joints = [{"a", "b", "kind", "c_a", "c_b", "axis_a", "axis_b"}]."""
import math

import numpy as np

import body_session_reference as bsr
import joints_reference as jr
import rigid_body_reference as rbr
import rigid_groups_reference as rg

POSED, FEW, DEGENERATE, RMS, JOINTED = 1, 2, 4, 8, 16
HINGE, BALL = jr.HINGE, jr.BALL
MAX_ROUNDS = 16
NAN = float("nan")
INT_OUT = ("flag", "hops", "via")
F64_OUT = ("quat", "R", "t_pose", "rms_j")

same_bits = bsr.same_bits


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in INT_OUT) and all(same_bits(a[k].reshape(b[k].shape), b[k]) for k in F64_OUT)


# ---------------------------------------------------------------------------------------------------------------------- the host's part
def validate(B, joints, axis_len, max_rms, max_rounds):
    J = len(joints)
    if not 2 <= B <= 64:
        return "B"
    if not 1 <= J <= B - 1:
        return "J"
    if not (axis_len > 0.0 and math.isfinite(axis_len)):
        return "axis_len"
    if not max_rms > 0.0:
        return "max_rms"
    if not 1 <= max_rounds <= MAX_ROUNDS:
        return "max_rounds"
    top = list(range(B))
    for jt in joints:
        a, b = int(jt["a"]), int(jt["b"])
        if not (0 <= a < B and 0 <= b < B):
            return "body out of range"
        if a == b:
            return "a == b"
        if int(jt["kind"]) not in (HINGE, BALL):
            return "kind"
        if not (np.isfinite(np.asarray(jt["c_a"], dtype=np.float64)).all() and np.isfinite(np.asarray(jt["c_b"], dtype=np.float64)).all()):
            return "centre"
        if int(jt["kind"]) == HINGE:
            for key in ("axis_a", "axis_b"):
                x, y, z = (float(v) for v in jt[key])
                if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
                    return "axis not finite"
                if not abs(((x * x + y * y) + z * z) - 1.0) <= 1e-6:
                    return "axis norm"
        while top[a] != a:
            a = top[a]
        while top[b] != b:
            b = top[b]
        if a == b:
            return "no forest"
        top[max(a, b)] = min(a, b)
    return None


def dir_mask(Q, virtual):
    """Q [N][3] the body's markers, virtual [nv][3] -> [2^N] bools: the subset with every virtual point holds a spanning triple."""
    pts = [[float(v) for v in row] for row in list(np.asarray(Q, dtype=np.float64).reshape(-1, 3)) + [list(v) for v in virtual]]
    n, npt = len(pts) - len(virtual), len(pts)
    good = [(i, j, k) for i in range(npt) for j in range(i + 1, npt) for k in range(j + 1, npt) if rbr.triple_spans(pts[i], pts[j], pts[k])]
    virt = ((1 << len(virtual)) - 1) << n
    return [any(((s | virt) >> i & 1) and ((s | virt) >> j & 1) and ((s | virt) >> k & 1) for (i, j, k) in good) for s in range(1 << n)]


def directed(joints, y, axis_len):
    """The joints of body y in ascending joint index, as y sees them -> [(j, x, hinge, v0, v1, c_x, ax_x)] in Python floats."""
    out = []
    for j, jt in enumerate(joints):
        if int(jt["a"]) == y:
            x, c_y, c_x, ax_y, ax_x = int(jt["b"]), jt["c_a"], jt["c_b"], jt.get("axis_a"), jt.get("axis_b")
        elif int(jt["b"]) == y:
            x, c_y, c_x, ax_y, ax_x = int(jt["a"]), jt["c_b"], jt["c_a"], jt.get("axis_b"), jt.get("axis_a")
        else:
            continue
        hinge = int(jt["kind"]) == HINGE
        v0 = [float(v) for v in c_y]
        v1 = [v0[i] + axis_len * float(ax_y[i]) for i in range(3)] if hinge else None
        out.append((j, x, hinge, v0, v1, [float(v) for v in c_x], [float(v) for v in ax_x] if hinge else None))
    return out


# ---------------------------------------------------------------------------------------------------------------------- THE statement
def pose_joints(traj, bodies, flag, quat, Rm, t_pose, joints, axis_len=0.1, max_rms=float("inf"), max_rounds=4, scalar=False, trace=None):
    """trace: a dict that receives counters: (kind, k, outcome) per try with outcome in "impossible", "ok", "rms", "not finite";
    "contested": successes where a later joint of the body was open and possible in the same round; ("hops", r): poses set in round r;
    "rescued": DEGENERATE frames that end JOINTED."""
    traj = np.asarray(traj, dtype=np.float64)
    _, F, _ = traj.shape
    B = len(bodies)
    flag = np.asarray(flag, dtype=np.int32).reshape(B, F)
    quat = np.asarray(quat, dtype=np.float64).reshape(B, F, 4)
    Rm = np.asarray(Rm, dtype=np.float64).reshape(B, F, 9)
    t_pose = np.asarray(t_pose, dtype=np.float64).reshape(B, F, 3)
    axis_len = float(axis_len)
    posed = flag == POSED
    out = {"flag": flag.copy(), "hops": np.where(posed, 0, -1).astype(np.int32), "via": np.full((B, F), -1, dtype=np.int32),
           "quat": np.where(posed[:, :, None], quat, NAN), "R": np.where(posed[:, :, None], Rm, NAN),
           "t_pose": np.where(posed[:, :, None], t_pose, NAN), "rms_j": np.full((B, F), NAN)}
    hops, Rj, tj = out["hops"], out["R"], out["t_pose"]
    count = (lambda key, n=1: trace.__setitem__(key, trace.get(key, 0) + int(n))) if trace is not None else (lambda key, n=1: None)
    per_body = []
    for y, (rows, markers) in enumerate(bodies):
        Q = np.asarray(markers, dtype=np.float64).reshape(-1, 3)
        P = traj[np.asarray(rows, dtype=np.int64)]                     # [N][F][3]
        pm = np.isfinite(P).all(axis=2)                                # [N][F]
        pres = (pm.astype(np.int64) << np.arange(Q.shape[0])[:, None]).sum(axis=0)
        dirs = [d + (np.array(dir_mask(Q, [d[3]] + ([d[4]] if d[2] else []))),) for d in directed(joints, y, axis_len)]
        per_body.append((Q, P, pm, pres, dirs))
    with np.errstate(all="ignore"):
        for r in range(1, max_rounds + 1):
            for y in range(B):
                Q, P, pm, pres, dirs = per_body[y]
                N = Q.shape[0]
                cand = (hops[y] == -1) & ((flag[y] == FEW) | (flag[y] == DEGENERATE))
                for i, (j, x, hinge, v0, v1, c_x, ax_x, mask) in enumerate(dirs):
                    open_ = cand & (hops[y] == -1) & (hops[x] == r - 1)
                    possible = mask[pres]
                    kind = HINGE if hinge else BALL
                    if trace is not None:
                        for k in np.unique(pm[:, open_ & ~possible].sum(axis=0)):
                            count((kind, int(k), "impossible"), (pm[:, open_ & ~possible].sum(axis=0) == k).sum())
                    at = np.flatnonzero(open_ & possible)
                    if at.size == 0:
                        continue
                    Rx, tx = Rj[x][at], tj[x][at]
                    w0 = [((Rx[:, 3 * c] * c_x[0] + Rx[:, 3 * c + 1] * c_x[1]) + Rx[:, 3 * c + 2] * c_x[2]) + tx[:, c] for c in range(3)]
                    pts, model, on = [P[m][at] for m in range(N)], [Q[m] for m in range(N)], [pm[m][at] for m in range(N)]
                    pts.append(np.stack(w0, axis=1))
                    model.append(v0)
                    on.append(np.ones(at.size, dtype=bool))
                    if hinge:
                        u = [(Rx[:, 3 * c] * ax_x[0] + Rx[:, 3 * c + 1] * ax_x[1]) + Rx[:, 3 * c + 2] * ax_x[2] for c in range(3)]
                        pts.append(np.stack([w0[c] + axis_len * u[c] for c in range(3)], axis=1))
                        model.append(v1)
                        on.append(np.ones(at.size, dtype=bool))
                    if scalar:
                        q4, R9, t3, rms = np.zeros((at.size, 4)), np.zeros((at.size, 9)), np.zeros((at.size, 3)), np.zeros(at.size)
                        for n in range(at.size):
                            use = [m for m in range(len(pts)) if on[m][n]]
                            q4[n], R9[n], t3[n], rms[n] = bsr.pose_sample([pts[m][n].tolist() for m in use], [model[m] for m in use])
                    else:
                        q4, R9, t3, rms = bsr._fit_lanes(pts, np.array(on), model)
                    finite = np.isfinite(q4).all(axis=1)
                    ok = finite & (rms <= max_rms)
                    if trace is not None:
                        ks = pm[:, at].sum(axis=0)
                        for k in np.unique(ks):
                            for name, sel in (("ok", ok), ("not finite", ~finite), ("rms", finite & ~ok)):
                                count((kind, int(k), name), (sel & (ks == k)).sum())
                        later = np.zeros(at.size, dtype=bool)
                        for (_, x2, _, _, _, _, _, mask2) in dirs[i + 1:]:
                            later |= (hops[x2][at] == r - 1) & mask2[pres[at]]
                        count("contested", (ok & later).sum())
                        count(("hops", r), ok.sum())
                    won = at[ok]
                    out["flag"][y, won], out["via"][y, won], out["rms_j"][y, won] = JOINTED, j, rms[ok]
                    out["quat"][y, won], Rj[y, won], tj[y, won] = q4[ok], R9[ok], t3[ok]
                    hops[y, won] = r
    if trace is not None:
        count("rescued", ((flag == DEGENERATE) & (out["flag"] == JOINTED)).sum())
    for b in range(B):
        s = bsr.sign_walk(out["quat"][b], (out["flag"][b] == POSED) | (out["flag"][b] == JOINTED))
        out["quat"][b] = np.where(s[:, None] == 1, -out["quat"][b], out["quat"][b])
    out["R"] = out["R"].reshape(B, F, 3, 3)
    return out


def fill_flag(flag_j):
    """The flag mocap_fill_rows and mocap_joint_series are given: JOINTED reads POSED."""
    return np.where(flag_j == JOINTED, POSED, flag_j).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------- scenes
def _templates(rng, n_markers, size=0.12):
    out = []
    for N in n_markers:
        while True:
            q = rng.uniform(-size, size, (N, 3))
            if rbr.posable_table(q)[-1]:
                out.append(q)
                break
    return out


def _rows_of(templates, Rm, t, n_loose, rng, tau):
    rows, bodies = [], []
    for b, q in enumerate(templates):
        bodies.append((list(range(len(rows), len(rows) + len(q))), q))
        for m in range(len(q)):
            rows.append(np.einsum("fij,j->fi", Rm[b], q[m]) + t[b])
    for _ in range(n_loose):
        rows.append(rg.rigid_motion(rng, tau, 1.0)[1])
    return np.array(rows), bodies


def _hide(rng, traj, bodies, shares, patterns=None):
    """Per (body, frame) the number of visible markers is drawn: shares = {k: probability}, the rest fully seen; the visible subset is
    random, or one of patterns[b][k] (a list of marker tuples) with probability one half."""
    F = traj.shape[1]
    ks, ps = list(shares), np.array([shares[k] for k in shares])
    for b, (rows, q) in enumerate(bodies):
        N = len(rows)
        pick = rng.choice(len(ks) + 1, size=F, p=np.append(ps, 1.0 - ps.sum()))
        for f in np.flatnonzero(pick < len(ks)):
            k = min(ks[pick[f]], N)
            keep = rng.choice(N, size=k, replace=False)
            special = (patterns or {}).get(b, {}).get(k)
            if special and rng.uniform() < 0.5:
                keep = special[rng.integers(len(special))]
            for m in range(N):
                if m not in keep:
                    traj[rows[m], f] = np.nan


def tree_session(seed, F, parent, n_markers=None, sigma=0.0, shares=None, n_loose=1, rate=120.0):
    """Bodies hung on each other: parent[b] < b or -1 (a root, flying free); body b > 0 with a parent hangs on it by a ball joint (b
    odd) or a hinge (b even).  -> traj [R][F][3], bodies [(rows, template)], joints (planted, in the order of the child), truth
    {"R" [B][F][3][3], "t" [B][F][3]}."""
    rng = np.random.default_rng(seed)
    B = len(parent)
    tau = np.arange(F) / rate
    Rm, t, joints = np.zeros((B, F, 3, 3)), np.zeros((B, F, 3)), []
    for b in range(B):
        p = parent[b]
        if p < 0:
            Rm[b], t[b] = rg.rigid_motion(rng, tau, amplitude=0.6, spin=0.3)
            continue
        ca, cb = rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.1, 0.1, 3)
        R0 = rg.random_rotation(rng)
        if b % 2:
            Rm[b] = Rm[p] @ rg._rodrigues(jr.swing(rng, tau, 0.5)) @ R0
            joints.append({"a": p, "b": b, "kind": BALL, "c_a": ca, "c_b": cb, "axis_a": np.full(3, NAN), "axis_b": np.full(3, NAN)})
        else:
            u = jr.unit(rng)
            Rm[b] = Rm[p] @ jr.rot_axis(u, 0.5 * np.sin(2 * np.pi * rng.uniform(0.5, 1.5) * tau)) @ R0
            joints.append({"a": p, "b": b, "kind": HINGE, "c_a": ca, "c_b": cb, "axis_a": u, "axis_b": R0.T @ u})
        t[b] = np.einsum("fij,j->fi", Rm[p], ca) + t[p] - np.einsum("fij,j->fi", Rm[b], cb)
    templates = _templates(rng, n_markers if n_markers is not None else [3 + (b % 3) for b in range(B)])
    clean, bodies = _rows_of(templates, Rm, t, n_loose, rng, tau)
    traj = clean + sigma * rng.standard_normal(clean.shape)
    _hide(rng, traj, bodies, shares if shares is not None else {0: 0.04, 1: 0.08, 2: 0.12})
    return traj, bodies, joints, {"R": Rm, "t": t}


def five_body_session(seed, F=1500, sigma=0.0, outliers=0.02, shares=None):
    """joints_reference.five_body_scene's poses (0 - ball - 1 - hinge - 2; 3 rigid on 0; 4 free) with 5, 5, 5, 4 and 4 markers.  Body 1
    has three collinear markers (0, 1, 2), body 2 its marker 0 on the hinge axis.  The joints are the planted ball and hinge and a
    ball joint between 0 and 3 (two bodies rigid on each other share every point).  `outliers` of the samples of bodies 0 .. 3 are
    off by 3 cm, as a mislabelled blob would be.  -> t [F], traj, bodies, joints, truth {"R", "t", "outlier" [R][F] bool}."""
    _, Rm, t, tr = jr.five_body_scene(seed, F=F)
    rng = np.random.default_rng(seed + 1000)
    tau = np.arange(F) / 120.0
    templates = _templates(rng, [5, 5, 5, 4, 4])
    line = jr.unit(rng)
    for m, s in enumerate((-0.1, 0.02, 0.11)):
        templates[1][m] = np.array([0.0, 0.05, 0.03]) + s * line
    templates[2][0] = tr["hinge_p2"] + 0.07 * tr["hinge_u2"]
    assert all(rbr.posable_table(q)[-1] for q in templates) and not rbr.posable_table(templates[1])[0b00111]
    R03 = Rm[0, 0].T @ Rm[3, 0]
    d03 = Rm[0, 0].T @ (t[3, 0] - t[0, 0])
    p03 = np.array([0.03, -0.02, 0.04])
    joints = [{"a": 0, "b": 1, "kind": BALL, "c_a": tr["ball_a"], "c_b": tr["ball_b"], "axis_a": np.full(3, NAN), "axis_b": np.full(3, NAN)},
              {"a": 1, "b": 2, "kind": HINGE, "c_a": tr["hinge_p1"], "c_b": tr["hinge_p2"], "axis_a": tr["hinge_u1"], "axis_b": tr["hinge_u2"]},
              {"a": 0, "b": 3, "kind": BALL, "c_a": p03, "c_b": R03.T @ (p03 - d03), "axis_a": np.full(3, NAN), "axis_b": np.full(3, NAN)}]
    clean, bodies = _rows_of(templates, Rm, t, 1, rng, tau)
    traj = clean + sigma * rng.standard_normal(clean.shape)
    n_body_rows = sum(len(q) for q in templates[:4])
    outlier = np.zeros(traj.shape[:2], dtype=bool)
    outlier[:n_body_rows] = rng.uniform(size=(n_body_rows, F)) < outliers
    traj[outlier] += 0.03 * np.array([jr.unit(rng) for _ in range(int(outlier.sum()))]).reshape(-1, 3)
    _hide(rng, traj, bodies, shares if shares is not None else {0: 0.05, 1: 0.12, 2: 0.12, 3: 0.08},
          patterns={1: {3: [(0, 1, 2)]}, 2: {1: [(0,)]}})
    t_s = 2.0 + tau
    return t_s, traj, bodies, joints, {"R": Rm, "t": t, "outlier": outlier & np.isfinite(traj).all(axis=2)}
