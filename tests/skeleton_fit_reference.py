"""The "skeleton fit" contract of include/mocap_core.h in plain Python and NumPy, in the order the header writes.

    validate(B, joints, axis_len, w_joint, iters)     None, or the reason the core returns MOCAP_E_ARG for (the joints and the three
                                                      parameters; the bodies and the session are body_session_reference.validate's)
    forest(B, joints)                                 the host's tables: {"parent", "depth", "joint_up", "order", "child_of", "dirs"}
    fit_skeleton(traj, bodies, flag, quat, t_pose, joints, axis_len, w_joint, iters)
                                                      THE statement, lanes over frames -> {"quat", "R", "t_pose", "rms_s", "cost0",
                                                      "cost", "steps", "n_act"}; scalar=True: one frame at a time with every operation
                                                      in Python floats, asserted equal bit for bit in
                                                      tests/test_skeleton_fit_reference_cpu.py; the device is compared with the lanes
    terms(...), step(...)                             one linearisation and one solve of a frame, for the tests of the solve

ONE text serves both forms: every function below takes `ops`, the few operations that differ between an array of lanes and a
Python float (select, square root, division by what may be zero, finite).  Everything else is + - * and comparisons, which mean
the same on both.  The scenes are joint_pose_reference's (tree_session, five_body_session)."""
import math

import numpy as np

import body_session_reference as bsr
import joint_pose_reference as jp

POSED, JOINTED = jp.POSED, jp.JOINTED
HINGE, BALL = jp.HINGE, jp.BALL
MAX_ITERS = 16
NAN = float("nan")
INT_OUT = ("steps", "n_act")
F64_OUT = ("quat", "R", "t_pose", "rms_s", "cost0", "cost")

same_bits = bsr.same_bits


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in INT_OUT) and all(same_bits(np.asarray(a[k]).reshape(b[k].shape), b[k]) for k in F64_OUT)


class Lanes:
    sel = staticmethod(np.where)
    sqrt = staticmethod(np.sqrt)
    finite = staticmethod(np.isfinite)

    @staticmethod
    def div(a, b):
        return a / b

    @staticmethod
    def no(c):
        return ~c


class Scalar:
    finite = staticmethod(math.isfinite)

    @staticmethod
    def sel(c, a, b):
        return a if c else b

    @staticmethod
    def sqrt(x):
        return math.sqrt(x) if x >= 0.0 else NAN      # (NaN compares false: NaN in, NaN out; -0.0 >= 0.0)

    @staticmethod
    def div(a, b):
        if b != 0.0:
            return a / b
        if a != a or a == 0.0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)

    @staticmethod
    def no(c):
        return not c


# ---------------------------------------------------------------------------------------------------------------------- the host's part
def validate(B, joints, axis_len, w_joint, iters):
    if not 2 <= B <= 64:
        return "B"
    if not 1 <= len(joints) <= B - 1:
        return "J"
    if not (axis_len > 0.0 and math.isfinite(axis_len)):
        return "axis_len"
    if not (w_joint > 0.0 and math.isfinite(w_joint)):
        return "w_joint"
    if not 1 <= iters <= MAX_ITERS:
        return "iters"
    return jp.validate(B, joints, 0.1, 1.0, 1)      # the joints' own rules: "joint poses"' check


def forest(B, joints):
    """parent (-1 = root: a component's lowest body), depth, joint_up per body; order: by (depth descending, body ascending);
    child_of per joint; dirs[y] = the joints of y in ascending index as y sees them: (j, x, hinge, up, c_y, ax_y, c_x, ax_x)."""
    parent, depth, joint_up, child_of = [-1] * B, [0] * B, [-1] * B, [-1] * len(joints)
    seen = [False] * B
    for root in range(B):
        if seen[root]:
            continue
        seen[root], queue = True, [root]
        while queue:
            p = queue.pop(0)
            for j, jt in enumerate(joints):
                a, b = int(jt["a"]), int(jt["b"])
                c = b if a == p else a if b == p else -1
                if c < 0 or seen[c]:
                    continue
                seen[c], parent[c], depth[c], joint_up[c], child_of[j] = True, p, depth[p] + 1, j, c
                queue.append(c)
    order = sorted(range(B), key=lambda b: (-depth[b], b))
    dirs = []
    for y in range(B):
        mine = []
        for j, jt in enumerate(joints):
            if int(jt["a"]) == y:
                x, c_y, c_x, ax_y, ax_x = int(jt["b"]), jt["c_a"], jt["c_b"], jt.get("axis_a"), jt.get("axis_b")
            elif int(jt["b"]) == y:
                x, c_y, c_x, ax_y, ax_x = int(jt["a"]), jt["c_b"], jt["c_a"], jt.get("axis_b"), jt.get("axis_a")
            else:
                continue
            hinge = int(jt["kind"]) == HINGE
            vec = lambda v, on=True: [float(e) for e in v] if on else [0.0, 0.0, 0.0]
            mine.append((j, x, hinge, joint_up[y] == j, vec(c_y), vec(ax_y, hinge), vec(c_x), vec(ax_x, hinge)))
        dirs.append(mine)
    return {"parent": parent, "depth": depth, "joint_up": joint_up, "order": order, "child_of": child_of, "dirs": dirs}


# ---------------------------------------------------------------------------------------------------------------------- arithmetic
def tri(i, k):
    return i * (i + 1) // 2 + k


def _rot(R, p):
    return [(R[3 * i] * p[0] + R[3 * i + 1] * p[1]) + R[3 * i + 2] * p[2] for i in range(3)]


def _sq(r):
    return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]


def _own_add(ops, o, on, y, r, w):
    """o = [S (6), m (3), s, g (6)] as one list of 16; the point's terms added where `on`."""
    new = [o[0] + w * (y[1] * y[1] + y[2] * y[2]), o[1] - w * (y[0] * y[1]), o[2] - w * (y[0] * y[2]),
           o[3] + w * (y[0] * y[0] + y[2] * y[2]), o[4] - w * (y[1] * y[2]), o[5] + w * (y[0] * y[0] + y[1] * y[1]),
           o[6] + w * y[0], o[7] + w * y[1], o[8] + w * y[2], o[9] + w,
           o[10] + w * (y[1] * r[2] - y[2] * r[1]), o[11] + w * (y[2] * r[0] - y[0] * r[2]), o[12] + w * (y[0] * r[1] - y[1] * r[0]),
           o[13] + w * r[0], o[14] + w * r[1], o[15] + w * r[2]]
    return [ops.sel(on, n, c) for n, c in zip(new, o)]


def _own_block(o, lam, zero):
    S, m, s = o[0:6], o[6:9], o[9]
    tt = s + lam * s
    return [S[0] + lam * S[0], S[1], S[3] + lam * S[3], S[2], S[4], S[5] + lam * S[5], zero, m[2], -m[1], tt, -m[2], zero, m[0], zero, tt,
            m[1], -m[0], zero, zero, zero, tt]


def _up_point(yc, yp):
    dot = (yc[0] * yp[0] + yc[1] * yp[1]) + yc[2] * yp[2]
    return [dot - yp[i] * yc[k] if i == k else -(yp[i] * yc[k]) for i in range(3) for k in range(3)]


def _up_block(yc0, yp0, yc1, yp1, hinge, w, zero):
    """The coupling C [child's rows][parent's columns] as a 6 x 6 list."""
    E0 = _up_point(yc0, yp0)
    E1 = _up_point(yc1, yp1) if hinge else None
    G = [-(w * (E0[e] + E1[e] if hinge else E0[e])) for e in range(9)]
    u = [w * (yc0[i] + yc1[i] if hinge else yc0[i]) for i in range(3)]
    v = [w * (yp0[i] + yp1[i] if hinge else yp0[i]) for i in range(3)]
    n = w * (2.0 if hinge else 1.0)
    C = [[zero] * 6 for _ in range(6)]
    for i in range(3):
        for k in range(3):
            C[i][k] = G[3 * i + k]
        C[3 + i][3 + i] = -n + zero
    C[0][4], C[0][5], C[1][3], C[1][5], C[2][3], C[2][4] = u[2], -u[1], -u[2], u[0], u[1], -u[0]
    C[3][1], C[3][2], C[4][0], C[4][2], C[5][0], C[5][1] = -v[2], v[1], v[2], -v[0], -v[1], v[0]
    return C


def _ldl6(ops, A):
    L, T, d, ok = {}, {}, [], True
    for i in range(6):
        di = A[tri(i, i)]
        for k in range(i):
            t = A[tri(i, k)]
            for m in range(k):
                t = t - L[i, m] * T[k, m]
            T[i, k] = t
            L[i, k] = ops.div(t, d[k])
            di = di - L[i, k] * t
        d.append(di)
        ok = ok & (ops.finite(di) & (di > 0.0))
    return L, d, ok


def _solve6(ops, L, d, b):
    u = []
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i, k] * u[k]
        u.append(s)
    x = [None] * 6
    for i in range(5, -1, -1):
        s = ops.div(u[i], d[i])
        for k in range(i + 1, 6):
            s = s - L[k, i] * x[k]
        x[i] = s
    return x


def _update(ops, q, t, delta):
    hx, hy, hz = delta[0] * 0.5, delta[1] * 0.5, delta[2] * 0.5
    nd = ops.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
    dw, dx, dy, dz = ops.div(1.0, nd), ops.div(hx, nd), ops.div(hy, nd), ops.div(hz, nd)
    w = ((dw * q[0] - dx * q[1]) - dy * q[2]) - dz * q[3]
    x = ((dw * q[1] + dx * q[0]) + dy * q[3]) - dz * q[2]
    y = ((dw * q[2] - dx * q[3]) + dy * q[0]) + dz * q[1]
    z = ((dw * q[3] + dx * q[2]) - dy * q[1]) + dz * q[0]
    nq = ops.sqrt(((w * w + x * x) + y * y) + z * z)
    return [ops.div(w, nq), ops.div(x, nq), ops.div(y, nq), ops.div(z, nq)], [t[0] + delta[3], t[1] + delta[4], t[2] + delta[5]]


# ---------------------------------------------------------------------------------------------------------------------- a frame
class Frame:
    """What a frame (or an array of them) is given: Q[b] the markers as Python floats, P[b][m] = [x, y, z], pres[b][m], act[b],
    and the tables.  zero: 0.0 as a lane value."""

    def __init__(self, ops, Q, P, pres, act, tables, joints, axis_len, w_joint, zero):
        self.ops, self.Q, self.P, self.pres, self.act, self.tb, self.zero = ops, Q, P, pres, act, tables, zero
        self.B, self.J, self.len, self.w = len(Q), len(joints), float(axis_len), float(w_joint)
        self.jact = [act[tables["child_of"][j]] & act[tables["parent"][tables["child_of"][j]]] for j in range(self.J)]


def terms(fr, q, t, lam=None):
    """-> body shares [B], joint shares [J], and with lam the blocks H [B] (21), gradients g [B] (6) and couplings C [B] (6 x 6 or
    None).  Whatever belongs to an inactive body or joint is not to be read."""
    ops, zero = fr.ops, fr.zero
    R = [bsr.quat_to_R(*q[b]) for b in range(fr.B)]
    share_b, share_j, H, g, C = [], [None] * fr.J, [], [], [None] * fr.B
    for b in range(fr.B):
        o = [zero] * 16
        cb = zero
        for m in range(len(fr.Q[b])):
            y = _rot(R[b], fr.Q[b][m])
            r = [(y[i] + t[b][i]) - fr.P[b][m][i] for i in range(3)]
            cb = ops.sel(fr.pres[b][m], cb + _sq(r), cb)
            if lam is not None:
                o = _own_add(ops, o, fr.pres[b][m], y, r, 1.0)
        for (j, x, hinge, up, c_y, ax_y, c_x, ax_x) in fr.tb["dirs"][b]:
            on = fr.act[b] & fr.act[x]
            yb, yx, ub, ux = _rot(R[b], c_y), _rot(R[x], c_x), _rot(R[b], ax_y), _rot(R[x], ax_x)
            wy, wx = [yb[i] + t[b][i] for i in range(3)], [yx[i] + t[x][i] for i in range(3)]
            r0 = [wy[i] - wx[i] for i in range(3)]
            y1b, y1x = [yb[i] + fr.len * ub[i] for i in range(3)], [yx[i] + fr.len * ux[i] for i in range(3)]
            r1 = [(wy[i] + fr.len * ub[i]) - (wx[i] + fr.len * ux[i]) for i in range(3)]
            if lam is not None:
                o = _own_add(ops, o, on, yb, r0, fr.w)
                if hinge:
                    o = _own_add(ops, o, on, y1b, r1, fr.w)
            if up:
                share_j[j] = fr.w * _sq(r0) + fr.w * _sq(r1) if hinge else fr.w * _sq(r0)
                if lam is not None:
                    C[b] = _up_block(yb, yx, y1b, y1x, hinge, fr.w, zero)
        share_b.append(cb)
        if lam is not None:
            H.append(_own_block(o, lam, zero))
            g.append(o[10:16])
    return share_b, share_j, H, g, C


def cost_of(fr, share_b, share_j):
    c = fr.zero
    for b in range(fr.B):
        c = fr.ops.sel(fr.act[b], c + share_b[b], c)
    for j in range(fr.J):
        c = fr.ops.sel(fr.jact[j], c + share_j[j], c)
    return c


def step(fr, H, g, C):
    """The tree elimination -> delta [B] (6 each; an inactive body's is not to be read), every active body's pivots good."""
    ops, tb = fr.ops, fr.tb
    H, g = [list(h) for h in H], [list(v) for v in g]
    z, W, piv = [None] * fr.B, [None] * fr.B, True
    for i in tb["order"]:
        p = tb["parent"][i]
        L, d, ok = _ldl6(ops, H[i])
        piv = piv & (ok | ops.no(fr.act[i]))
        z[i] = _solve6(ops, L, d, g[i])
        if p < 0:
            continue
        up = fr.act[i] & fr.act[p]
        Ci = C[i]
        W[i] = [[None] * 6 for _ in range(6)]
        for col in range(6):
            wc = _solve6(ops, L, d, [Ci[e][col] for e in range(6)])
            for e in range(6):
                W[i][e][col] = wc[e]
            for r in range(col, 6):
                s = Ci[0][r] * wc[0]
                for e in range(1, 6):
                    s = s + Ci[e][r] * wc[e]
                H[p][tri(r, col)] = ops.sel(up, H[p][tri(r, col)] - s, H[p][tri(r, col)])
        for r in range(6):
            s = Ci[0][r] * z[i][0]
            for e in range(1, 6):
                s = s + Ci[e][r] * z[i][e]
            g[p][r] = ops.sel(up, g[p][r] - s, g[p][r])
    delta = [None] * fr.B
    for i in reversed(tb["order"]):
        p = tb["parent"][i]
        if p < 0:
            delta[i] = [-z[i][e] for e in range(6)]
            continue
        up = fr.act[i] & fr.act[p]
        delta[i] = []
        for e in range(6):
            s = W[i][e][0] * delta[p][0]
            for m in range(1, 6):
                s = s + W[i][e][m] * delta[p][m]
            delta[i].append(ops.sel(up, -(z[i][e] + s), -z[i][e]))
    return delta, piv


def fit_frame(fr, q, t, iters, lam0=1e-3):
    """-> q, t, rms per body, cost0, cost, steps"""
    ops = fr.ops
    lam, steps = lam0 + fr.zero, 0
    cost0 = None
    for it in range(iters):
        sb, sj, H, g, C = terms(fr, q, t, lam)
        cur = cost_of(fr, sb, sj)
        if it == 0:
            cost0 = cur
        delta, piv = step(fr, H, g, C)
        trial = [_update(ops, q[b], t[b], delta[b]) for b in range(fr.B)]
        tq, tt = [p[0] for p in trial], [p[1] for p in trial]
        tb_, tj_, _, _, _ = terms(fr, tq, tt)
        tc = cost_of(fr, tb_, tj_)
        take = piv & ops.finite(cost0) & ops.finite(tc) & (tc < cur)
        for b in range(fr.B):
            q[b] = [ops.sel(take & fr.act[b], tq[b][i], q[b][i]) for i in range(4)]
            t[b] = [ops.sel(take & fr.act[b], tt[b][i], t[b][i]) for i in range(3)]
        cost = ops.sel(take, tc, cur)
        lam = ops.sel(take, ops.div(lam, 10.0), lam * 10.0)
        steps = steps + ops.sel(take, 1, 0)
    sb, _, _, _, _ = terms(fr, q, t)
    rms = []
    for b in range(fr.B):
        k = fr.zero
        for m in range(len(fr.Q[b])):
            k = k + ops.sel(fr.pres[b][m], 1.0, 0.0)
        rms.append(ops.sel(fr.act[b] & (k > 0.0), ops.sqrt(ops.div(sb[b], k)), NAN))
    return q, t, rms, cost0, cost, steps


# ---------------------------------------------------------------------------------------------------------------------- THE statement
def prepare(traj, bodies, flag, quat, t_pose):
    traj = np.asarray(traj, dtype=np.float64)
    _, F, _ = traj.shape
    B = len(bodies)
    flag = np.asarray(flag, dtype=np.int32).reshape(B, F)
    quat = np.asarray(quat, dtype=np.float64).reshape(B, F, 4)
    t_pose = np.asarray(t_pose, dtype=np.float64).reshape(B, F, 3)
    act = ((flag == POSED) | (flag == JOINTED)) & np.isfinite(quat).all(axis=2) & np.isfinite(t_pose).all(axis=2)
    Q = [[[float(v) for v in row] for row in np.asarray(markers, dtype=np.float64).reshape(-1, 3)] for _, markers in bodies]
    P = [traj[np.asarray(rows, dtype=np.int64)] for rows, _ in bodies]      # [N][F][3]
    pres = [np.isfinite(p).all(axis=2) for p in P]
    return F, B, flag, quat, t_pose, act, Q, P, pres


def frames_of(traj, bodies, flag, quat, t_pose, joints, axis_len, w_joint, scalar=False):
    """The Frame of all lanes, or with scalar one Frame per frame, each with its start pose (q, t)."""
    F, B, flag, quat, t_pose, act, Q, P, pres = prepare(traj, bodies, flag, quat, t_pose)
    tables = forest(B, joints)
    if not scalar:
        fr = Frame(Lanes, Q, [[[p[m][:, i] for i in range(3)] for m in range(len(p))] for p in P], pres, list(act), tables, joints,
                   axis_len, w_joint, np.zeros(F))
        return [(fr, [[quat[b][:, i] for i in range(4)] for b in range(B)], [[t_pose[b][:, i] for i in range(3)] for b in range(B)])]
    out = []
    for f in range(F):
        fr = Frame(Scalar, Q, [[[float(p[m][f, i]) for i in range(3)] for m in range(len(p))] for p in P],
                   [[bool(pr[m][f]) for m in range(len(pr))] for pr in pres], [bool(act[b][f]) for b in range(B)], tables, joints, axis_len,
                   w_joint, 0.0)
        out.append((fr, [[float(v) for v in quat[b][f]] for b in range(B)], [[float(v) for v in t_pose[b][f]] for b in range(B)]))
    return out


def fit_skeleton(traj, bodies, flag, quat, t_pose, joints, axis_len=0.1, w_joint=1.0, iters=8, scalar=False):
    F, B, flag, quat, t_pose, act, _, _, _ = prepare(traj, bodies, flag, quat, t_pose)
    out = {"quat": np.full((B, F, 4), NAN), "R": np.full((B, F, 9), NAN), "t_pose": np.full((B, F, 3), NAN), "rms_s": np.full((B, F), NAN),
           "cost0": np.zeros(F), "cost": np.zeros(F), "steps": np.zeros(F, dtype=np.int32), "n_act": np.zeros(F, dtype=np.int32)}
    with np.errstate(all="ignore"):
        for n, (fr, q, t) in enumerate(frames_of(traj, bodies, flag, quat, t_pose, joints, axis_len, w_joint, scalar)):
            at = n if scalar else slice(None)
            q, t, rms, cost0, cost, steps = fit_frame(fr, q, t, int(iters))
            for b in range(B):
                R = bsr.quat_to_R(*q[b])
                on = fr.act[b]
                for i in range(4):
                    out["quat"][b, at, i] = fr.ops.sel(on, q[b][i], NAN)
                for i in range(9):
                    out["R"][b, at, i] = fr.ops.sel(on, R[i], NAN)
                for i in range(3):
                    out["t_pose"][b, at, i] = fr.ops.sel(on, t[b][i], NAN)
                out["rms_s"][b, at] = rms[b]
            out["cost0"][at], out["cost"][at], out["steps"][at] = cost0, cost, steps
            out["n_act"][at] = sum(fr.ops.sel(a, 1, 0) for a in fr.jact)
    carries = (flag == POSED) | (flag == JOINTED)
    for b in range(B):
        s = bsr.sign_walk(out["quat"][b], carries[b])
        out["quat"][b] = np.where(s[:, None] == 1, -out["quat"][b], out["quat"][b])
    out["R"] = out["R"].reshape(B, F, 3, 3)
    return out


# ---------------------------------------------------------------------------------------------------------------------- dense (tests)
def dense_system(fr, H, g, C):
    """One scalar frame's assembled system over its active bodies -> A [6 A][6 A], rhs [6 A], the bodies in ascending order."""
    ids = [b for b in range(fr.B) if fr.act[b]]
    at = {b: n for n, b in enumerate(ids)}
    A, rhs = np.zeros((6 * len(ids), 6 * len(ids))), np.zeros(6 * len(ids))
    for b in ids:
        n = at[b]
        for i in range(6):
            rhs[6 * n + i] = g[b][i]
            for k in range(i + 1):
                A[6 * n + i, 6 * n + k] = A[6 * n + k, 6 * n + i] = H[b][tri(i, k)]
        p = fr.tb["parent"][b]
        if p >= 0 and fr.act[p]:
            blk = np.array(C[b], dtype=np.float64)
            A[6 * n:6 * n + 6, 6 * at[p]:6 * at[p] + 6] = blk
            A[6 * at[p]:6 * at[p] + 6, 6 * n:6 * n + 6] = blk.T
    return ids, A, rhs
