"""The "joints" contract of include/mocap_core.h in plain Python and NumPy, in the order the header writes.

    pair_sums(flag, Rm, t)                   the sixteen SUMs and the count of every pair, lanes over frames, the tree of "rigid groups"
                                             (tests/rigid_groups_reference.py: tree_sum, the header's words as loops and as reshapes)
    jacobi6_scalar(M)                        THE 6 x 6 cyclic Jacobi in Python floats, written as the header words it
    jacobi6(M)                               the same over a stack of matrices; asserted equal to the scalar form bit for bit in
                                             tests/test_joints_reference_cpu.py; the device is compared with this one
    find_joints(flag, Rm, t, ...)            THE statement of stage A: sums, system, kind, solution, axis, residual, Kruskal
    kruskal(accepted, sep)                   the skeleton alone
    joint_series(flag, quat, Rm, t, joints)  THE statement of stage B
    fit_mp(flag, Rm, t, a, b, tol_rank)      the fit of one pair with 50 digits (mpmath), for the accuracy figures
    five_body_scene, session                 poses: the planted ball - hinge - fixed - free scene; chains of joints for the shapes
"""
import math

import numpy as np

import rigid_groups_reference as rg

INF = float("inf")
NAN = float("nan")
POSED, FEW = 1, 2
UNSEEN, SINGULAR, FIXED, HINGE, BALL = 0, 1, 2, 3, 4
SWEEPS = 30
INT_OUT = ("cnt", "kind", "accepted", "parent")
F64_OUT = ("lam", "sep", "centre", "axis")
SERIES_F64 = ("centre", "gap", "quat_rel", "twist")
PAIRS = [(p, q) for p in range(5) for q in range(p + 1, 6)]

same_bits = rg.same_bits


def same(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in INT_OUT) and int(a["n_joints"]) == int(b["n_joints"])
            and all(same_bits(a[k], b[k]) for k in F64_OUT))


# ---------------------------------------------------------------------------------------------------------------------- pair sums
def usable(flag, Rm, t):
    """[B][F]: the flag is POSED and the twelve values are finite."""
    B, F = flag.shape
    return (flag == POSED) & np.isfinite(Rm.reshape(B, F, 9)).all(axis=2) & np.isfinite(t).all(axis=2)


def pair_values(Ra, ta, Rb, tb):
    """The sixteen values per frame of one pair: Ra, Rb [F][3][3], ta, tb [F][3] -> [16][F]."""
    rel = [(Ra[:, 0, i] * Rb[:, 0, j] + Ra[:, 1, i] * Rb[:, 1, j]) + Ra[:, 2, i] * Rb[:, 2, j] for i in range(3) for j in range(3)]
    dt = [tb[:, k] - ta[:, k] for k in range(3)]
    d = [(Ra[:, 0, i] * dt[0] + Ra[:, 1, i] * dt[1]) + Ra[:, 2, i] * dt[2] for i in range(3)]
    g = [(rel[j] * d[0] + rel[3 + j] * d[1]) + rel[6 + j] * d[2] for j in range(3)]
    dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return np.array(rel + d + g + [dd])


def pair_sums(flag, Rm, t):
    """-> cnt [B][B] int32 (the diagonal included), sums [B][B][16] (a < b; elsewhere 0)."""
    flag = np.asarray(flag)
    B, F = flag.shape
    Rm = np.asarray(Rm, dtype=np.float64).reshape(B, F, 3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(B, F, 3)
    ok = usable(flag, Rm, t)
    cnt = np.zeros((B, B), dtype=np.int32)
    sums = np.zeros((B, B, 16))
    with np.errstate(all="ignore"):
        for a in range(B):
            cnt[a, a] = ok[a].sum()
            for b in range(a + 1, B):
                both = ok[a] & ok[b]
                cnt[a, b] = cnt[b, a] = both.sum()
                sums[a, b] = rg.tree_sum(np.where(both[None, :], pair_values(Rm[a], t[a], Rm[b], t[b]), 0.0))
    return cnt, sums


# ---------------------------------------------------------------------------------------------------------------------- the 6 x 6 Jacobi
def jacobi6_scalar(M):
    """M: 6 x 6 nested list of Python floats, symmetric -> (diagonal [6], V [6][6], sweeps that did work)."""
    A = [[float(M[i][j]) for j in range(6)] for i in range(6)]
    V = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
    used = 0
    for sweep in range(SWEEPS):
        off = None
        for p, q in PAIRS:
            off = abs(A[p][q]) if off is None else off + abs(A[p][q])
        if off == 0.0:
            break
        used += 1
        for p, q in PAIRS:
            apq = A[p][q]
            if apq == 0.0:
                continue
            g = 100.0 * abs(apq)
            if sweep > 3 and abs(A[p][p]) + g == abs(A[p][p]) and abs(A[q][q]) + g == abs(A[q][q]):
                A[p][q] = A[q][p] = 0.0
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            t = -t if theta < 0.0 else t
            cs = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * cs
            A[p][p] = A[p][p] - t * apq
            A[q][q] = A[q][q] + t * apq
            A[p][q] = A[q][p] = 0.0
            for k in range(6):
                if k != p and k != q:
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = A[p][k] = cs * akp - sn * akq
                    A[k][q] = A[q][k] = sn * akp + cs * akq
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = cs * vkp - sn * vkq
                V[k][q] = sn * vkp + cs * vkq
    return [A[k][k] for k in range(6)], V, used


def jacobi6(M):
    """The same over M [N][6][6] -> (diagonal [N][6], V [N][6][6], sweeps [N])."""
    A = np.array(M, dtype=np.float64)
    N = A.shape[0]
    V = np.broadcast_to(np.eye(6), (N, 6, 6)).copy()
    used = np.zeros(N, dtype=np.int32)
    with np.errstate(all="ignore"):
        for sweep in range(SWEEPS):
            off = None
            for p, q in PAIRS:
                off = np.abs(A[:, p, q]) if off is None else off + np.abs(A[:, p, q])
            active = ~(off == 0.0)
            if not active.any():
                break
            used += active
            for p, q in PAIRS:
                apq = A[:, p, q].copy()
                app, aqq = A[:, p, p].copy(), A[:, q, q].copy()
                act = active & ~(apq == 0.0)
                g = 100.0 * np.abs(apq)
                small = act & (sweep > 3) & (np.abs(app) + g == np.abs(app)) & (np.abs(aqq) + g == np.abs(aqq))
                rot = act & ~small
                theta = (aqq - app) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                cs = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * cs
                A[:, p, p] = np.where(rot, app - t * apq, app)
                A[:, q, q] = np.where(rot, aqq + t * apq, aqq)
                A[:, p, q] = A[:, q, p] = np.where(act, 0.0, apq)
                for k in range(6):
                    if k != p and k != q:
                        akp, akq = A[:, k, p].copy(), A[:, k, q].copy()
                        A[:, k, p] = A[:, p, k] = np.where(rot, cs * akp - sn * akq, akp)
                        A[:, k, q] = A[:, q, k] = np.where(rot, sn * akp + cs * akq, akq)
                    vkp, vkq = V[:, k, p].copy(), V[:, k, q].copy()
                    V[:, k, p] = np.where(rot, cs * vkp - sn * vkq, vkp)
                    V[:, k, q] = np.where(rot, sn * vkp + cs * vkq, vkq)
    return A[:, np.arange(6), np.arange(6)], V, used


# ---------------------------------------------------------------------------------------------------------------------- the fit
def system_of(sums, n):
    """sums [16], n -> (M 6 x 6, rhs [6]) as float64 arrays."""
    with np.errstate(all="ignore"):
        m = np.asarray(sums, dtype=np.float64) / np.float64(n)
    M = np.eye(6)
    M[:3, 3:] = -m[:9].reshape(3, 3)
    M[3:, :3] = -m[:9].reshape(3, 3).T
    return M, np.concatenate([m[9:12], -m[12:15]])


def solve_pair(lam, V, rhs, tol_rank):
    """The diagonal, V and rhs of one pair (Python floats) -> (kind, lam3, c_a, c_b, axis_a, axis_b), NaN where the header says so."""
    nan3 = [NAN] * 3
    if not all(math.isfinite(x) for x in lam) or not all(math.isfinite(x) for row in V for x in row):
        return SINGULAR, nan3, nan3, nan3, nan3, nan3
    order = sorted(range(6), key=lambda k: (lam[k], k))
    small = sum(1 for x in lam if x <= tol_rank)
    kind = FIXED if small >= 2 else HINGE if small == 1 else BALL
    x = [0.0] * 6
    for k in order:
        if lam[k] > tol_rank:
            h = 0.0
            for i in range(6):
                h = h + V[i][k] * rhs[i]
            h = h / lam[k]
            for i in range(6):
                x[i] = x[i] + h * V[i][k]
    xa, xb = nan3, nan3
    if kind == HINGE:
        v = [V[i][order[0]] for i in range(6)]
        na = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        nb = math.sqrt((v[3] * v[3] + v[4] * v[4]) + v[5] * v[5])
        if not na > 0.0 or not nb > 0.0:
            return SINGULAR, nan3, nan3, nan3, nan3, nan3
        xa, xb = [c / na for c in v[:3]], [c / nb for c in v[3:]]
        lead = xa[0] if xa[0] != 0.0 else xa[1] if xa[1] != 0.0 else xa[2]
        if lead < 0.0:
            xa, xb = [-c for c in xa], [-c for c in xb]
    return kind, [lam[k] for k in order[:3]], x[:3], x[3:], xa, xb


def kruskal(accepted, sep):
    """accepted [B][B], sep [B][B] -> (parent [B] int32, n_joints)."""
    B = accepted.shape[0]
    edges = sorted((int(np.float64(sep[a, b]).view(np.uint64)), a, b) for a in range(B) for b in range(a + 1, B) if accepted[a, b])
    top = list(range(B))

    def find(r):
        while top[r] != r:
            r = top[r]
        return r

    tree = [[] for _ in range(B)]
    n = 0
    for _, a, b in edges:
        x, y = find(a), find(b)
        if x != y:
            top[max(x, y)] = min(x, y)
            tree[a].append(b)
            tree[b].append(a)
            n += 1
    parent = np.full(B, -1, dtype=np.int32)
    seen = [False] * B
    for r in range(B):                                          # ascending: the first body met of a component is its lowest
        if not seen[r]:
            seen[r] = True
            todo = [r]
            while todo:
                u = todo.pop()
                for v in tree[u]:
                    if not seen[v]:
                        seen[v] = True
                        parent[v] = u
                        todo.append(v)
    return parent, n


def residual_values(Ra, ta, Rb, tb, ca, cb):
    """e.e per frame: Ra, Rb [F][3][3], ta, tb [F][3], ca, cb [3] -> [F]."""
    e = []
    for i in range(3):
        wa = ((Ra[:, i, 0] * ca[0] + Ra[:, i, 1] * ca[1]) + Ra[:, i, 2] * ca[2]) + ta[:, i]
        wb = ((Rb[:, i, 0] * cb[0] + Rb[:, i, 1] * cb[1]) + Rb[:, i, 2] * cb[2]) + tb[:, i]
        e.append(wa - wb)
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def find_joints(flag, Rm, t, min_common=30, tol_rank=1e-4, max_sep=INF, scalar=False, stats=None):
    """THE statement of mocap_find_joints.  scalar: the Jacobi in Python floats per pair, not stacked.  stats: a dict that receives
    "sweeps", the most sweeps any pair needed."""
    flag = np.asarray(flag)
    B, F = flag.shape
    Rm = np.asarray(Rm, dtype=np.float64).reshape(B, F, 3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(B, F, 3)
    ok = usable(flag, Rm, t)
    cnt, sums = pair_sums(flag, Rm, t)
    out = {"cnt": cnt, "kind": np.full((B, B), UNSEEN, dtype=np.int32), "accepted": np.zeros((B, B), dtype=np.int32),
           "lam": np.full((B, B, 3), NAN), "sep": np.full((B, B), NAN), "centre": np.full((B, B, 3), NAN), "axis": np.full((B, B, 3), NAN)}
    todo = [(a, b) for a in range(B) for b in range(a + 1, B) if cnt[a, b] >= min_common]
    systems = [system_of(sums[a, b], cnt[a, b]) for a, b in todo]
    if todo and not scalar:
        lam_all, V_all, used = jacobi6(np.array([s[0] for s in systems]))
    sweeps = 0
    with np.errstate(all="ignore"):
        for i, (a, b) in enumerate(todo):
            M, rhs = systems[i]
            if scalar:
                lam, V, n_sw = jacobi6_scalar(M.tolist())
            else:
                lam, V, n_sw = lam_all[i].tolist(), V_all[i].tolist(), int(used[i])
            sweeps = max(sweeps, n_sw)
            kind, lam3, ca, cb, xa, xb = solve_pair(lam, V, rhs.tolist(), tol_rank)
            out["kind"][a, b] = out["kind"][b, a] = kind
            out["lam"][a, b] = out["lam"][b, a] = lam3
            out["centre"][a, b], out["centre"][b, a] = ca, cb
            out["axis"][a, b], out["axis"][b, a] = xa, xb
            if kind >= FIXED:
                both = ok[a] & ok[b]
                ee = residual_values(Rm[a], t[a], Rm[b], t[b], ca, cb)
                sep = np.sqrt(rg.tree_sum(np.where(both, ee, 0.0)) / np.float64(cnt[a, b]))
                out["sep"][a, b] = out["sep"][b, a] = sep
                out["accepted"][a, b] = out["accepted"][b, a] = int(kind in (HINGE, BALL) and bool(sep <= max_sep))
    out["parent"], out["n_joints"] = kruskal(out["accepted"], out["sep"])
    if stats is not None:
        stats["sweeps"] = sweeps
    return out


# ---------------------------------------------------------------------------------------------------------------------- the series
def hamilton(p, q):
    return [((p[0] * q[0] - p[1] * q[1]) - p[2] * q[2]) - p[3] * q[3], ((p[0] * q[1] + p[1] * q[0]) + p[2] * q[3]) - p[3] * q[2],
            ((p[0] * q[2] - p[1] * q[3]) + p[2] * q[0]) + p[3] * q[1], ((p[0] * q[3] + p[1] * q[2]) - p[2] * q[1]) + p[3] * q[0]]


def joint_series(flag, quat, Rm, t, joints):
    """THE statement of mocap_joint_series.  joints: [{"a", "b", "kind", "c_a", "c_b", "axis_b", "q_ref"}]
    -> {"present" [J][F] int32, "centre" [J][F][3], "gap" [J][F], "quat_rel" [J][F][4], "twist" [J][F][2]}."""
    flag = np.asarray(flag)
    B, F = flag.shape
    Rm = np.asarray(Rm, dtype=np.float64).reshape(B, F, 3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(B, F, 3)
    quat = np.asarray(quat, dtype=np.float64).reshape(B, F, 4)
    J = len(joints)
    out = {"present": np.zeros((J, F), dtype=np.int32), "centre": np.full((J, F, 3), NAN), "gap": np.full((J, F), NAN),
           "quat_rel": np.full((J, F, 4), NAN), "twist": np.full((J, F, 2), NAN)}
    with np.errstate(all="ignore"):
        for j, jt in enumerate(joints):
            a, b = int(jt["a"]), int(jt["b"])
            ca, cb, ax, qr = (np.asarray(jt[k], dtype=np.float64) for k in ("c_a", "c_b", "axis_b", "q_ref"))
            pres = (flag[a] == POSED) & (flag[b] == POSED)
            e, c = [], []
            for i in range(3):
                wa = ((Rm[a][:, i, 0] * ca[0] + Rm[a][:, i, 1] * ca[1]) + Rm[a][:, i, 2] * ca[2]) + t[a][:, i]
                wb = ((Rm[b][:, i, 0] * cb[0] + Rm[b][:, i, 1] * cb[1]) + Rm[b][:, i, 2] * cb[2]) + t[b][:, i]
                c.append((wa + wb) * 0.5)
                e.append(wa - wb)
            gap = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            qa, qb = quat[a], quat[b]
            ab = hamilton([qa[:, 0], -qa[:, 1], -qa[:, 2], -qa[:, 3]], [qb[:, k] for k in range(4)])
            rel = hamilton([qr[0], -qr[1], -qr[2], -qr[3]], ab)
            tw = [np.full(F, NAN), np.full(F, NAN)]
            if int(jt["kind"]) == HINGE:
                s = (rel[1] * ax[0] + rel[2] * ax[1]) + rel[3] * ax[2]
                m = np.sqrt(rel[0] * rel[0] + s * s)
                good = m > 0.0
                tw = [np.where(good, rel[0] / m, NAN), np.where(good, s / m, NAN)]
            out["present"][j] = pres
            out["centre"][j] = np.where(pres[:, None], np.stack(c, axis=1), NAN)
            out["gap"][j] = np.where(pres, gap, NAN)
            out["quat_rel"][j] = np.where(pres[:, None], np.stack(rel, axis=1), NAN)
            out["twist"][j] = np.where(pres[:, None], np.stack(tw, axis=1), NAN)
    return out


def joint_arrays(joints):
    """The joints of a call as the C entry point takes them."""
    J = len(joints)
    return (np.array([j["a"] for j in joints], dtype=np.int32), np.array([j["b"] for j in joints], dtype=np.int32),
            np.array([j["kind"] for j in joints], dtype=np.int32), np.array([j["c_a"] for j in joints], dtype=np.float64).reshape(J, 3),
            np.array([j["c_b"] for j in joints], dtype=np.float64).reshape(J, 3),
            np.array([j["axis_b"] for j in joints], dtype=np.float64).reshape(J, 3),
            np.array([j["q_ref"] for j in joints], dtype=np.float64).reshape(J, 4))


# ---------------------------------------------------------------------------------------------------------------------- 50 digits
def fit_mp(flag, Rm, t, a, b, tol_rank, digits=50):
    """The fit of the pair (a, b) from exact sums of the float64 inputs -> {"lam" [3], "c_a", "c_b" [3], "sep"} as floats."""
    import mpmath as mp
    flag = np.asarray(flag)
    B, F = flag.shape
    Rm = np.asarray(Rm, dtype=np.float64).reshape(B, F, 3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(B, F, 3)
    both = usable(flag, Rm, t)
    frames = np.flatnonzero(both[a] & both[b])
    with mp.workdps(digits):
        n = len(frames)
        Ra = [mp.matrix(Rm[a, f].tolist()) for f in frames]
        Rb = [mp.matrix(Rm[b, f].tolist()) for f in frames]
        ta = [mp.matrix(t[a, f].tolist()) for f in frames]
        tb = [mp.matrix(t[b, f].tolist()) for f in frames]
        Rbar, dbar, gbar = mp.zeros(3, 3), mp.zeros(3, 1), mp.zeros(3, 1)
        for k in range(n):
            rel = Ra[k].T * Rb[k]
            d = Ra[k].T * (tb[k] - ta[k])
            Rbar += rel
            dbar += d
            gbar += rel.T * d
        Rbar, dbar, gbar = Rbar / n, dbar / n, gbar / n
        M = mp.eye(6)
        for i in range(3):
            for j in range(3):
                M[i, 3 + j] = -Rbar[i, j]
                M[3 + j, i] = -Rbar[i, j]
        rhs = mp.matrix([dbar[0], dbar[1], dbar[2], -gbar[0], -gbar[1], -gbar[2]])
        E, Q = mp.eigsy(M)
        order = sorted(range(6), key=lambda k: E[k])
        x = mp.zeros(6, 1)
        for k in order:
            if E[k] > tol_rank:
                h = sum(Q[i, k] * rhs[i] for i in range(6)) / E[k]
                for i in range(6):
                    x[i] += h * Q[i, k]
        ss = mp.mpf(0)
        for k in range(n):
            e = (Ra[k] * x[0:3, 0] + ta[k]) - (Rb[k] * x[3:6, 0] + tb[k])
            ss += e[0] ** 2 + e[1] ** 2 + e[2] ** 2
        return {"lam": [float(E[k]) for k in order[:3]], "c_a": [float(x[i]) for i in range(3)], "c_b": [float(x[3 + i]) for i in range(3)],
                "sep": float(mp.sqrt(ss / n))}


# ---------------------------------------------------------------------------------------------------------------------- poses
def rot_axis(u, th):
    """Rotations by the angles th [F] about the unit axis u -> [F][3][3]."""
    return rg._rodrigues(np.asarray(th)[:, None] * np.asarray(u)[None, :])


def swing(rng, tau, amplitude):
    """A rotation vector per frame whose every component swings within +- amplitude -> [F][3]."""
    f1, ph = rng.uniform(0.4, 1.6, 3), rng.uniform(0, 2 * np.pi, 3)
    return amplitude * np.sin(2 * np.pi * f1 * tau[:, None] + ph)


def quat_of(Rm):
    """Unit quaternions (w, x, y, z) of Rm [F][3][3], sign-continuous along F (the first with a positive leading component)."""
    F = Rm.shape[0]
    q = np.zeros((F, 4))
    for f in range(F):
        R = Rm[f]
        K = np.array([[R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]],
                      [R[2, 1] - R[1, 2], R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]],
                      [R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1]],
                      [R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1]]])
        w, v = np.linalg.eigh(K)
        q[f] = v[:, 3]
        if f == 0:
            lead = q[f][np.flatnonzero(q[f])[0]]
            if lead < 0:
                q[f] = -q[f]
        elif q[f] @ q[f - 1] < 0:
            q[f] = -q[f]
    return q


def noisy(rng, Rm, t, sigma_t, sigma_r):
    if sigma_t == 0.0 and sigma_r == 0.0:
        return Rm, t
    return Rm @ rg._rodrigues(sigma_r * rng.standard_normal(t.shape)), t + sigma_t * rng.standard_normal(t.shape)


def unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def five_body_scene(seed, F=2000, amplitude=0.5, sigma_t=0.0, sigma_r=0.0, rate=120.0):
    """body 0 - ball - body 1 - hinge - body 2; body 3 rigidly attached to body 0; body 4 flying free.
    -> flag [5][F] (all POSED), Rm [5][F][3][3], t [5][F][3], truth {"ball_a", "ball_b", "hinge_p1", "hinge_u1", "hinge_p2", "hinge_u2",
    "theta" [F]}."""
    rng = np.random.default_rng(seed)
    tau = np.arange(F) / rate
    R0, t0 = rg.rigid_motion(rng, tau, amplitude=0.6, spin=0.3)
    # body 1 is a segment of 0.28 m with its origin half way and the hinge axis square to it, as an elbow's is; every other joint lies within 9 cm of its body's origin: 5 mrad of
    # orientation noise then moves a centre by less than a millimetre, and the two joints of body 1 are far enough apart for the
    # pair (0, 2) to be no joint by a wide margin
    ball_a, ball_b = rng.uniform(-0.05, 0.05, 3), np.array([-0.14, 0.0, 0.0]) + rng.uniform(-0.02, 0.02, 3)
    R1 = R0 @ rg._rodrigues(swing(rng, tau, amplitude)) @ rg.random_rotation(rng)
    t1 = np.einsum("fij,j->fi", R0, ball_a) + t0 - np.einsum("fij,j->fi", R1, ball_b)
    phi = rng.uniform(0, 2 * np.pi)
    u1, p1, p2 = np.array([0.0, np.cos(phi), np.sin(phi)]), np.array([0.14, 0.0, 0.0]) + rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.05, 0.05, 3)
    theta = amplitude * np.sin(2 * np.pi * 0.7 * tau + 0.4)
    R12_0 = rg.random_rotation(rng)
    R2 = R1 @ rot_axis(u1, theta) @ R12_0
    t2 = np.einsum("fij,j->fi", R1, p1) + t1 - np.einsum("fij,j->fi", R2, p2)
    R3 = R0 @ rg.random_rotation(rng)
    t3 = np.einsum("fij,j->fi", R0, rng.uniform(-0.05, 0.05, 3)) + t0
    R4, t4 = rg.rigid_motion(rng, tau, amplitude=1.0)
    Rm, t = np.stack([R0, R1, R2, R3, R4]), np.stack([t0, t1, t2, t3, t4])
    for b in range(5):
        Rm[b], t[b] = noisy(rng, Rm[b], t[b], sigma_t, sigma_r)
    truth = {"ball_a": ball_a, "ball_b": ball_b, "hinge_p1": p1, "hinge_u1": u1, "hinge_p2": p2, "hinge_u2": R12_0.T @ u1, "theta": theta}
    return np.full((5, F), POSED, dtype=np.int32), np.ascontiguousarray(Rm), np.ascontiguousarray(t), truth


def line_distance(x, p, u):
    """The distance of x from the line p + s u (u a unit vector)."""
    w = np.asarray(x) - np.asarray(p)
    return float(np.linalg.norm(w - (w @ u) * u))


def session(seed, F, B, dropout=0.08):
    """B bodies over F frames: body b > 0 hangs on body b - 1 by a ball joint (b odd) or a hinge (b even), every fourth body flies
    free; `dropout` of the (body, frame) flags are FEW with NaN poses.  With four or more bodies the last one is never POSED, and
    the one before carries a NaN and +-1e200 inside POSED frames.  -> flag [B][F], Rm [B][F][3][3], t [B][F][3]."""
    rng = np.random.default_rng(seed)
    tau = np.arange(F) / 120.0
    Rm, t = np.zeros((B, F, 3, 3)), np.zeros((B, F, 3))
    for b in range(B):
        if b % 4 == 0:
            Rm[b], t[b] = rg.rigid_motion(rng, tau, amplitude=0.6, spin=0.3)
            continue
        ca, cb = rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.3, 0.3, 3)
        rel = rg._rodrigues(swing(rng, tau, 0.5)) if b % 2 else rot_axis(unit(rng), 0.5 * np.sin(2 * np.pi * rng.uniform(0.5, 1.5) * tau))
        Rm[b] = Rm[b - 1] @ rel @ rg.random_rotation(rng)
        t[b] = np.einsum("fij,j->fi", Rm[b - 1], ca) + t[b - 1] - np.einsum("fij,j->fi", Rm[b], cb)
        Rm[b], t[b] = noisy(rng, Rm[b], t[b], 0.0005, 0.005)
    flag = np.full((B, F), POSED, dtype=np.int32)
    if F > 2:
        flag[rng.uniform(size=(B, F)) < dropout] = FEW
    if B >= 4:
        flag[B - 1] = FEW
        f = np.arange(F)
        Rm[B - 2, f % 7 == 3, 1, 1] = np.nan
        t[B - 2, f % 7 == 5, 2] = 1e200
        t[B - 2, f % 7 == 6, 0] = -1e200
    Rm[flag != POSED] = np.nan
    t[flag != POSED] = np.nan
    return flag, Rm, t


def unwrapped_angle(twist, present):
    """2 atan2(twist_s, twist_c) per joint, unwrapped along its present frames (NaN elsewhere): twist [J][F][2], present [J][F]."""
    out = np.full(twist.shape[:2], NAN)
    for j in range(twist.shape[0]):
        at = np.flatnonzero((present[j] != 0) & ~np.isnan(twist[j, :, 0]))
        if at.size:
            out[j, at] = np.unwrap(2.0 * np.arctan2(twist[j, at, 1], twist[j, at, 0]))
    return out


def scene_poses(flag, Rm, t):
    """The poses of a scene as session_body_poses returns them: {"flag", "R", "t_pose", "quat"} (quat: sign-continuous, NaN where
    the body is not POSED)."""
    B, F = flag.shape
    quat = np.full((B, F, 4), NAN)
    for b in range(B):
        at = np.flatnonzero((flag[b] == POSED) & np.isfinite(Rm[b].reshape(F, 9)).all(axis=1))
        if at.size:
            quat[b, at] = quat_of(Rm[b, at])
    return {"flag": np.ascontiguousarray(flag, dtype=np.int32), "R": np.ascontiguousarray(Rm), "t_pose": np.ascontiguousarray(t), "quat": quat}


def scene_joints(out):
    """The tree edges of find_joints' tables as the helper lists them, with the fields joint_series reads."""
    joints = []
    for child in range(out["parent"].size):
        if out["parent"][child] >= 0:
            a, b = sorted((child, int(out["parent"][child])))
            joints.append({"a": a, "b": b, "kind": int(out["kind"][a, b]), "c_a": out["centre"][a, b].copy(), "c_b": out["centre"][b, a].copy(),
                           "axis_a": out["axis"][a, b].copy(), "axis_b": out["axis"][b, a].copy(), "sep": float(out["sep"][a, b]),
                           "frames": int(out["cnt"][a, b])})
    return sorted(joints, key=lambda j: (j["a"], j["b"]))


def first_relative(quat, flag, a, b):
    """conj(q_a) (x) q_b at the first frame with both bodies POSED, normalised: the helper's q_ref."""
    f0 = int(np.flatnonzero((flag[a] == POSED) & (flag[b] == POSED))[0])
    qa, qb = quat[a, f0], quat[b, f0]
    ref = np.array(hamilton([qa[0], -qa[1], -qa[2], -qa[3]], qb))
    return ref / np.sqrt(ref @ ref), f0
