"""Plain statement of the rigid-body contract of include/mocap_core.h ("rigid bodies"), for the tests.

  - validate():       the MOCAP_E_ARG rules of mocap_set_rigid_bodies
  - posable_table():  the 256-entry table over marker subsets
  - search():         the EXHAUSTIVE recursion over the assignment tuples -- no pruning beyond the gates -- that returns the
                      winner's key (-count, score, tuple) and the runner-up's
  - count_extensions(): the walk the header documents for the work cap (depth first, candidates ascending, then "unassigned",
                      pruned on the search's own best count only) and the number of extensions it makes
  - locate():         bodies in index order over one frame, claiming, SVD-Kabsch for the pose, rms rejection, work cap
  - kabsch(), horn(): the pose by SVD and by Horn's quaternion matrix, float64
  - pose_mp():        the pose of a given assignment with 50 significant digits (mpmath)
  - make_body(), make_scene(): synthetic bodies and frames with planted poses

Scalars are Python floats: IEEE double, one rounding per operation, math.sqrt correctly rounded, nothing fused -- the
arithmetic the contract prescribes for D, the gate and the score."""
import math

import numpy as np

MAX_BODIES, MAX_MARKERS, MAX_POINTS = 8, 8, 64
DEFAULT_WORK_CAP = 65536
ST_RMS, ST_WORK_CAP = 1, 2


def dist(p, q):
    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def triple_spans(qi, qj, qk):
    u = [qj[0] - qi[0], qj[1] - qi[1], qj[2] - qi[2]]
    v = [qk[0] - qi[0], qk[1] - qi[1], qk[2] - qi[2]]
    c = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    nc = math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    nu = math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    nv = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return nc >= (0.1 * nu) * nv


def posable_table(markers):
    """[2^N] bools: subset s (bit m = marker m) has >= 3 markers and holds a spanning triple."""
    q = [[float(v) for v in row] for row in np.asarray(markers, dtype=np.float64).reshape(-1, 3)]
    n = len(q)
    good = [(i, j, k) for i in range(n) for j in range(i + 1, n) for k in range(j + 1, n) if triple_spans(q[i], q[j], q[k])]
    return [any((s >> i & 1) and (s >> j & 1) and (s >> k & 1) for (i, j, k) in good) for s in range(1 << n)]


def validate(bodies, tol, max_rms, work_cap=0):
    """None when mocap_set_rigid_bodies accepts the registration, else the reason it returns MOCAP_E_ARG for."""
    if len(bodies) > MAX_BODIES:
        return "more than 8 bodies"
    if len(bodies) == 0:
        return None
    if not (tol > 0 and max_rms > 0 and math.isfinite(tol) and math.isfinite(max_rms)) or work_cap < 0:
        return "tol / max_rms / work_cap"
    for b, m in enumerate(bodies):
        m = np.asarray(m, dtype=np.float64).reshape(-1, 3)
        if not 3 <= m.shape[0] <= MAX_MARKERS:
            return f"body {b}: {m.shape[0]} markers"
        if not np.isfinite(m).all():
            return f"body {b}: non-finite coordinate"
        q = m.tolist()
        for i in range(len(q)):
            for j in range(i + 1, len(q)):
                if dist(q[i], q[j]) < 2.0 * tol:
                    return f"body {b}: markers {i} and {j} closer than 2 tol"
        if not posable_table(m)[-1]:
            return f"body {b}: not posable"
    return None


class Model:
    def __init__(self, markers):
        self.q = np.asarray(markers, dtype=np.float64).reshape(-1, 3)
        self.n = self.q.shape[0]
        ql = self.q.tolist()
        self.d = [[dist(ql[i], ql[j]) for j in range(self.n)] for i in range(self.n)]
        self.posable = posable_table(self.q)


def _dmat(points):
    P = [[float(v) for v in row] for row in points]
    return [[dist(p, q) for q in P] for p in P]


def _key(model, D, a):
    """(-count, score, tuple) of a complete tuple whose pairs pass the gates; None when the subset is not posable."""
    sub = sum(1 << m for m, p in enumerate(a) if p >= 0)
    if not model.posable[sub]:
        return None
    score = 0.0
    for i in range(model.n):
        for j in range(i + 1, model.n):
            if a[i] >= 0 and a[j] >= 0:
                e = D[a[i]][a[j]] - model.d[i][j]
                score = score + e * e
    return (-bin(sub).count("1"), score, tuple(a))


def _passes(model, D, a, m, p, tol):
    return all(a[i] < 0 or abs(D[a[i]][p] - model.d[i][m]) < tol for i in range(m))


def search(points, model, tol, free=None):
    """Exhaustive: every tuple that passes the gates is visited.  -> {"best": key or None, "runner_up": key or None, "nodes"}."""
    n = len(points)
    D = _dmat(points)
    free = set(range(n)) if free is None else set(free)
    out = {"best": None, "runner_up": None, "nodes": 0}
    a = [-1] * model.n

    def rec(m):
        out["nodes"] += 1
        if m == model.n:
            k = _key(model, D, a)
            if k is not None:
                if out["best"] is None or k < out["best"]:
                    out["best"], out["runner_up"] = k, out["best"]
                elif out["runner_up"] is None or k < out["runner_up"]:
                    out["runner_up"] = k
            return
        a[m] = -1
        rec(m + 1)
        for p in sorted(free):
            if p not in a[:m] and _passes(model, D, a, m, p, tol):
                a[m] = p
                rec(m + 1)
        a[m] = -1

    rec(0)
    return out


def count_extensions(points, model, tol, free=None, cap=None):
    """The walk of the header's "work cap" paragraph.  -> (extensions made, best key it found); stops at cap + 1 extensions."""
    n = len(points)
    D = _dmat(points)
    free = set(range(n)) if free is None else set(free)
    st = {"work": 0, "best": None, "capped": False}
    a = [-1] * model.n

    def rec(m, c):
        if st["capped"]:
            return
        left = model.n - m
        bc = -st["best"][0] if st["best"] is not None else 0
        if c + left < 3 or c + left < bc:
            return
        if m == model.n:
            k = _key(model, D, a)
            if k is not None and (st["best"] is None or k < st["best"]):
                st["best"] = k
            return
        for p in sorted(free):
            if p not in a[:m] and _passes(model, D, a, m, p, tol):
                st["work"] += 1
                if cap is not None and st["work"] > cap:
                    st["capped"] = True
                    return
                a[m] = p
                rec(m + 1, c + 1)
                if st["capped"]:
                    return
        a[m] = -1
        rec(m + 1, c)

    rec(0, 0)
    return st["work"], st["best"]


def kabsch(Q, P):
    """Least-squares proper rotation and translation body -> world by SVD: P ~ R Q + t.  -> R, t, rms."""
    Q, P = np.asarray(Q, dtype=np.float64), np.asarray(P, dtype=np.float64)
    qb, pb = Q.mean(axis=0), P.mean(axis=0)
    H = (Q - qb).T @ (P - pb)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    t = pb - R @ qb
    r = (R @ Q.T).T + t - P
    return R, t, float(np.sqrt((r * r).sum() / Q.shape[0]))


def _horn_matrix(S):
    return [[S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]],
            [S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]],
            [S[2][0] - S[0][2], S[0][1] + S[1][0], S[1][1] - S[0][0] - S[2][2], S[1][2] + S[2][1]],
            [S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], S[2][2] - S[0][0] - S[1][1]]]


def _quat_to_R(w, x, y, z):
    return [[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]]


def horn(Q, P):
    """The same pose by the contract's route: dominant eigenvector of Horn's 4 x 4 matrix (numpy eigh), float64."""
    Q, P = np.asarray(Q, dtype=np.float64), np.asarray(P, dtype=np.float64)
    qb, pb = Q.mean(axis=0), P.mean(axis=0)
    S = (Q - qb).T @ (P - pb)
    w, V = np.linalg.eigh(np.array(_horn_matrix(S)))
    q = V[:, np.argmax(w)]
    q = q / np.linalg.norm(q)
    R = np.array(_quat_to_R(*q))
    t = pb - R @ qb
    r = (R @ (Q - qb).T).T - (P - pb)
    return R, t, float(np.sqrt((r * r).sum() / Q.shape[0]))


def pose_mp(Q, P, digits=50):
    """The pose of the contract with `digits` significant digits.  -> (R 3x3, t [3], rms) as mpmath numbers in lists."""
    import mpmath as mp
    with mp.workdps(digits):
        n = len(Q)
        Qm = [[mp.mpf(float(v)) for v in row] for row in Q]
        Pm = [[mp.mpf(float(v)) for v in row] for row in P]
        qb = [sum(r[k] for r in Qm) / n for k in range(3)]
        pb = [sum(r[k] for r in Pm) / n for k in range(3)]
        S = [[sum((Qm[i][a] - qb[a]) * (Pm[i][b] - pb[b]) for i in range(n)) for b in range(3)] for a in range(3)]
        E, V = mp.eigsy(mp.matrix(_horn_matrix(S)))
        k = max(range(4), key=lambda i: E[i])
        q = [V[i, k] for i in range(4)]
        nq = mp.sqrt(sum(v * v for v in q))
        R = _quat_to_R(*[v / nq for v in q])
        t = [pb[i] - sum(R[i][j] * qb[j] for j in range(3)) for i in range(3)]
        ss = mp.mpf(0)
        for i in range(n):
            for r in range(3):
                e = sum(R[r][j] * Qm[i][j] for j in range(3)) + t[r] - Pm[i][r]
                ss += e * e
        return R, t, mp.sqrt(ss / n)


def pose_errors(R, t, rms, ref):
    """max |R - R_ref|, max |t - t_ref|, |rms - rms_ref| of a float64 pose against pose_mp's, evaluated in mpmath."""
    import mpmath as mp
    Rm, tm, rm = ref
    with mp.workdps(50):
        dR = max(abs(mp.mpf(float(R[i][j])) - Rm[i][j]) for i in range(3) for j in range(3))
        dt = max(abs(mp.mpf(float(t[i])) - tm[i]) for i in range(3))
        dr = abs(mp.mpf(float(rms)) - rm)
        return float(dR), float(dt), float(dr)


def locate(points, n, bodies, tol, max_rms, work_cap=DEFAULT_WORK_CAP, with_runner_up=True):
    """One frame: `points` [K_max][3], its first n count; bodies = list of Model.  -> one dict per body with the contract's
    outputs (zero-filled when not found) plus "runner_up" (key), "best" (key) and "extensions"."""
    K_max = len(points)
    n = 0 if (n < 0 or n > K_max) else int(n)
    pts = np.asarray(points, dtype=np.float64)[:n]
    free = set(range(n))
    res = []
    for model in bodies:
        o = {"found": 0, "n_used": 0, "assign": [0] * MAX_MARKERS, "R": np.zeros((3, 3)), "t": np.zeros(3), "rms": 0.0,
             "score": 0.0, "status": 0, "best": None, "runner_up": None, "extensions": 0}
        ext, walk_best = count_extensions(pts, model, tol, free, cap=work_cap)
        o["extensions"] = ext
        if ext > work_cap:
            o["status"] = ST_WORK_CAP
            res.append(o)
            continue
        if with_runner_up:
            s = search(pts, model, tol, free)
            assert s["best"] == walk_best, "the pruned walk and the exhaustive recursion disagree"
            o["best"], o["runner_up"] = s["best"], s["runner_up"]
        else:
            o["best"] = walk_best
        if o["best"] is not None:
            cnt, score, a = o["best"]
            used = [m for m in range(model.n) if a[m] >= 0]
            R, t, rms = kabsch(model.q[used], pts[[a[m] for m in used]])
            if rms > max_rms:
                o["status"] = ST_RMS
            else:
                o.update(found=1, n_used=-cnt, assign=list(a) + [-1] * (MAX_MARKERS - model.n), R=R, t=t, rms=rms, score=score)
                free -= {a[m] for m in used}
        res.append(o)
    return res


# ---------------------------------------------------------------- synthetic bodies and scenes
def random_rotation(rng):
    A = rng.standard_normal((3, 3))
    Qm, Rm = np.linalg.qr(A)
    Qm = Qm * np.sign(np.diag(Rm))
    if np.linalg.det(Qm) < 0:
        Qm[:, 0] = -Qm[:, 0]
    return Qm


def make_body(rng, n_markers, size=0.3, min_sep=0.06):
    """n markers in a cube of edge `size`, every pair at least min_sep apart, the full set posable."""
    for _ in range(10000):
        q = rng.uniform(-size / 2, size / 2, (n_markers, 3))
        d = [dist(q[i], q[j]) for i in range(n_markers) for j in range(i + 1, n_markers)]
        if min(d) < min_sep:
            continue
        if posable_table(q)[-1]:
            return q
    raise RuntimeError("no body found")


def make_scene(rng, bodies, K_max, n_clutter, noise=0.0005, hide=(), cube=2.0, shuffle=True):
    """One frame: every body planted at a random pose in a cube of edge `cube` (markers listed in hide[b] left out), n_clutter
    uniform points, Gaussian noise, shuffled.  -> points [K_max][3] (NaN beyond n), n, planted = [{"R", "t", "assign"}]."""
    pts, owner = [], []
    planted = []
    for b, q in enumerate(bodies):
        q = np.asarray(q, dtype=np.float64)
        R, t = random_rotation(rng), rng.uniform(-cube / 2, cube / 2, 3)
        planted.append({"R": R, "t": t, "assign": [-1] * q.shape[0]})
        hidden = set(hide[b]) if b < len(hide) else set()
        for m in range(q.shape[0]):
            if m not in hidden:
                pts.append(R @ q[m] + t + rng.normal(0.0, noise, 3) if noise else R @ q[m] + t)
                owner.append((b, m))
    for _ in range(n_clutter):
        pts.append(rng.uniform(-cube / 2, cube / 2, 3))
        owner.append(None)
    n = len(pts)
    assert n <= K_max, (n, K_max)
    order = rng.permutation(n) if shuffle else np.arange(n)
    out = np.full((K_max, 3), np.nan)
    for slot, src in enumerate(order):
        out[slot] = pts[src]
        if owner[src] is not None:
            b, m = owner[src]
            planted[b]["assign"][m] = slot
    return out, n, planted
