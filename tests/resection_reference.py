"""The "camera resection" contract of include/mocap_core.h, stated twice.

  DOUBLE  plain IEEE doubles in the order the header pins (Python floats and NumPy elementwise operations, the math module for sin,
          cos, acos, cbrt, sqrt): the sampler, Grunert's three-point solver, the per-view residual and inlier rule, the winner, the
          rows of the normal equations, the Levenberg-Marquardt step with the cost's change taken from the increment, the two-round
          schedule and the re-gauge for camera 0.  The sums of a linearisation are folded in row order (the device folds them
          through its tree: equal up to rounding).
  MP      mpmath at 50 digits: the per-view formulas, the reprojection of a sample's three points under a given pose, and the
          minimiser of the cost over a given inlier set (Gauss-Newton from a given pose until the step is below 1e-30).

Inputs come from a seeded generator (planted_case): one camera, a planted pose, points in front of it."""
import math

import mpmath
import numpy as np

DPS = 50
MAX_POINTS, MAX_HYP, INFO = 131072, 4096, 12
OK, TOO_FEW, NO_MODEL = 0, 1, 2
INFO_KEYS = ("valid", "winner_inliers", "winner_hypothesis", "winner_solution", "no_solution", "inliers", "accepted", "linearisations",
             "rms_prior", "rms_winner", "rms_final", "status")
M64 = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15
K_TEST = np.array([[310.0, 0.0, 161.5], [0.0, 295.0, 119.25], [0.0, 0.0, 1.0]])   # plain, fx != fy


# ---------------------------------------------------------------------------------------------------------------- sampler
def mix(z):
    z = (z + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def sample(seed, h, n):
    """The three distinct valid rows of hypothesis h: a pure function of (seed, h, n)."""
    r = [mix((seed + (3 * h + k) * GOLDEN) & M64) for k in range(3)]
    i0 = r[0] % n
    i1 = r[1] % (n - 1)
    if i1 >= i0:
        i1 += 1
    i2 = r[2] % (n - 2)
    lo, hi = min(i0, i1), max(i0, i1)
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return i0, i1, i2


# ------------------------------------------------------------------------------------------------------- views and scoring
def plain_K(K):
    K = np.asarray(K, dtype=np.float64).reshape(9)
    return bool((K[[1, 3, 6, 7]] == 0).all() and K[8] == 1 and np.isfinite(K[[0, 4, 2, 5]]).all() and K[0] > 0 and K[4] > 0)


def k4_of(K):
    K = np.asarray(K, dtype=np.float64).reshape(9)
    return [float(K[0]), float(K[4]), float(K[2]), float(K[5])]


def pose_of(R, t):
    return [float(v) for v in np.asarray(R, dtype=np.float64).reshape(9)] + [float(v) for v in np.asarray(t, dtype=np.float64).reshape(3)]


def valid_rows(X, obs):
    X, obs = np.asarray(X, dtype=np.float64).reshape(-1, 3), np.asarray(obs, dtype=np.float64).reshape(-1, 2)
    ok = np.isfinite(X).all(axis=1) & np.isfinite(obs).all(axis=1)
    idx = np.nonzero(ok)[0]
    return np.hstack([X[idx], obs[idx]]), idx


def view(pose, k4, row):
    """One view in Python floats: (P, x, xn, yn, du, dv, s2)."""
    X0, X1, X2, u, v = (float(a) for a in row)
    P = [(pose[3 * i] * X0 + pose[3 * i + 1] * X1) + pose[3 * i + 2] * X2 for i in range(3)]
    x = [P[i] + pose[9 + i] for i in range(3)]
    with np.errstate(all="ignore"):
        xn, yn = float(np.float64(x[0]) / np.float64(x[2])), float(np.float64(x[1]) / np.float64(x[2]))
    du = (k4[0] * xn + k4[2]) - u
    dv = (k4[1] * yn + k4[3]) - v
    return P, x, xn, yn, du, dv, du * du + dv * dv


def views(pose, k4, rows):
    """All rows at once (NumPy elementwise, the same operations in the same order) -> (x2, s2)."""
    p = np.asarray(pose, dtype=np.float64)
    X0, X1, X2, u, v = rows.T
    with np.errstate(all="ignore"):
        P = [(p[3 * i] * X0 + p[3 * i + 1] * X1) + p[3 * i + 2] * X2 for i in range(3)]
        x = [P[i] + p[9 + i] for i in range(3)]
        du = (k4[0] * (x[0] / x[2]) + k4[2]) - u
        dv = (k4[1] * (x[1] / x[2]) + k4[3]) - v
        return x[2], du * du + dv * dv


def classify(pose, k4, rows, thr):
    x2, s2 = views(pose, k4, rows)
    with np.errstate(all="ignore"):
        return (x2 > 0.0) & (s2 < thr * thr)


def cost_over(pose, k4, rows, mask):
    """Sum of s2 over the mask, in row order."""
    _, s2 = views(pose, k4, rows)
    acc = 0.0
    for v in s2[mask]:
        acc = acc + float(v)
    return acc


# ---------------------------------------------------------------------------------------------------- rows, step, schedule
def jacobian(P, x, xn, yn, k4):
    a0, b1 = k4[0] / x[2], k4[1] / x[2]
    a2, b2 = -(a0 * xn), -(b1 * yn)
    Ju = [a2 * P[1], a0 * P[2] - a2 * P[0], -(a0 * P[1]), a0, 0.0, a2]
    Jv = [b2 * P[1] - b1 * P[2], -(b2 * P[0]), b1 * P[0], 0.0, b1, b2]
    return Ju, Jv


def row_sums(pose, k4, row):
    """The 31 values one inlier row contributes: H (upper triangle, row-major) | g | cost | 1 | behind | 0 (the cost's change)."""
    P, x, xn, yn, du, dv, s2 = view(pose, k4, row)
    Ju, Jv = jacobian(P, x, xn, yn, k4)
    s = [Ju[i] * Ju[j] + Jv[i] * Jv[j] for i in range(6) for j in range(i, 6)]
    s += [Ju[i] * du + Jv[i] * dv for i in range(6)]
    s += [s2, 1.0, 0.0 if (math.isfinite(x[2]) and x[2] > 0.0) else 1.0, 0.0]
    return s


def linearise(pose, k4, rows, mask, base=None, inc=None):
    """The sums over the mask in row order; with a base, [30] is the cost's change of the trial `pose` = base + inc."""
    acc = [0.0] * 31
    for row in rows[mask]:
        s = row_sums(pose, k4, row)
        if base is not None:
            s[30] = delta_row(base, k4, row, inc)
        acc = [a + b for a, b in zip(acc, s)]
    return acc


def lm_step(s, lam):
    A = [[0.0] * 6 for _ in range(6)]
    e = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = s[e]
            e += 1
    for i in range(6):
        A[i][i] = A[i][i] + lam * A[i][i]
    L = [[0.0] * 6 for _ in range(6)]
    for i in range(6):
        for j in range(i + 1):
            acc = A[i][j]
            for k in range(j):
                acc = acc - L[i][k] * L[j][k]
            if i == j:
                if not (math.isfinite(acc) and acc > 0.0):
                    return None
                L[i][i] = math.sqrt(acc)
            else:
                L[i][j] = acc / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        acc = -s[21 + i]
        for k in range(i):
            acc = acc - L[i][k] * y[k]
        y[i] = acc / L[i][i]
    d = [0.0] * 6
    for i in range(5, -1, -1):
        acc = y[i]
        for k in range(i + 1, 6):
            acc = acc - L[k][i] * d[k]
        d[i] = acc / L[i][i]
    return d


def increment(d):
    """(G [9] | dt [3]) of the step d = (w, dt): G = exp([w]x) - I."""
    wx, wy, wz = d[0], d[1], d[2]
    th2 = (wx * wx + wy * wy) + wz * wz
    th = math.sqrt(th2)
    if th < 1e-8:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, b = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    return [-(b * (wy * wy + wz * wz)), b * (wx * wy) - a * wz, b * (wx * wz) + a * wy,
            b * (wx * wy) + a * wz, -(b * (wx * wx + wz * wz)), b * (wy * wz) - a * wx,
            b * (wx * wz) - a * wy, b * (wy * wz) + a * wx, -(b * (wx * wx + wy * wy))] + [float(v) for v in d[3:6]]


def apply_step(pose, d, inc=None):
    """(exp([w]x) R, t + dt): E = I + G, R' = E R."""
    inc = increment(d) if inc is None else inc
    E = [[1.0 + inc[3 * i + j] if i == j else inc[3 * i + j] for j in range(3)] for i in range(3)]
    R = [(E[i][0] * pose[j] + E[i][1] * pose[3 + j]) + E[i][2] * pose[6 + j] for i in range(3) for j in range(3)]
    return R + [pose[9 + k] + inc[9 + k] for k in range(3)]


def delta_row(base, k4, row, inc):
    """s2(trial) - s2(base) of one row from the increment: the quantity 'strictly lower' is decided on."""
    P, x, xn, yn, du, dv, _ = view(base, k4, row)
    dx = [((inc[3 * i] * P[0] + inc[3 * i + 1] * P[1]) + inc[3 * i + 2] * P[2]) + inc[9 + i] for i in range(3)]
    x2t = x[2] + dx[2]
    dxn, dyn = (dx[0] - xn * dx[2]) / x2t, (dx[1] - yn * dx[2]) / x2t
    ddu, ddv = k4[0] * dxn, k4[1] * dyn
    return ddu * (2.0 * du + ddu) + ddv * (2.0 * dv + ddv)


def lm_round(pose, max_iter, lin, start=None):
    """One round over a fixed mask.  lin(pose, base, inc) -> the 31 sums (without a base the mask is re-made at the pose first).
    -> (pose, cost, accepted, linearisations)."""
    cur = start if start is not None else lin(pose, None, None)
    accepted, lins, lam = 0, 1, 1e-3
    while accepted < max_iter and cur[28] > 0.0 and lam <= 1e12:
        d = lm_step(cur, lam)
        if d is None:
            lam = lam * 10.0
            continue
        inc = increment(d)
        trial = apply_step(pose, d, inc)
        tr = lin(trial, pose, inc)
        lins += 1
        wmax = max(abs(v) for v in d[:3])
        dmax = max(abs(v) for v in d[3:])
        tmax = max(abs(v) for v in pose[9:])
        small = wmax <= 1e-12 and dmax <= 1e-12 * (1.0 + tmax)
        if math.isfinite(tr[27]) and tr[29] == 0.0 and tr[30] < 0.0:
            pose, cur = trial, tr
            lam = lam / 10.0 if lam / 10.0 > 1e-12 else 1e-12
            accepted += 1
        else:
            lam = lam * 10.0
        if small:
            break
    return pose, cur[27], accepted, lins


def refine(pose, k4, rows, thr, max_iter):
    """The two rounds -> (pose, accepted, linearisations)."""
    state = {"mask": None}

    def lin(p, base, inc):
        if base is None:
            state["mask"] = classify(p, k4, rows, thr)
        return linearise(p, k4, rows, state["mask"], base, inc)

    accepted = lins = 0
    for _ in range(2):
        pose, _, a, n = lm_round(pose, max_iter, lin)
        accepted += a
        lins += n
    return pose, accepted, lins


# ----------------------------------------------------------------------------------------------------- three-point solver
def _finite(x):
    return math.isfinite(x)


def cubic_largest(a1, a2, a3):
    Q, R = (a1 * a1 - 3.0 * a2) / 9.0, (2.0 * a1 * a1 * a1 - 9.0 * a1 * a2 + 27.0 * a3) / 54.0
    d = Q * Q * Q - R * R
    if d > 0.0:
        theta = math.acos(R / math.sqrt(Q * Q * Q))
        x = max(-2.0 * math.sqrt(Q) * math.cos((theta + k * 2.0 * math.pi) / 3.0) - a1 / 3.0 for k in range(3))
    else:
        e = (math.sqrt(-d) + abs(R)) ** (1.0 / 3.0)
        if R > 0.0:
            e = -e
        x = -a1 / 3.0 if e == 0.0 else (e + Q / e) - a1 / 3.0
    for _ in range(2):
        f, fp = ((x + a1) * x + a2) * x + a3, (3.0 * x + 2.0 * a1) * x + a2
        if fp != 0.0 and _finite(f / fp):
            x = x - f / fp
    return x


def quartic(A):
    """Real roots of A[4] x^4 + .. + A[0] (Ferrari), each polished by two Newton steps."""
    big = max(abs(v) for v in A)
    if not (_finite(big) and abs(A[4]) > 1e-14 * big):
        return []
    b, c, d, e = A[3] / A[4], A[2] / A[4], A[1] / A[4], A[0] / A[4]
    b2 = b * b
    p = c - 0.375 * b2
    q = (d - 0.5 * (b * c)) + 0.125 * (b2 * b)
    r = ((e - 0.25 * (b * d)) + 0.0625 * (b2 * c)) - (3.0 / 256.0) * (b2 * b2)
    m = cubic_largest(p, 0.25 * (p * p) - r, -0.125 * (q * q))
    y = []
    if not m > 1e-14 * max(abs(p), 1.0):
        disc = p * p - 4.0 * r
        if not disc >= 0.0:
            return []
        sq = math.sqrt(disc)
        for z in (0.5 * (-p + sq), 0.5 * (-p - sq)):
            if z >= 0.0:
                y += [math.sqrt(z), -math.sqrt(z)]
    else:
        s, h, k = math.sqrt(2.0 * m), 0.5 * p + m, q / (2.0 * math.sqrt(2.0 * m))
        d1 = s * s - 4.0 * (h + k)
        if d1 >= 0.0:
            y += [0.5 * (s + math.sqrt(d1)), 0.5 * (s - math.sqrt(d1))]
        d2 = s * s - 4.0 * (h - k)
        if d2 >= 0.0:
            y += [0.5 * (-s + math.sqrt(d2)), 0.5 * (-s - math.sqrt(d2))]
    out = []
    for yi in y:
        v = yi - 0.25 * b
        for _ in range(2):
            f = (((A[4] * v + A[3]) * v + A[2]) * v + A[1]) * v + A[0]
            fp = ((4.0 * A[4] * v + 3.0 * A[3]) * v + 2.0 * A[2]) * v + A[1]
            if fp != 0.0 and _finite(f / fp):
                v = v - f / fp
        out.append(v)
    return out


def _triad(p1, p2, p3):
    a, c = p2 - p1, p3 - p1
    na = math.sqrt(float(a @ a))
    if not na > 0.0:
        return None
    e1 = a / na
    e3 = np.cross(e1, c)
    n3 = math.sqrt(float(e3 @ e3))
    if not n3 > 0.0:
        return None
    e3 = e3 / n3
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)


def p3p(P, uv, k4):
    """Grunert -> list of (pose [12], conditioning) with conditioning = (relative gap to the nearest other real root,
    |cos gamma - v cos alpha|)."""
    P, uv = np.asarray(P, dtype=np.float64), np.asarray(uv, dtype=np.float64)
    j = np.stack([(uv[:, 0] - k4[2]) / k4[0], (uv[:, 1] - k4[3]) / k4[1], np.ones(3)], axis=1)
    j = j / np.sqrt((j * j).sum(axis=1))[:, None]
    a2, b2, c2 = (float(((P[i] - P[k]) ** 2).sum()) for i, k in ((1, 2), (0, 2), (0, 1)))
    longest = max(a2, b2, c2)
    if not (_finite(longest) and min(a2, b2, c2) > 1e-18 * longest):
        return []
    cr = np.cross(P[1] - P[0], P[2] - P[0])
    if not float(cr @ cr) > 1e-12 * (b2 * c2):
        return []
    ca, cb, cg = float(j[1] @ j[2]), float(j[0] @ j[2]), float(j[0] @ j[1])
    q, p, rc, ra = (a2 - c2) / b2, (a2 + c2) / b2, c2 / b2, a2 / b2
    A = [0.0] * 5
    A[4] = (q - 1.0) ** 2 - 4.0 * rc * ca * ca
    A[3] = 4.0 * ((q * (1.0 - q) * cb - (1.0 - p) * ca * cg) + 2.0 * rc * ca * ca * cb)
    A[2] = 2.0 * (((((q * q - 1.0) + 2.0 * q * q * cb * cb) + 2.0 * ((b2 - c2) / b2) * ca * ca) - 4.0 * p * ca * cb * cg)
                  + 2.0 * ((b2 - a2) / b2) * cg * cg)
    A[1] = 4.0 * ((-(q * (1.0 + q)) * cb + 2.0 * ra * cg * cg * cb) - (1.0 - p) * ca * cg)
    A[0] = (1.0 + q) ** 2 - 4.0 * ra * cg * cg
    roots = quartic(A)
    Tw = _triad(P[0], P[1], P[2])
    if Tw is None:
        return []
    out, b = [], math.sqrt(b2)
    for r, v in enumerate(roots):
        if not v > 0.0:
            continue
        den = 2.0 * (cg - v * ca)
        if den == 0.0:
            continue
        u = ((((q - 1.0) * v * v - 2.0 * q * cb * v) + 1.0) + q) / den
        w = (1.0 + v * v) - 2.0 * v * cb
        if not (u > 0.0 and w > 0.0):
            continue
        s1 = b / math.sqrt(w)
        Q = [s1 * j[0], u * s1 * j[1], v * s1 * j[2]]
        Tc = _triad(*Q)
        if Tc is None:
            continue
        R = Tc @ Tw.T
        t = Q[0] - R @ P[0]
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            continue
        gap = min([abs(v - o) for k, o in enumerate(roots) if k != r] or [math.inf]) / max(abs(v), 1.0)
        out.append((pose_of(R, t), (gap, abs(cg - v * ca))))
    return out


# ---------------------------------------------------------------------------------------------------- search and full solve
def hypotheses(X, obs, K, prior, thr, n_hyp, seed):
    """The candidate table: sample [H][3] (input rows, -1: none), n_sol [H], poses [H][4][12] (NaN: none), counts [H][4], and the
    conditioning of every solution."""
    rows, idx = valid_rows(X, obs)
    k4, n, H = k4_of(K), len(idx), max(int(n_hyp), 1)
    out = dict(sample=np.full((H, 3), -1, dtype=np.int32), n_sol=np.zeros(H, dtype=np.int32), poses=np.full((H, 4, 12), np.nan),
               counts=np.zeros((H, 4), dtype=np.int32), cond=[[] for _ in range(H)], rows=rows, idx=idx)
    for h in range(H):
        if h == 0 and prior is not None:
            sols = [(pose_of(*prior), (math.inf, math.inf))]
        elif n >= 4:
            pick = sample(int(seed), h, n)
            out["sample"][h] = idx[list(pick)]
            sols = p3p(rows[list(pick), :3], rows[list(pick), 3:], k4)
        else:
            sols = []
        out["n_sol"][h] = len(sols)
        for s, (pose, cond) in enumerate(sols):
            out["poses"][h, s] = pose
            out["counts"][h, s] = int(classify(pose, k4, rows, thr).sum())
            out["cond"][h].append(cond)
    return out


def score_poses(poses, n_sol, K, X, obs, thr):
    """counts [H][4] of given poses (the device's own) under the stated rule."""
    rows, _ = valid_rows(X, obs)
    k4 = k4_of(K)
    counts = np.zeros(poses.shape[:2], dtype=np.int32)
    for h in range(poses.shape[0]):
        for s in range(int(n_sol[h])):
            counts[h, s] = int(classify(list(poses[h, s]), k4, rows, thr).sum())
    return counts


def winner(counts, n_sol):
    """Most inliers, ties to the lower (hypothesis, solution) -> (h, s, count) or (-1, -1, 0)."""
    best = (-1, -1, -1)
    for h in range(counts.shape[0]):
        for s in range(int(n_sol[h])):
            if int(counts[h, s]) > best[2]:
                best = (h, s, int(counts[h, s]))
    return best if best[0] >= 0 else (-1, -1, 0)


def _rms(pose, k4, rows, mask):
    n = int(mask.sum())
    return math.sqrt(cost_over(pose, k4, rows, mask) / n) if n else math.nan


def resect(X, obs, K, prior=None, thr=2.0, n_hyp=256, seed=0, min_inliers=6, max_iter=20):
    """mocap_resect_camera -> (R [3][3], t [3], mask [N] bool, info dict)."""
    N = np.asarray(X).reshape(-1, 3).shape[0]
    tab = hypotheses(X, obs, K, prior, thr, n_hyp, seed)
    rows, idx, k4 = tab["rows"], tab["idx"], k4_of(K)
    h, s, cnt = winner(tab["counts"], tab["n_sol"])
    status = TOO_FEW if len(idx) < 4 else NO_MODEL if (h < 0 or cnt < min_inliers) else OK
    accepted = lins = 0
    if status == OK:
        win = [float(v) for v in tab["poses"][h, s]]
        pose = win
        if max_iter > 0:
            pose, accepted, lins = refine(win, k4, rows, thr, max_iter)
    else:
        win = pose = pose_of(*prior) if prior is not None else [math.nan] * 12
        lins = 1 if max_iter > 0 else 0
    fm = classify(pose, k4, rows, thr)
    mask = np.zeros(N, dtype=bool)
    mask[idx[fm]] = True
    info = dict(valid=len(idx), winner_inliers=cnt, winner_hypothesis=h, winner_solution=s,
                no_solution=int((tab["n_sol"] == 0).sum()), inliers=int(fm.sum()), accepted=accepted, linearisations=lins,
                rms_prior=_rms(pose_of(*prior), k4, rows, fm) if prior is not None else math.nan, rms_winner=_rms(win, k4, rows, fm),
                rms_final=_rms(pose, k4, rows, fm), status=status)
    return np.array(pose[:9]).reshape(3, 3), np.array(pose[9:]), mask, info


# ------------------------------------------------------------------------------------------------------------- re-gauge
def regauge(R, t, R0, t0):
    """Camera 0 re-seated at (R0, t0) in the old frame -> poses in the frame where it is (I, 0) again, and the matrix to right-multiply
    onto to_world_coords_matrix so that world coordinates do not move: R_c' = R_c R0^T, t_c' = t_c - R_c R0^T t0."""
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    R0, t0 = np.asarray(R0, dtype=np.float64).reshape(3, 3), np.asarray(t0, dtype=np.float64).reshape(3)
    Rn = np.array([Rc @ R0.T for Rc in R])
    tn = np.array([tc - Rc @ R0.T @ t0 for Rc, tc in zip(R, t)])
    Rn[0], tn[0] = np.eye(3), np.zeros(3)
    D = np.diag([-1.0, -1.0, 1.0])
    M = np.eye(4)
    M[:3, :3] = D @ R0.T @ D
    M[:3, 3] = -D @ R0.T @ t0
    return Rn, tn, M


# --------------------------------------------------------------------------------------------------------------- 50 digits
def _mpf(v):
    return mpmath.mpf(float(v))


def mp_residual(pose, k4, row):
    """(du, dv, x2) of one view at 50 digits; pose and row are the doubles as given."""
    with mpmath.workdps(DPS):
        p, r, k = [_mpf(v) for v in pose], [_mpf(v) for v in row], [_mpf(v) for v in k4]
        x = [p[3 * i] * r[0] + p[3 * i + 1] * r[1] + p[3 * i + 2] * r[2] + p[9 + i] for i in range(3)]
        return k[0] * x[0] / x[2] + k[2] - r[3], k[1] * x[1] / x[2] + k[3] - r[4], x[2]


def mp_sample_error(pose, k4, sample_rows):
    """Largest reprojection distance (pixels) of a sample's three rows under a pose, and max |R^T R - I|, at 50 digits."""
    with mpmath.workdps(DPS):
        worst = mpmath.mpf(0)
        for row in sample_rows:
            du, dv, _ = mp_residual(pose, k4, row)
            worst = max(worst, mpmath.sqrt(du * du + dv * dv))
        R = mpmath.matrix(3, 3)
        for i in range(9):
            R[i // 3, i % 3] = _mpf(pose[i])
        E = R.T * R - mpmath.eye(3)
        return float(worst), float(max(abs(E[i, k]) for i in range(3) for k in range(3)))


def _mp_rodrigues(w):
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    W = mpmath.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th2 == 0:
        return mpmath.eye(3)
    th = mpmath.sqrt(th2)
    return mpmath.eye(3) + (mpmath.sin(th) / th) * W + ((1 - mpmath.cos(th)) / th2) * (W * W)


def _mp_terms(R, t, k, rows):
    """Residuals and the analytic rows [-D [R X]x | D] at 50 digits."""
    out = []
    for r in rows:
        X = mpmath.matrix([r[0], r[1], r[2]])
        P = R * X
        x = P + t
        xn, yn = x[0] / x[2], x[1] / x[2]
        du, dv = k[0] * xn + k[2] - r[3], k[1] * yn + k[3] - r[4]
        a0, b1 = k[0] / x[2], k[1] / x[2]
        a2, b2 = -a0 * xn, -b1 * yn
        Ju = [a2 * P[1], a0 * P[2] - a2 * P[0], -a0 * P[1], a0, mpmath.mpf(0), a2]
        Jv = [b2 * P[1] - b1 * P[2], -b2 * P[0], b1 * P[0], mpmath.mpf(0), b1, b2]
        out.append((du, dv, Ju, Jv))
    return out


def _mp_pose(pose):
    R = mpmath.matrix(3, 3)
    for i in range(9):
        R[i // 3, i % 3] = _mpf(pose[i])
    for _ in range(6):                       # the nearest rotation (Newton's polar iteration): the doubles are orthonormal to 1e-16 only
        R = (R + mpmath.inverse(R).T) / 2
    return R, mpmath.matrix([_mpf(v) for v in pose[9:]])


def mp_jacobian_fd(pose, k4, row, h=1e-20):
    """Central differences of (du, dv) in the six unknowns at 50 digits, and the analytic rows -> (fd [2][6], analytic [2][6])."""
    with mpmath.workdps(DPS):
        R, t = _mp_pose(pose)
        k, r = [_mpf(v) for v in k4], [_mpf(v) for v in row]
        _, _, Ju, Jv = _mp_terms(R, t, k, [r])[0]
        fd = [[None] * 6, [None] * 6]
        hh = mpmath.mpf(h)
        for i in range(6):
            vals = []
            for sgn in (1, -1):
                d = [mpmath.mpf(0)] * 6
                d[i] = sgn * hh
                du, dv, _, _ = _mp_terms(_mp_rodrigues(d[:3]) * R, t + mpmath.matrix(d[3:]), k, [r])[0]
                vals.append((du, dv))
            fd[0][i] = (vals[0][0] - vals[1][0]) / (2 * hh)
            fd[1][i] = (vals[0][1] - vals[1][1]) / (2 * hh)
        return fd, [Ju, Jv]


def mp_minimise(pose, k4, rows, mask, tol=1e-30, max_steps=30):
    """The minimiser of sum s2 over the rows of the mask: Gauss-Newton at 50 digits from `pose` until the step is below tol
    -> (R mpmath 3x3, t mpmath 3, cost)."""
    with mpmath.workdps(DPS):
        R, t = _mp_pose(pose)
        k = [_mpf(v) for v in k4]
        rr = [[_mpf(v) for v in row] for row in np.asarray(rows)[np.asarray(mask, dtype=bool)]]
        for _ in range(max_steps):
            H, g = mpmath.zeros(6, 6), mpmath.zeros(6, 1)
            for du, dv, Ju, Jv in _mp_terms(R, t, k, rr):
                for i in range(6):
                    g[i] += Ju[i] * du + Jv[i] * dv
                    for j in range(i, 6):
                        H[i, j] += Ju[i] * Ju[j] + Jv[i] * Jv[j]
            for i in range(6):
                for j in range(i):
                    H[i, j] = H[j, i]
            d = mpmath.lu_solve(H, -g)
            R = _mp_rodrigues([d[0], d[1], d[2]]) * R
            t = t + mpmath.matrix([d[3], d[4], d[5]])
            if max(abs(v) for v in d) < tol:
                break
        else:
            raise RuntimeError("the 50-digit Gauss-Newton iteration did not converge")
        cost = sum((du * du + dv * dv for du, dv, _, _ in _mp_terms(R, t, k, rr)), mpmath.mpf(0))
        return R, t, cost


def mp_distance(pose, Rm, tm):
    """(max |R - R_min|, |t - t_min|) of a double pose to a 50-digit one."""
    with mpmath.workdps(DPS):
        dr = max(abs(_mpf(pose[i]) - Rm[i // 3, i % 3]) for i in range(9))
        dt = mpmath.sqrt(sum((_mpf(pose[9 + i]) - tm[i]) ** 2 for i in range(3)))
        return float(dr), float(dt)


def mp_cost(pose, k4, rows, mask):
    with mpmath.workdps(DPS):
        acc = mpmath.mpf(0)
        for row in np.asarray(rows)[np.asarray(mask, dtype=bool)]:
            du, dv, _ = mp_residual(pose, k4, row)
            acc += du * du + dv * dv
        return acc


# ------------------------------------------------------------------------------------------------------------------ inputs
def _rotation(rng, max_angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    return np.array(apply_step([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0], list(axis * max_angle) + [0.0] * 3)[:9]).reshape(3, 3)


def planted_case(N, outliers=0.0, noise=0.0, n_nan=0, prior_off=None, seed=0, K=K_TEST):
    """One camera with a planted pose, N points in front of it (depth 2 .. 6, inside a 320 x 240 picture).  `outliers`: that share of
    the views moved by 20 .. 50 px; `noise`: Gaussian, pixels; n_nan rows get a NaN in X or obs; prior_off = (degrees, metres): a prior
    that far from the planted pose.  -> dict(X, obs, K, R, t, mask (the planted inliers), prior)."""
    rng = np.random.default_rng([int(N), int(seed), 20261020])
    R = _rotation(rng, 0.7) @ np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])
    t = np.array([0.2, -0.1, 0.3]) + rng.normal(size=3) * 0.1
    k4 = k4_of(K)
    u = rng.uniform(10.0, 310.0, N)
    v = rng.uniform(10.0, 230.0, N)
    z = rng.uniform(2.0, 6.0, N)
    xc = np.stack([(u - k4[2]) / k4[0] * z, (v - k4[3]) / k4[1] * z, z], axis=1)
    X = (xc - t) @ R                                   # R^T (xc - t)
    proj = X @ R.T + t
    obs = np.stack([k4[0] * proj[:, 0] / proj[:, 2] + k4[2], k4[1] * proj[:, 1] / proj[:, 2] + k4[3]], axis=1)
    if noise:
        obs = obs + np.clip(rng.normal(size=obs.shape), -3.0, 3.0) * noise
    mask = np.ones(N, dtype=bool)
    n_out = int(round(outliers * N))
    if n_out:
        bad = rng.choice(N, n_out, replace=False)
        ang, mag = rng.uniform(0, 2 * np.pi, n_out), rng.uniform(20.0, 50.0, n_out)
        obs[bad] += np.stack([np.cos(ang), np.sin(ang)], axis=1) * mag[:, None]
        mask[bad] = False
    if n_nan:
        gone = rng.choice(N, n_nan, replace=False)
        for k, i in enumerate(gone):
            if k % 2:
                X[i, k % 3] = np.nan
            else:
                obs[i, k % 2] = np.nan
        mask[gone] = False
    prior = None
    if prior_off is not None:
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        step = list(axis * math.radians(prior_off[0]))
        shift = rng.normal(size=3)
        shift *= prior_off[1] / np.linalg.norm(shift)
        p = apply_step(pose_of(R, t), step + list(shift))
        prior = (np.array(p[:9]).reshape(3, 3), np.array(p[9:]))
    return dict(X=X, obs=obs, K=np.array(K, dtype=np.float64), R=R, t=t, mask=mask, prior=prior)


# the four inputs of the GPU test: (N, n_hyp) and how the data is made; the threshold is 2 px throughout
CASES = {
    "exact6": dict(N=6, n_hyp=16, make=dict()),
    "noisy67": dict(N=67, n_hyp=64, make=dict(outliers=0.2, noise=0.3)),
    "prior257": dict(N=257, n_hyp=64, make=dict(outliers=0.3, noise=0.3, n_nan=9, prior_off=(3.0, 0.03))),
    "noisy1031": dict(N=1031, n_hyp=257, make=dict(outliers=0.2, noise=0.3)),
}
THRESHOLD = 2.0
SEED = 7
MAX_ITER = 20

_cases = {}


def case(name):
    """A case with the statement's own results, computed once: the candidate table, the full solve and the 50-digit minimiser over
    the statement's final mask with the statement's distance to it."""
    if name not in _cases:
        spec = CASES[name]
        c = planted_case(spec["N"], seed=3, **spec["make"])
        c["n_hyp"], c["min_inliers"] = spec["n_hyp"], min(8, spec["N"])
        c["table"] = hypotheses(c["X"], c["obs"], c["K"], c["prior"], THRESHOLD, c["n_hyp"], SEED)
        c["solve"] = resect(c["X"], c["obs"], c["K"], c["prior"], THRESHOLD, c["n_hyp"], SEED, c["min_inliers"], MAX_ITER)
        _cases[name] = c
    return _cases[name]


def minimiser(name):
    """(R_min, t_min, cost_min, statement's distance (dR, dt)) over the statement's final mask, computed once."""
    c = case(name)
    if "min" not in c:
        R, t, mask, _ = c["solve"]
        rows, idx = c["table"]["rows"], c["table"]["idx"]
        Rm, tm, cost = mp_minimise(pose_of(R, t), k4_of(c["K"]), rows, mask[idx])
        c["min"] = (Rm, tm, cost, mp_distance(pose_of(R, t), Rm, tm))
    return c["min"]
