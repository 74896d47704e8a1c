"""The "body trajectories" contract of include/mocap_core.h in plain Python and NumPy, in the scalar order the header writes.

    validate(bodies, R, F)                          None, or the reason the core returns MOCAP_E_ARG for
    pose_sample(points, model)                      the fit of one (body, frame) in Python floats -> (quat, R, t, rms)
    pose_rows(traj, bodies, max_rms)                stage 1 -> {"n_used", "present", "quat", "R", "t_pose", "rms", "flag"}
    sign_walk(quat, posed) / sign_parity(...)       the sign rule as the header's walk, and as the prefix parity the device computes
    smooth_rotations(t, quat, degree, W, span, n_min, max_gap)   stage 2 -> {"quat_s", "omega", "res", "n_used", "flag"}
    smooth_rotations_mp(...)                        quat_s and omega of the same windows in 50 digits (mpmath)
    fill_rows(traj, bodies, flag, Rm, t_pose, flag_s=None, quat_s=None, pos_s=None)   stage 3 -> {"filled", "src"}

pose_rows() and smooth_rotations() are vectorised over frames only, as tests/track_smooth_reference.py's smooth() is: every element
goes through the operations of the scalar statement in the same order (NumPy's elementwise +, -, *, /, sqrt are IEEE double, one
rounding each, never fused), markers, Jacobi pairs and window offsets are walked by Python loops, and a lane that takes no part in a
step keeps its value (np.where, not a product with 0).  pose_sample() is the same fit in Python floats; the two are compared bit
for bit in tests/test_body_session_reference_cpu.py; the device is compared with the vectorised forms.

bodies = [(rows [N], markers [N][3])].  The posable table, the scenes and the smoother's decisions come from the statements that
already exist: rigid_body_reference, rigid_groups_reference, track_smooth_reference."""
import math

import numpy as np

import rigid_body_reference as rbr
import track_smooth_reference as tsr
from rigid_groups_reference import rigid_motion, template  # noqa: F401  (the scenes of the tests)
from track_smooth_reference import same_bits  # noqa: F401

MAX_BODIES, MAX_MARKERS, MAX_ROWS = 64, 8, 1024
POSED, FEW, DEGENERATE, RMS = 1, 2, 4, 8
SRC_NONE, SRC_MEASURED, SRC_RIGID, SRC_RIGID_FILLED = 0, 1, 2, 3
NAN = float("nan")
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def validate(bodies, R, F):
    if not 1 <= len(bodies) <= MAX_BODIES:
        return "B outside 1 .. 64"
    if F < 1 or not 1 <= R <= MAX_ROWS or R * F > 2 ** 31:
        return "n_frames / R"
    taken = set()
    for b, (rows, markers) in enumerate(bodies):
        m = np.asarray(markers, dtype=np.float64).reshape(-1, 3)
        if not 3 <= len(rows) <= MAX_MARKERS or len(rows) != m.shape[0]:
            return f"body {b}: {len(rows)} markers"
        for r in rows:
            if not 0 <= int(r) < R:
                return f"body {b}: row {r} out of range"
            if int(r) in taken:
                return f"body {b}: row {r} used twice"
            taken.add(int(r))
        if not np.isfinite(m).all():
            return f"body {b}: non-finite coordinate"
        if not rbr.posable_table(m)[-1]:
            return f"body {b}: not posable"
    return None


# ---------------------------------------------------------------------------------------------------------------------- the fit
def quat_to_R(w, x, y, z):
    """The rigid-body section's formula, its order; works on floats and on arrays."""
    return [((w * w + x * x) - y * y) - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), ((w * w - x * x) + y * y) - z * z, 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((w * w - x * x) - y * y) + z * z]


def _horn(S):
    A = [[None] * 4 for _ in range(4)]
    A[0][0] = (S[0][0] + S[1][1]) + S[2][2]
    A[1][1] = (S[0][0] - S[1][1]) - S[2][2]
    A[2][2] = (S[1][1] - S[0][0]) - S[2][2]
    A[3][3] = (S[2][2] - S[0][0]) - S[1][1]
    A[0][1] = A[1][0] = S[1][2] - S[2][1]
    A[0][2] = A[2][0] = S[2][0] - S[0][2]
    A[0][3] = A[3][0] = S[0][1] - S[1][0]
    A[1][2] = A[2][1] = S[0][1] + S[1][0]
    A[1][3] = A[3][1] = S[2][0] + S[0][2]
    A[2][3] = A[3][2] = S[1][2] + S[2][1]
    return A


def jacobi4(A):
    """Cyclic Jacobi on a symmetric 4 x 4 matrix of Python floats, in place -> V (columns = eigenvectors)."""
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for sweep in range(40):
        off = ((((abs(A[0][1]) + abs(A[0][2])) + abs(A[0][3])) + abs(A[1][2])) + abs(A[1][3])) + abs(A[2][3])
        if off == 0.0:
            break
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
            for k in range(4):
                if k != p and k != q:
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = A[p][k] = cs * akp - sn * akq
                    A[k][q] = A[q][k] = sn * akp + cs * akq
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = cs * vkp - sn * vkq
                V[k][q] = sn * vkp + cs * vkq
    return V


def pose_sample(points, model):
    """The fit of the header's stage 1 over the present markers, in ascending marker order, Python floats.
    points, model: [n][3] -> (quat [4] as computed (no sign rule), R [9], t [3], rms)."""
    P = [[float(v) for v in p] for p in points]
    Q = [[float(v) for v in q] for q in model]
    c = len(P)
    inv = 1.0 / float(c)
    qb, pb = [0.0] * 3, [0.0] * 3
    for m in range(c):
        for k in range(3):
            qb[k] = qb[k] + Q[m][k]
            pb[k] = pb[k] + P[m][k]
    qb = [v * inv for v in qb]
    pb = [v * inv for v in pb]
    S = [[0.0] * 3 for _ in range(3)]
    mq = [[Q[m][k] - qb[k] for k in range(3)] for m in range(c)]
    wp = [[P[m][k] - pb[k] for k in range(3)] for m in range(c)]
    for m in range(c):
        for i in range(3):
            for j in range(3):
                S[i][j] = S[i][j] + mq[m][i] * wp[m][j]
    A = _horn(S)
    V = jacobi4(A)
    lam, col = A[0][0], 0
    for k in range(1, 4):
        if A[k][k] > lam:
            lam, col = A[k][k], k
    w, x, y, z = V[0][col], V[1][col], V[2][col], V[3][col]
    qn = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / qn, x / qn, y / qn, z / qn
    R = quat_to_R(w, x, y, z)
    t = [pb[i] - ((R[3 * i] * qb[0] + R[3 * i + 1] * qb[1]) + R[3 * i + 2] * qb[2]) for i in range(3)]
    ss = 0.0
    for m in range(c):
        for i in range(3):
            r = ((R[3 * i] * mq[m][0] + R[3 * i + 1] * mq[m][1]) + R[3 * i + 2] * mq[m][2]) - wp[m][i]
            ss = ss + r * r
    return [w, x, y, z], R, t, math.sqrt(ss * inv)


def _jacobi4_lanes(A):
    """jacobi4 over lanes: A = 4 x 4 lists of [n] arrays, in place -> V.  A lane that has left the iteration keeps its values."""
    n = A[0][0].shape[0]
    V = [[np.ones(n) if i == j else np.zeros(n) for j in range(4)] for i in range(4)]
    active = np.ones(n, dtype=bool)
    for sweep in range(40):
        off = ((((np.abs(A[0][1]) + np.abs(A[0][2])) + np.abs(A[0][3])) + np.abs(A[1][2])) + np.abs(A[1][3])) + np.abs(A[2][3])
        active = active & ~(off == 0.0)
        if not active.any():
            break
        for p, q in PAIRS:
            apq = A[p][q]
            do = active & ~(apq == 0.0)
            g = 100.0 * np.abs(apq)
            small = do & (sweep > 3) & (np.abs(A[p][p]) + g == np.abs(A[p][p])) & (np.abs(A[q][q]) + g == np.abs(A[q][q]))
            rot = do & ~small
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            t = np.where(theta < 0.0, -t, t)
            cs = 1.0 / np.sqrt(t * t + 1.0)
            sn = t * cs
            A[p][p] = np.where(rot, A[p][p] - t * apq, A[p][p])
            A[q][q] = np.where(rot, A[q][q] + t * apq, A[q][q])
            A[p][q] = A[q][p] = np.where(do, 0.0, apq)
            for k in range(4):
                if k != p and k != q:
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = A[p][k] = np.where(rot, cs * akp - sn * akq, akp)
                    A[k][q] = A[q][k] = np.where(rot, sn * akp + cs * akq, akq)
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = np.where(rot, cs * vkp - sn * vkq, vkp)
                V[k][q] = np.where(rot, sn * vkp + cs * vkq, vkq)
    return V


def _fit_lanes(P, pm, Q):
    """The fit over lanes.  P [N][n][3] samples, pm [N][n] bool present, Q [N][3] model -> quat [n][4], R [n][9], t [n][3], rms [n]."""
    N, n = pm.shape
    cnt = pm.sum(axis=0)
    inv = 1.0 / cnt.astype(np.float64)
    qb = [np.zeros(n) for _ in range(3)]
    pb = [np.zeros(n) for _ in range(3)]
    for m in range(N):
        for k in range(3):
            qb[k] = np.where(pm[m], qb[k] + Q[m][k], qb[k])
            pb[k] = np.where(pm[m], pb[k] + P[m][:, k], pb[k])
    qb = [v * inv for v in qb]
    pb = [v * inv for v in pb]
    S = [[np.zeros(n) for _ in range(3)] for _ in range(3)]
    mq = [[Q[m][k] - qb[k] for k in range(3)] for m in range(N)]
    wp = [[P[m][:, k] - pb[k] for k in range(3)] for m in range(N)]
    for m in range(N):
        for i in range(3):
            for j in range(3):
                S[i][j] = np.where(pm[m], S[i][j] + mq[m][i] * wp[m][j], S[i][j])
    A = _horn(S)
    V = _jacobi4_lanes(A)
    lam = A[0][0]
    q4 = [V[i][0] for i in range(4)]
    for k in range(1, 4):
        up = A[k][k] > lam
        lam = np.where(up, A[k][k], lam)
        q4 = [np.where(up, V[i][k], q4[i]) for i in range(4)]
    w, x, y, z = q4
    qn = np.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / qn, x / qn, y / qn, z / qn
    R = quat_to_R(w, x, y, z)
    t = [pb[i] - ((R[3 * i] * qb[0] + R[3 * i + 1] * qb[1]) + R[3 * i + 2] * qb[2]) for i in range(3)]
    ss = np.zeros(n)
    for m in range(N):
        for i in range(3):
            r = ((R[3 * i] * mq[m][0] + R[3 * i + 1] * mq[m][1]) + R[3 * i + 2] * mq[m][2]) - wp[m][i]
            ss = np.where(pm[m], ss + r * r, ss)
    return np.stack([w, x, y, z], axis=1), np.stack(R, axis=1), np.stack(t, axis=1), np.sqrt(ss * inv)


# ---------------------------------------------------------------------------------------------------------------------- the sign rule
def _dot(u, v):
    return ((u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]) + u[3] * v[3]


def _first_bit(q):
    for v in q:
        if v != 0.0:
            return 1 if v < 0.0 else 0
    return 0


def sign_walk(quat, posed):
    """The header's walk over one body: quat [F][4] as computed, posed [F] bool -> s [F] (1 = negated; 0 where not POSED).
    d is taken against the previous POSED frame's OUTPUT quaternion."""
    s = np.zeros(len(quat), dtype=np.int32)
    prev_out, state = None, 0
    for f in range(len(quat)):
        if not posed[f]:
            continue
        q = [float(v) for v in quat[f]]
        if prev_out is None:
            state = _first_bit(q)
        else:
            d = _dot(prev_out, q)
            if d < 0.0:
                state = 1
            elif d > 0.0:
                state = 0
        s[f] = state
        prev_out = [-v for v in q] if state else q
    return s


def sign_parity(quat, posed):
    """The same as a prefix parity: the flip [d_raw < 0] between consecutive computed quaternions (the first frame's own bit), XORed
    along the POSED frames."""
    idx = np.flatnonzero(posed)
    s = np.zeros(len(quat), dtype=np.int32)
    if idx.size == 0:
        return s
    flips = np.zeros(idx.size, dtype=np.int32)
    flips[0] = _first_bit([float(v) for v in quat[idx[0]]])
    for i in range(1, idx.size):
        d = _dot([float(v) for v in quat[idx[i - 1]]], [float(v) for v in quat[idx[i]]])
        flips[i] = 1 if d < 0.0 else 0
    s[idx] = np.bitwise_xor.accumulate(flips)
    return s


# ---------------------------------------------------------------------------------------------------------------------- stage 1
def pose_rows(traj, bodies, max_rms, raw=False):
    """raw = True also returns "quat_raw": the quaternions before the sign rule."""
    traj = np.asarray(traj, dtype=np.float64)
    _, F, _ = traj.shape
    B = len(bodies)
    out = {"n_used": np.zeros((B, F), dtype=np.int32), "present": np.zeros((B, F), dtype=np.int32),
           "flag": np.zeros((B, F), dtype=np.int32), "quat": np.full((B, F, 4), np.nan), "R": np.full((B, F, 3, 3), np.nan),
           "t_pose": np.full((B, F, 3), np.nan), "rms": np.full((B, F), np.nan)}
    quat_raw = np.full((B, F, 4), np.nan)
    for b, (rows, markers) in enumerate(bodies):
        Q = np.asarray(markers, dtype=np.float64).reshape(-1, 3)
        N = Q.shape[0]
        table = np.array(rbr.posable_table(Q))
        P = traj[np.asarray(rows, dtype=np.int64)]                     # [N][F][3]
        pm = np.isfinite(P).all(axis=2)                                # [N][F]
        present = (pm.astype(np.int64) << np.arange(N)[:, None]).sum(axis=0)
        cnt = pm.sum(axis=0)
        few = cnt < 3
        degenerate = ~few & ~table[present]
        fit = np.flatnonzero(~few & ~degenerate)
        flag = np.where(few, FEW, DEGENERATE).astype(np.int32)
        if fit.size:
            with np.errstate(all="ignore"):
                q4, Rm, t, rms = _fit_lanes(P[:, fit], pm[:, fit], Q)
                over = rms > max_rms
            flag[fit] = np.where(over, RMS, POSED)
            out["rms"][b, fit] = rms
            ok = fit[~over]
            quat_raw[b, ok] = q4[~over]
            out["R"][b, ok] = Rm[~over].reshape(-1, 3, 3)
            out["t_pose"][b, ok] = t[~over]
        out["n_used"][b], out["present"][b], out["flag"][b] = cnt, present, flag
        s = sign_walk(quat_raw[b], flag == POSED)
        out["quat"][b] = np.where(s[:, None] == 1, -quat_raw[b], quat_raw[b])
    if raw:
        out["quat_raw"] = quat_raw
    return out


# ---------------------------------------------------------------------------------------------------------------------- stage 2
def present4(t, quat):
    return tsr.good_times(t)[None, :] & np.isfinite(np.asarray(quat, dtype=np.float64)).all(axis=2)


def smooth_rotations(t, quat, degree, W, span, n_min, max_gap, coeffs=False):
    """tests/track_smooth_reference.py's smooth() with four coordinates, and the header's tail: n2, quat_s, omega, res."""
    d = degree
    t = np.asarray(t, dtype=np.float64)
    quat = np.asarray(quat, dtype=np.float64)
    R, F, _ = quat.shape
    good = tsr.good_times(t)
    pres = present4(t, quat)
    tp = np.concatenate([np.zeros(W), t, np.zeros(W)])
    pp = np.concatenate([np.zeros((R, W), dtype=bool), pres, np.zeros((R, W), dtype=bool)], axis=1)
    xp = np.concatenate([np.zeros((R, W, 4)), np.where(pres[:, :, None], quat, 0.0), np.zeros((R, W, 4))], axis=1)
    tf = np.where(good, t, 0.0)
    offs = range(-W, W + 1)

    def at(j):
        sl = slice(W + j, W + j + F)
        s = np.broadcast_to(tp[sl] - tf, (R, F))
        p = pp[:, sl] & good[None, :]
        return p, s, p & (np.abs(s) <= span), xp[:, sl]

    with np.errstate(all="ignore"):
        n = np.zeros((R, F), dtype=np.int32)
        h = np.zeros((R, F))
        ja = np.zeros((R, F), dtype=np.int32)
        jb = np.zeros((R, F), dtype=np.int32)
        sa = np.zeros((R, F), dtype=bool)
        sb = np.zeros((R, F), dtype=bool)
        for j in offs:
            p, s, ins, _ = at(j)
            n += ins
            h = np.where(ins & (np.abs(s) > h), np.abs(s), h)
            if j < 0:
                ja, sa = np.where(p, j, ja), np.where(p, ins, sa)
            elif j > 0:
                first = p & (jb == 0)
                jb, sb = np.where(first, j, jb), np.where(first, ins, sb)
        fillable = ~pres & good[None, :] & (max_gap > 0) & (ja != 0) & (jb != 0) & (jb - ja - 1 <= max_gap) & sa & sb
        due = good[None, :] & (pres | fillable) & (n >= n_min)

        S = [np.zeros((R, F)) for _ in range(2 * d + 1)]
        Bs = [[np.zeros((R, F)) for _ in range(4)] for _ in range(d + 1)]
        for j in offs:
            _, s, ins, x = at(j)
            u = s / h
            p = np.ones((R, F))
            for i in range(2 * d + 1):
                S[i] = np.where(ins, S[i] + p, S[i])
                if i <= d:
                    for k in range(4):
                        Bs[i][k] = np.where(ins, Bs[i][k] + p * x[:, :, k], Bs[i][k])
                p = p * u
        L = [[None] * (d + 1) for _ in range(d + 1)]
        ok = np.ones((R, F), dtype=bool)
        for i in range(d + 1):
            for j in range(i + 1):
                s = S[i + j]
                for k in range(j):
                    s = s - L[i][k] * L[j][k]
                if j == i:
                    ok &= (s > 0.0) & (s < np.inf)
                    L[i][i] = np.sqrt(s)
                else:
                    L[i][j] = s / L[j][j]
        c = [[None] * 4 for _ in range(d + 1)]
        for k in range(4):
            y = [None] * (d + 1)
            for i in range(d + 1):
                s = Bs[i][k]
                for m in range(i):
                    s = s - L[i][m] * y[m]
                y[i] = s / L[i][i]
            for i in range(d, -1, -1):
                s = y[i]
                for m in range(i + 1, d + 1):
                    s = s - L[m][i] * c[m][k]
                c[i][k] = s / L[i][i]
        pw, px, py, pz = c[0]
        n2 = ((pw * pw + px * px) + py * py) + pz * pz
        ok2 = (n2 > 0.0) & (n2 < np.inf)
        ss = np.zeros((R, F))
        for j in offs:
            _, s, ins, x = at(j)
            u = s / h
            for k in range(4):
                q = c[d][k]
                for i in range(d - 1, -1, -1):
                    q = q * u + c[i][k]
                e = x[:, :, k] - q
                ss = np.where(ins, ss + e * e, ss)
        fit = due & ok & ok2
        nan = np.full((R, F), np.nan)
        nq = np.sqrt(n2)
        dw, dx, dy, dz = (c[1][k] / h for k in range(4))
        om = [(2.0 * ((pw * dx - dw * px) - (dy * pz - dz * py))) / n2,
              (2.0 * ((pw * dy - dw * py) - (dz * px - dx * pz))) / n2,
              (2.0 * ((pw * dz - dw * pz) - (dx * py - dy * px))) / n2]
        quat_s = np.stack([np.where(fit, c[0][k] / nq, nan) for k in range(4)], axis=2)
        omega = np.stack([np.where(fit, om[k], nan) for k in range(3)], axis=2)
        res = np.where(fit, np.sqrt(ss / (4 * n).astype(np.float64)), nan)
    flag = np.where(~good[None, :], tsr.BAD_TIME,
                    np.where(~(pres | fillable), 0,
                             np.where(n < n_min, tsr.FEW,
                                      np.where(~(ok & ok2), tsr.SINGULAR, np.where(pres, tsr.SMOOTHED, tsr.FILLED))))).astype(np.int32)
    n_used = np.where(good[None, :], n, 0).astype(np.int32)
    out = {"quat_s": quat_s, "omega": omega, "res": res, "n_used": n_used, "flag": flag}
    if coeffs:
        out["c0"] = np.stack(c[0], axis=2)
    return out


def smooth_rotations_mp(t, quat, degree, W, span, n_min, max_gap, ref, where):
    """quat_s and omega of the (b, f) in `where` that the float64 statement fitted, in 50 digits from the same doubles (the normal
    equations solved exactly enough to call it exact) -> {"quat_s", "omega"} float64, NaN elsewhere."""
    import mpmath
    d = degree
    t = np.asarray(t, dtype=np.float64)
    quat = np.asarray(quat, dtype=np.float64)
    B, F, _ = quat.shape
    pres = present4(t, quat)
    out = {"quat_s": np.full((B, F, 4), np.nan), "omega": np.full((B, F, 3), np.nan)}
    with mpmath.mp.workdps(50):
        for b in range(B):
            for f in range(F):
                if not where[b, f] or ref["flag"][b, f] not in (tsr.SMOOTHED, tsr.FILLED):
                    continue
                gs = [g for g, _, ok in tsr.window(t, pres[b], f, W, span) if ok]
                s = [mpmath.mpf(float(t[g])) - mpmath.mpf(float(t[f])) for g in gs]
                h = max(abs(v) for v in s)
                u = [v / h for v in s]
                A = mpmath.matrix(d + 1, d + 1)
                for i in range(d + 1):
                    for j in range(d + 1):
                        A[i, j] = mpmath.fsum(v ** (i + j) for v in u)
                p, dp = [], []
                for k in range(4):
                    x = [mpmath.mpf(float(quat[b, g, k])) for g in gs]
                    rhs = mpmath.matrix([mpmath.fsum(v ** i * xv for v, xv in zip(u, x)) for i in range(d + 1)])
                    c = mpmath.lu_solve(A, rhs)
                    p.append(c[0])
                    dp.append(c[1] / h)
                n2 = sum(v * v for v in p)
                nq = mpmath.sqrt(n2)
                out["quat_s"][b, f] = [float(v / nq) for v in p]
                pw, px, py, pz = p
                dw, dx, dy, dz = dp
                out["omega"][b, f] = [float(2 * ((pw * dx - dw * px) - (dy * pz - dz * py)) / n2),
                                      float(2 * ((pw * dy - dw * py) - (dz * px - dx * pz)) / n2),
                                      float(2 * ((pw * dz - dw * pz) - (dx * py - dy * px)) / n2)]
    return out


# ---------------------------------------------------------------------------------------------------------------------- stage 3
def fill_rows(traj, bodies, flag, Rm, t_pose, flag_s=None, quat_s=None, pos_s=None):
    traj = np.asarray(traj, dtype=np.float64)
    R, F, _ = traj.shape
    Rm = np.asarray(Rm, dtype=np.float64).reshape(len(bodies), F, 9)
    filled = np.full((R, F, 3), np.nan)
    src = np.zeros((R, F), dtype=np.int32)
    measured = np.isfinite(traj).all(axis=2)
    filled[measured] = traj[measured]
    src[measured] = SRC_MEASURED
    with np.errstate(all="ignore"):
        for b, (rows, markers) in enumerate(bodies):
            Q = np.asarray(markers, dtype=np.float64).reshape(-1, 3)
            for m, r in enumerate(rows):
                q = Q[m]
                rigid = ~measured[r] & (flag[b] == POSED)
                for i in range(3):
                    x = ((Rm[b, :, 3 * i] * q[0] + Rm[b, :, 3 * i + 1] * q[1]) + Rm[b, :, 3 * i + 2] * q[2]) + t_pose[b, :, i]
                    filled[r, :, i] = np.where(rigid, x, filled[r, :, i])
                src[r] = np.where(rigid, SRC_RIGID, src[r])
                if flag_s is not None:
                    smoothed = ~measured[r] & ~rigid & (flag_s[b] == tsr.FILLED)
                    Rs = quat_to_R(*[quat_s[b, :, k] for k in range(4)])
                    for i in range(3):
                        x = ((Rs[3 * i] * q[0] + Rs[3 * i + 1] * q[1]) + Rs[3 * i + 2] * q[2]) + pos_s[b, :, i]
                        filled[r, :, i] = np.where(smoothed, x, filled[r, :, i])
                    src[r] = np.where(smoothed, SRC_RIGID_FILLED, src[r])
    return {"filled": filled, "src": src}


# ---------------------------------------------------------------------------------------------------------------------- scenes
def make_session(seed, F, n_markers, n_loose=1, sigma=0.0005, dropout=0.10, rate=120.0, amplitude=1.0, jitter=0.2):
    """A labelled session: bodies of n_markers[b] markers under seeded rigid motions (rigid_groups_reference), rows in body order,
    then n_loose rows of no body; `sigma` of noise, a fraction `dropout` of the samples NaN.
    -> t [F], traj [R][F][3], bodies [(rows, template)], truth {"R": [B][F][3][3], "c": [B][F][3], "rows": [R][F][3] noise-free}."""
    rng = np.random.default_rng(seed)
    t = 2.0 + np.cumsum((1.0 + jitter * rng.uniform(-1.0, 1.0, F)) / rate)
    tau = t - t[0]
    rows, bodies, Rs, cs = [], [], [], []
    for N in n_markers:
        while True:
            q = template(rng, N)
            if rbr.posable_table(q)[-1]:
                break
        Rm, c = rigid_motion(rng, tau, amplitude)
        bodies.append((list(range(len(rows), len(rows) + N)), q))
        for m in range(N):
            rows.append(np.einsum("fij,j->fi", Rm, q[m]) + c)
        Rs.append(Rm)
        cs.append(c)
    for _ in range(n_loose):
        rows.append(rigid_motion(rng, tau, amplitude)[1])
    clean = np.array(rows)
    traj = clean + sigma * rng.standard_normal(clean.shape)
    traj[rng.uniform(size=traj.shape[:2]) < dropout] = np.nan
    return t, traj, bodies, {"R": np.array(Rs), "c": np.array(cs), "rows": clean}
