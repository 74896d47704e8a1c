"""The "trajectories" contract of include/mocap_core.h in plain Python and NumPy, in the scalar order the header writes.

    gather(xyz, n_pts, ids, relabel, R, hits=None, min_hits=0) -> traj [R][F][3]
    smooth(t, traj, degree, W, span, n_min, max_gap)           -> {"pos", "vel", "acc", "res", "n_used", "flag"}
    smooth_sample(t, traj, r, f, ...)                           one (r, f) of the same in Python floats, one rounding per operation
    smooth_mp(t, traj, ..., ref=None)                           the same fit evaluated in 50 digits (mpmath); the discrete decisions
                                                                (good times, samples, flags) are those of the float64 statement

smooth() is vectorised over (row, frame) only: every element goes through the operations of smooth_sample in the same order (NumPy's
elementwise +, -, *, /, sqrt are IEEE double, one rounding each, never fused), the window is walked in ascending g by a Python loop
and a sample that does not take part leaves the sums as they are (np.where, not a product with 0).  The two are compared bit for bit
in tests/test_track_smooth_reference_cpu.py; the device is compared with smooth().
"""
import math

import numpy as np

SMOOTHED, FILLED, FEW, SINGULAR, BAD_TIME = 1, 2, 4, 8, 16
INF = float("inf")
NAN = float("nan")
FIELDS = ("pos", "vel", "acc", "res")


# ---------------------------------------------------------------------------------------------------------------------- gather
def gather(xyz, n_pts, ids, relabel, R, hits=None, min_hits=0):
    xyz = np.asarray(xyz, dtype=np.float64)
    F, K_max, _ = xyz.shape
    relabel = np.asarray(relabel)
    traj = np.full((R, F, 3), np.nan)
    for f in range(F):
        n = int(n_pts[f])
        if n < 0 or n > K_max:
            n = 0
        taken = set()
        for j in range(n):
            i = int(ids[f][j])
            if i < 0 or i >= relabel.size:
                continue
            r = int(relabel[i])
            if r < 0 or r >= R or r in taken:
                continue
            if hits is not None and int(hits[f][j]) < min_hits:
                continue
            if not np.isfinite(xyz[f, j]).all():
                continue
            traj[r, f] = xyz[f, j]
            taken.add(r)
    return traj


# ---------------------------------------------------------------------------------------------------------------------- smooth
def good_times(t):
    """[F] bool: t_f finite and above every finite t before it."""
    t = np.asarray(t, dtype=np.float64)
    fin = np.isfinite(t)
    low = np.where(fin, t, -np.inf)
    before = np.concatenate([[-np.inf], np.maximum.accumulate(low)[:-1]])
    return fin & (low > before)


def present_mask(t, traj):
    return good_times(t)[None, :] & np.isfinite(np.asarray(traj, dtype=np.float64)).all(axis=2)


def window(t, present_row, f, W, span):
    """The frames of the window of f that are present, each with "is a sample": [(g, s_g, in)] in ascending g."""
    out = []
    for g in range(max(f - W, 0), min(f + W, len(t) - 1) + 1):
        if present_row[g]:
            s = float(t[g]) - float(t[f])
            out.append((g, s, abs(s) <= span))
    return out


def decide(t, good, present_row, f, W, span, n_min, max_gap):
    """-> (flag or None when a fit is due, n, samples [(g, s_g)], is_present)."""
    if not good[f]:
        return BAD_TIME, 0, [], False
    win = window(t, present_row, f, W, span)
    samples = [(g, s) for g, s, ok in win if ok]
    n = len(samples)
    below = [(g, ok) for g, _, ok in win if g < f]
    above = [(g, ok) for g, _, ok in win if g > f]
    present = bool(present_row[f])
    fillable = (not present and max_gap > 0 and bool(below) and bool(above) and above[0][0] - below[-1][0] - 1 <= max_gap
                and below[-1][1] and above[0][1])
    if not present and not fillable:
        return 0, n, samples, present
    if n < n_min:
        return FEW, n, samples, present
    return None, n, samples, present


def smooth_sample(t, traj, r, f, degree, W, span, n_min, max_gap, good=None, present=None):
    """One (r, f) in Python floats -> (pos [3], vel [3], acc [3], res, n_used, flag)."""
    d = degree
    good = good_times(t) if good is None else good
    present = present_mask(t, traj) if present is None else present
    nan3 = [NAN, NAN, NAN]
    flag, n, samples, is_present = decide(t, good, present[r], f, W, span, n_min, max_gap)
    if flag is not None:
        return nan3, nan3, nan3, NAN, n, flag
    h = 0.0
    for _, s in samples:
        h = abs(s) if abs(s) > h else h
    S = [0.0] * (2 * d + 1)
    B = [[0.0, 0.0, 0.0] for _ in range(d + 1)]
    for g, s in samples:
        u = s / h                      # h > 0: n >= 2 and good times differ (inf / inf is NaN in Python too)
        x =[float(v) for v in traj[r][g]]
        p = 1.0
        for i in range(2 * d + 1):
            S[i] = S[i] + p
            if i <= d:
                for k in range(3):
                    B[i][k] = B[i][k] + p * x[k]
            p = p * u
    L = [[0.0] * (d + 1) for _ in range(d + 1)]
    ok = True
    for i in range(d + 1):
        for j in range(i + 1):
            s = S[i + j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            if j == i:
                if not (s > 0.0 and s < INF):
                    ok = False
                L[i][i] = math.sqrt(s) if s >= 0.0 else NAN
            else:
                L[i][j] = _div(s, L[j][j])
    if not ok:
        return nan3, nan3, nan3, NAN, n, SINGULAR
    c = [[0.0, 0.0, 0.0] for _ in range(d + 1)]
    for k in range(3):
        y = [0.0] * (d + 1)
        for i in range(d + 1):
            s = B[i][k]
            for m in range(i):
                s = s - L[i][m] * y[m]
            y[i] = s / L[i][i]
        for i in range(d, -1, -1):
            s = y[i]
            for m in range(i + 1, d + 1):
                s = s - L[m][i] * c[m][k]
            c[i][k] = s / L[i][i]
    ss = 0.0
    for g, s in samples:
        u = s / h
        for k in range(3):
            q = c[d][k]
            for i in range(d - 1, -1, -1):
                q = q * u + c[i][k]
            e = float(traj[r][g][k]) - q
            ss = ss + e * e
    pos = [c[0][k] for k in range(3)]
    vel = [c[1][k] / h for k in range(3)]
    acc = [((2.0 * c[2][k]) / h) / h for k in range(3)] if d >= 2 else nan3
    return pos, vel, acc, math.sqrt(ss / float(3 * n)), n, SMOOTHED if is_present else FILLED


def _div(a, b):
    """IEEE a / b where Python would raise or where an operand is not finite."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def smooth(t, traj, degree, W, span, n_min, max_gap):
    d = degree
    t = np.asarray(t, dtype=np.float64)
    traj = np.asarray(traj, dtype=np.float64)
    R, F, _ = traj.shape
    good = good_times(t)
    pres = present_mask(t, traj)
    tp = np.concatenate([np.zeros(W), t, np.zeros(W)])
    pp = np.concatenate([np.zeros((R, W), dtype=bool), pres, np.zeros((R, W), dtype=bool)], axis=1)
    xp = np.concatenate([np.zeros((R, W, 3)), np.where(pres[:, :, None], traj, 0.0), np.zeros((R, W, 3))], axis=1)
    tf = np.where(good, t, 0.0)
    offs = range(-W, W + 1)

    def at(j):
        """(present, s_g, is a sample) of the frames f + j, each [R][F] or broadcastable"""
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
        B = [[np.zeros((R, F)) for _ in range(3)] for _ in range(d + 1)]
        for j in offs:
            _, s, ins, x = at(j)
            u = s / h
            p = np.ones((R, F))
            for i in range(2 * d + 1):
                S[i] = np.where(ins, S[i] + p, S[i])
                if i <= d:
                    for k in range(3):
                        B[i][k] = np.where(ins, B[i][k] + p * x[:, :, k], B[i][k])
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
        c = [[None] * 3 for _ in range(d + 1)]
        for k in range(3):
            y = [None] * (d + 1)
            for i in range(d + 1):
                s = B[i][k]
                for m in range(i):
                    s = s - L[i][m] * y[m]
                y[i] = s / L[i][i]
            for i in range(d, -1, -1):
                s = y[i]
                for m in range(i + 1, d + 1):
                    s = s - L[m][i] * c[m][k]
                c[i][k] = s / L[i][i]
        ss = np.zeros((R, F))
        for j in offs:
            _, s, ins, x = at(j)
            u = s / h
            for k in range(3):
                q = c[d][k]
                for i in range(d - 1, -1, -1):
                    q = q * u + c[i][k]
                e = x[:, :, k] - q
                ss = np.where(ins, ss + e * e, ss)
        fit = due & ok
        nan = np.full((R, F), np.nan)
        pos = np.stack([np.where(fit, c[0][k], nan) for k in range(3)], axis=2)
        vel = np.stack([np.where(fit, c[1][k] / h, nan) for k in range(3)], axis=2)
        acc = np.stack([np.where(fit, ((2.0 * c[2][k]) / h) / h, nan) if d >= 2 else nan for k in range(3)], axis=2)
        res = np.where(fit, np.sqrt(ss / (3 * n).astype(np.float64)), nan)
    flag = np.where(~good[None, :], BAD_TIME,
                    np.where(~(pres | fillable), 0,
                             np.where(n < n_min, FEW, np.where(~ok, SINGULAR, np.where(pres, SMOOTHED, FILLED))))).astype(np.int32)
    n_used = np.where(good[None, :], n, 0).astype(np.int32)
    return {"pos": pos, "vel": vel, "acc": acc, "res": res, "n_used": n_used, "flag": flag}


# ---------------------------------------------------------------------------------------------------------------------- 50 digits
def smooth_mp(t, traj, degree, W, span, n_min, max_gap, ref=None, where=None):
    """The fit of every (r, f) the float64 statement fitted (flag SMOOTHED or FILLED; `where` [R][F] bool narrows it), evaluated in
    50 digits from the same doubles: s_g = t_g - t_f exactly, the normal equations solved exactly enough to call it exact.
    -> {"pos", "vel", "acc", "res"} as float64 arrays, NaN elsewhere, plus "scale" [R][F]: max |x_g[k]| over the samples and
    "h" [R][F], "cond" [R][F] the 2-norm condition number of the Gram matrix in u (float64, numpy.linalg.cond)."""
    import mpmath
    mp = mpmath.mp
    d = degree
    t = np.asarray(t, dtype=np.float64)
    traj = np.asarray(traj, dtype=np.float64)
    R, F, _ = traj.shape
    ref = smooth(t, traj, degree, W, span, n_min, max_gap) if ref is None else ref
    good, pres = good_times(t), present_mask(t, traj)
    out = {k: np.full((R, F, 3), np.nan) for k in ("pos", "vel", "acc")}
    out.update({k: np.full((R, F), np.nan) for k in ("res", "scale", "h", "cond")})
    with mp.workdps(50):
        for r in range(R):
            for f in range(F):
                if ref["flag"][r, f] not in (SMOOTHED, FILLED) or (where is not None and not where[r, f]):
                    continue
                gs = [g for g, _, ok in window(t, pres[r], f, W, span) if ok]
                s = [mpmath.mpf(float(t[g])) - mpmath.mpf(float(t[f])) for g in gs]
                h = max(abs(v) for v in s)
                u = [v / h for v in s]
                A = mpmath.matrix(d + 1, d + 1)
                for i in range(d + 1):
                    for j in range(d + 1):
                        A[i, j] = mpmath.fsum(v ** (i + j) for v in u)
                ss = mpmath.mpf(0)
                for k in range(3):
                    x = [mpmath.mpf(float(traj[r, g, k])) for g in gs]
                    b = mpmath.matrix([mpmath.fsum(v ** i * xv for v, xv in zip(u, x)) for i in range(d + 1)])
                    c = mpmath.lu_solve(A, b)
                    out["pos"][r, f, k] = float(c[0])
                    out["vel"][r, f, k] = float(c[1] / h)
                    if d >= 2:
                        out["acc"][r, f, k] = float(2 * c[2] / h / h)
                    ss += mpmath.fsum((xv - mpmath.polyval([c[i] for i in range(d, -1, -1)], v)) ** 2 for v, xv in zip(u, x))
                out["res"][r, f] = float(mpmath.sqrt(ss / (3 * len(gs))))
                out["scale"][r, f] = float(np.abs(traj[r, gs]).max())
                out["h"][r, f] = float(h)
                uf = np.array([float(v) for v in u])
                out["cond"][r, f] = np.linalg.cond(np.array([[np.sum(uf ** (i + j)) for j in range(d + 1)] for i in range(d + 1)]))
    return out


def scaled_errors(got, exact, degree):
    """The largest error of pos, vel and acc, each relative to the natural size of that quantity in its window: X = max |x_g[k]| over
    the samples for pos, X / h for vel, X / h^2 for acc (h = the window's largest |t_g - t_f|)."""
    m = np.isfinite(exact["res"])
    X, h = exact["scale"][m][:, None], exact["h"][m][:, None]
    errs = {"pos": (np.abs(got["pos"][m] - exact["pos"][m]) / X).max(), "vel": (np.abs(got["vel"][m] - exact["vel"][m]) * h / X).max()}
    if degree >= 2:
        errs["acc"] = (np.abs(got["acc"][m] - exact["acc"][m]) * h * h / X).max()
    return {k: float(v) for k, v in errs.items()}


# ---------------------------------------------------------------------------------------------------------------------- sessions
def make_session(seed, F, R, rate=120.0, jitter=0.3, noise=0.0005, dropout=0.08, max_run=6):
    """A synthetic session: irregular increasing t [F], truth [R][F][3] (sums of sines inside a 3 m room), traj = truth + noise with
    runs of 1 .. max_run missing frames (NaN) starting at a fraction `dropout` of the frames."""
    rng = np.random.default_rng(seed)
    t = 5.0 + np.cumsum((1.0 + jitter * rng.uniform(-1.0, 1.0, F)) / rate)
    w = rng.uniform(0.5, 6.0, (R, 3, 3))
    ph = rng.uniform(0.0, 2.0 * np.pi, (R, 3, 3))
    amp = rng.uniform(0.05, 0.4, (R, 3, 3))
    truth = rng.uniform(-1.0, 1.0, (R, 1, 3)) + (amp[:, None] * np.sin(w[:, None] * t[None, :, None, None] + ph[:, None])).sum(axis=3)
    traj = truth + noise * rng.standard_normal((R, F, 3))
    for r in range(R):
        for f in np.nonzero(rng.uniform(size=F) < dropout)[0]:
            traj[r, f:f + int(rng.integers(1, max_run + 1))] = np.nan
    return t, truth, traj


def same_bits(a, b):
    """Equal bit for bit, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
