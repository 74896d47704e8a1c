"""The "joint bundle adjustment" section of include/mocap_core.h as plain Python / NumPy: linearisation, Schur complement,
Levenberg-Marquardt loop, Huber weights, gauge.  One text for three kinds of number:

  FLOAT   NumPy doubles: the reference the solver tests run (its sums are NumPy's, not the device's tree: equal to rounding).
  MP      mpmath at 50 digits: every per-view formula (residual, Huber weight, the rows of A and B, rho).
  FIXED   Python integers scaled by 2^200 (60 digits): the per-point algebra behind the views (V, its Cholesky factor, E, z, U, the
          Gram sums).  mpmath's own numbers are integers times a power of two; taking the sums on integers keeps them exact and
          three orders of magnitude faster than mpf objects (16 cameras x 1 031 points: 38 million multiply-adds in sum E^T E, done
          as exact float64 products of 20-bit limbs).  tests/test_ba_joint_reference_cpu.py checks FIXED against MP run end to end.

linearise_mp = MP views -> FIXED algebra -> mpmath numbers: the 50-digit S, rhs and cost the device is compared with."""
import math
from fractions import Fraction

import mpmath
import numpy as np

DPS = 50
Q = 200                      # fixed point: value * 2^Q
MAX_CAMERAS, MAX_POINTS = 16, 131072
ST_CAMERA_UNSEEN, ST_NO_POINTS, ST_SINGULAR, ST_POINT_SINGULAR, ST_LAMBDA, ST_MAX_ITER, ST_BAD_DEPTH = 1, 2, 4, 8, 16, 32, 64


# ----------------------------------------------------------------------------------------------------------------- number kinds
class FLOAT:
    name = "float"
    mul = staticmethod(lambda a, b: a * b)
    div = staticmethod(lambda a, b: a / b)
    sqrt = staticmethod(np.sqrt)
    lift = staticmethod(lambda a: np.asarray(a, dtype=np.float64))
    zeros = staticmethod(lambda shape: np.zeros(shape))
    one = 1.0


class MP:
    name = "mp"
    mul = staticmethod(lambda a, b: a * b)
    div = staticmethod(lambda a, b: a / b)
    sqrt = staticmethod(np.frompyfunc(mpmath.sqrt, 1, 1))
    _lift = np.frompyfunc(mpmath.mpf, 1, 1)
    lift = staticmethod(lambda a: MP._lift(np.asarray(a, dtype=object)))
    one = mpmath.mpf(1)

    @staticmethod
    def zeros(shape):
        z = np.empty(shape, dtype=object)
        z.fill(mpmath.mpf(0))
        return z


class FIXED:
    name = "fixed"
    mul = staticmethod(lambda a, b: (a * b) >> Q)
    div = staticmethod(lambda a, b: (a << Q) // b)
    sqrt = staticmethod(np.frompyfunc(lambda v: math.isqrt(v << Q) if v > 0 else 0, 1, 1))
    one = 1 << Q

    @staticmethod
    def zeros(shape):
        z = np.empty(shape, dtype=object)
        z.fill(0)
        return z

    @staticmethod
    def from_float(x):       # exact
        return int(Fraction(float(x)) * (1 << Q))

    from_mp = staticmethod(np.frompyfunc(lambda v: int(mpmath.floor(mpmath.ldexp(v, Q))), 1, 1))
    to_mp = staticmethod(np.frompyfunc(lambda v: mpmath.ldexp(mpmath.mpf(v), -Q), 1, 1))


def n_cam_params(C, focal):
    return 6 * (C - 1) + (C if focal else 0)


def plain_K(K):
    K = np.asarray(K, dtype=np.float64).reshape(-1, 3, 3)
    return bool(np.all(K[:, 0, 1] == 0) and np.all(K[:, 1, 0] == 0) and np.all(K[:, 2, 0] == 0) and np.all(K[:, 2, 1] == 0) and
                np.all(K[:, 2, 2] == 1))


def check_args(C, N, K, focal, huber_px=0.0, ftol=0.0, max_iter=1, lam=0.0):
    """The MOCAP_E_ARG rules: None when the call is taken, else the reason."""
    if not 2 <= C <= MAX_CAMERAS:
        return "cameras"
    if not 1 <= N <= MAX_POINTS:
        return "points"
    if not plain_K(K):
        return "K is not plain"
    if focal and C < 3:
        return "focal needs 3 cameras"
    for v in (huber_px, ftol, lam):
        if not (np.isfinite(v) and v >= 0):
            return "negative or non-finite"
    if max_iter < 1:
        return "max_iter"
    return None


def participating(obs, X):
    """>= 2 views, all of them finite, and a finite position."""
    obs = np.asarray(obs, dtype=np.float64)
    seen = ~np.isnan(obs).any(axis=2)
    fin = np.where(seen, np.isfinite(obs).all(axis=2), True).all(axis=1)
    return (seen.sum(axis=1) >= 2) & fin & np.isfinite(np.asarray(X, dtype=np.float64)).all(axis=1), seen


# ---------------------------------------------------------------------------------------------------------------------- views
def view_terms(F, R, t, fx, fy, cx, cy, X, u, v, huber):
    """One camera's view of the points X (three arrays over the points, numbers of kind F), in the header's order.  Returns a dict
    of arrays; nothing is masked here except the division by a depth that is not > 0."""
    P = [(X[0] * R[i][0] + X[1] * R[i][1]) + X[2] * R[i][2] for i in range(3)]
    Y = [P[i] + t[i] for i in range(3)]
    pos = (Y[2] > 0).astype(bool)
    if F is FLOAT:
        pos &= np.isfinite(Y[2])
    Y2 = np.where(pos, Y[2], F.one)
    xn, yn = Y[0] / Y2, Y[1] / Y2
    ru, rv = (xn * fx + cx) - u, (yn * fy + cy) - v
    s2 = ru * ru + rv * rv
    s = F.sqrt(s2)
    if huber > 0:
        down = (s > huber).astype(bool)
        ss = np.where(down, s, F.one)
        w = np.where(down, huber / ss, F.one)
        rho = np.where(down, s * (2.0 * huber) - huber * huber, s2)
    else:
        down = np.zeros(len(s), dtype=bool)
        w = np.where(down, F.one, F.one)
        rho = s2
    sw = F.sqrt(w)
    du0, dv1 = sw * (fx / Y2), sw * (fy / Y2)
    du2, dv2 = -(du0 * xn), -(dv1 * yn)
    Bu = [du0 * R[0][j] + du2 * R[2][j] for j in range(3)]
    Bv = [dv1 * R[1][j] + dv2 * R[2][j] for j in range(3)]
    zero = du0 * 0
    Au = [du2 * P[1], du0 * P[2] - du2 * P[0], -(du0 * P[1]), du0, zero, du2, sw * (xn * fx)]
    Av = [dv2 * P[1] - dv1 * P[2], -(dv2 * P[0]), dv1 * P[0], zero, dv1, dv2, sw * (yn * fy)]
    return {"pos": pos, "down": down, "rho": rho, "ru": sw * ru, "rv": sw * rv, "Bu": Bu, "Bv": Bv, "Au": Au, "Av": Av}


def view_stage(F, obs, R, t, K, fscale, X, huber):
    """Every view of every point: arrays [C][...][N] of kind F, zero where the view is not used."""
    obs = np.asarray(obs, dtype=np.float64)
    N, C = obs.shape[:2]
    part, seen = participating(obs, X)
    seen = seen & part[:, None]
    Xs = np.where(part[:, None], np.asarray(X, dtype=np.float64), 0.0)
    Xl = [F.lift(Xs[:, k]) for k in range(3)]
    out = {"part": part, "seen": seen, "used": np.zeros((C, N), bool), "down": np.zeros((C, N), bool), "views": []}
    s = np.ones(C) if fscale is None else np.asarray(fscale, dtype=np.float64)
    lift1 = (lambda x: float(x)) if F is FLOAT else (lambda x: mpmath.mpf(float(x)))
    for c in range(C):
        o = np.where(seen[:, c, None], obs[:, c], 0.0)
        Rc = [[lift1(R[c][i][j]) for j in range(3)] for i in range(3)]
        tcam = [lift1(t[c][i]) for i in range(3)]
        fx, fy = lift1(K[c][0][0]) * lift1(s[c]), lift1(K[c][1][1]) * lift1(s[c])
        v = view_terms(F, Rc, tcam, fx, fy, lift1(K[c][0][2]), lift1(K[c][1][2]), Xl, F.lift(o[:, 0]), F.lift(o[:, 1]), huber)
        used = seen[:, c] & v["pos"]
        z = F.zeros(N)

        def m(a):
            return np.where(used, a, z)
        out["used"][c] = used
        out["down"][c] = used & v["down"]
        out["views"].append({"rho": m(v["rho"]), "ru": m(v["ru"]), "rv": m(v["rv"]), "Bu": [m(a) for a in v["Bu"]],
                             "Bv": [m(a) for a in v["Bv"]], "Au": [m(a) for a in v["Au"]], "Av": [m(a) for a in v["Av"]]})
    out["skipped"] = int((seen.T & ~out["used"]).sum())
    return out


def views_to_fixed(vs):
    out = dict(vs)
    conv = FIXED.from_mp
    out["views"] = [{k: ([conv(a) for a in v] if isinstance(v, list) else conv(v)) for k, v in view.items()} for view in vs["views"]]
    return out


# ---------------------------------------------------------------------------------------------------------------- exact Gram
def _gram_fixed(J):
    """J^T J of an object array of integers, exactly: 20-bit signed limbs as float64 matrices (every product < 2^40, every sum of
    < 4096 of them < 2^52: exact whatever the order), recombined on Python integers."""
    rows, n = J.shape
    G = np.zeros((n, n), dtype=object)
    for r0 in range(0, rows, 4000):
        Jb = J[r0:r0 + 4000]
        sign = np.where(Jb < 0, -1.0, 1.0).astype(np.float64)
        mag = np.abs(Jb)
        bits = max(int(v).bit_length() for v in mag.ravel()) if mag.size else 0
        nl = max(1, (bits + 19) // 20)
        limbs = [((mag >> (20 * k)) & 0xFFFFF).astype(np.float64) * sign for k in range(nl)]
        for d in range(2 * nl - 1):
            acc = np.zeros((n, n), dtype=np.int64)   # <= 9 terms below 2^52 each
            for k in range(max(0, d - nl + 1), min(nl, d + 1)):
                acc += (limbs[k].T @ limbs[d - k]).astype(np.int64)
            G += acc.astype(object) << (20 * d)
    return G >> Q


# ---------------------------------------------------------------------------------------------------------------------- Schur
def schur_stage(F, vs, C, focal, lam):
    """The per-point algebra and the reduced camera system from the views `vs` (numbers of kind F; lam a number of kind F)."""
    N = len(vs["part"])
    n_c = n_cam_params(C, focal)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    V = [F.zeros(N) for _ in pairs]
    g = [F.zeros(N) for _ in range(3)]
    rho = F.zeros(N)
    for c in range(C):
        v = vs["views"][c]
        rho = rho + v["rho"]
        for e, (i, j) in enumerate(pairs):
            V[e] = V[e] + (F.mul(v["Bu"][i], v["Bu"][j]) + F.mul(v["Bv"][i], v["Bv"][j]))
        for j in range(3):
            g[j] = g[j] + (F.mul(v["Bu"][j], v["ru"]) + F.mul(v["Bv"][j], v["rv"]))
    one = F.zeros(N) + F.one
    a00, a11, a22 = (V[e] + F.mul(V[e], lam) for e in (0, 3, 5))
    ok = (a00 > 0).astype(bool)
    l00 = F.sqrt(np.where(ok, a00, one))
    l10, l20 = F.div(V[1], l00), F.div(V[2], l00)
    d1 = a11 - F.mul(l10, l10)
    ok &= (d1 > 0).astype(bool)
    l11 = F.sqrt(np.where(ok, d1, one))
    l21 = F.div(V[4] - F.mul(l20, l10), l11)
    d2 = (a22 - F.mul(l20, l20)) - F.mul(l21, l21)
    ok &= (d2 > 0).astype(bool)
    if F is FLOAT:
        ok &= np.isfinite(a00) & np.isfinite(d1) & np.isfinite(d2)
    l22 = F.sqrt(np.where(ok, d2, one))
    singular = vs["part"] & ~ok
    zero = F.zeros(N)

    def fwd(w0, w1, w2):
        e0 = F.div(w0, l00)
        e1 = F.div(w1 - F.mul(l10, e0), l11)
        e2 = F.div((w2 - F.mul(l20, e0)) - F.mul(l21, e1), l22)
        return [np.where(ok, e, zero) for e in (e0, e1, e2)]
    J = F.zeros((N, 3, n_c + 1))
    for k, e in enumerate(fwd(g[0], g[1], g[2])):
        J[:, k, n_c] = e
    S = F.zeros((n_c, n_c))
    rhs = F.zeros(n_c)
    for c in range(C):
        v = vs["views"][c]
        idx = [6 * (c - 1) + k if c else -1 for k in range(6)] + [6 * (C - 1) + c if focal else -1]
        for k in range(7):
            if idx[k] < 0:
                continue
            w = [F.mul(v["Au"][k], v["Bu"][j]) + F.mul(v["Av"][k], v["Bv"][j]) for j in range(3)]
            for r, e in enumerate(fwd(*w)):
                J[:, r, idx[k]] = e
            for k2 in range(k, 7):
                if idx[k2] < 0:
                    continue
                u = (F.mul(v["Au"][k], v["Au"][k2]) + F.mul(v["Av"][k], v["Av"][k2])).sum()
                if k2 == k:
                    u = u + F.mul(u, lam)
                S[idx[k], idx[k2]] = S[idx[k2], idx[k]] = u
            rhs[idx[k]] = -((F.mul(v["Au"][k], v["ru"]) + F.mul(v["Av"][k], v["rv"])).sum())
    Jm = J.reshape(3 * N, n_c + 1)
    if F is FIXED:
        G = _gram_fixed(Jm)
    else:
        G = Jm.T @ Jm
    S = S - G[:n_c, :n_c]
    rhs = rhs + G[:n_c, n_c]
    return {"S": S, "rhs": rhs, "cost": rho.sum(), "rho": rho, "J": J, "L": (l00, l10, l20, l11, l21, l22), "ok": ok,
            "singular": int(singular.sum())}


def _status(vs, sch):
    C = len(vs["views"])
    unseen = any(not vs["seen"][:, c].any() for c in range(C))
    return ((ST_CAMERA_UNSEEN if unseen else 0) | (0 if vs["part"].any() else ST_NO_POINTS) |
            (ST_POINT_SINGULAR if sch["singular"] else 0) | (ST_BAD_DEPTH if vs["skipped"] else 0))


def linearise(obs, R, t, K, X, fscale=None, focal=False, huber=0.0, lam=0.0):
    """mocap_ba_joint_normal_eq in plain doubles -> dict(S, rhs, cost, ...)."""
    C = len(R)
    vs = view_stage(FLOAT, obs, R, t, K, fscale if focal else None, X, huber)
    sch = schur_stage(FLOAT, vs, C, focal, float(lam))
    sch.update(part=vs["part"], seen=vs["seen"], down=int(vs["down"].sum()), skipped=vs["skipped"], status=_status(vs, sch))
    return sch


_mp_views = {}


def linearise_mp(obs, R, t, K, X, fscale=None, focal=False, huber=0.0, lam=0.0, algebra=FIXED):
    """The same at 50 digits -> dict(S, rhs, cost) of mpmath numbers.  The views (independent of lam) are kept per input."""
    C = len(R)
    with mpmath.workdps(DPS):
        key = (np.asarray(obs).tobytes(), np.asarray(R).tobytes(), np.asarray(t).tobytes(), np.asarray(K).tobytes(),
               np.asarray(X).tobytes(), None if not focal else np.asarray(fscale).tobytes(), float(huber), algebra.name)
        if key not in _mp_views:
            if len(_mp_views) > 3:
                _mp_views.clear()
            vs = view_stage(MP, obs, R, t, K, fscale if focal else None, X, huber)
            cost = sum((v["rho"].sum() for v in vs["views"]), mpmath.mpf(0))
            _mp_views[key] = (views_to_fixed(vs) if algebra is FIXED else vs, cost)
        vs, cost = _mp_views[key]
        if algebra is FIXED:
            sch = schur_stage(FIXED, vs, C, focal, FIXED.from_float(lam))
            return {"S": FIXED.to_mp(sch["S"]), "rhs": FIXED.to_mp(sch["rhs"]), "cost": cost}
        sch = schur_stage(MP, vs, C, focal, mpmath.mpf(float(lam)))
        return {"S": sch["S"], "rhs": sch["rhs"], "cost": cost}


def rel_errors(got, exact):
    """Largest entry-wise error of S relative to max |S|, of rhs relative to max |rhs|, and of the cost, against 50-digit values."""
    with mpmath.workdps(DPS):
        out = []
        for k in ("S", "rhs"):
            ex = np.asarray(exact[k], dtype=object)
            scale = max(abs(v) for v in ex.ravel())
            d = max(abs(mpmath.mpf(float(a)) - b) for a, b in zip(np.asarray(got[k], dtype=np.float64).ravel(), ex.ravel()))
            out.append(float(d / scale) if scale else float(d))
        c = exact["cost"]
        out.append(float(abs(mpmath.mpf(float(got["cost"])) - c) / c) if c else float(abs(got["cost"])))
        return tuple(out)


# ----------------------------------------------------------------------------------------------------------------------- loop
def rotate(w, R):
    """exp([w]x) R by Rodrigues."""
    w = np.asarray(w, dtype=np.float64)
    t2 = float(w @ w)
    th = math.sqrt(t2)
    a = 1.0 - t2 / 6.0 if th < 1e-4 else math.sin(th) / th
    b = 0.5 - t2 / 24.0 if th < 1e-4 else (1.0 - math.cos(th)) / t2
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return (np.eye(3) + a * Wx + b * (Wx @ Wx)) @ R


def dlt_start(obs, R, t, K):
    """The DLT point of each point's views on P_c = K_c [R_c | t_c], NaN where the point does not take part."""
    obs = np.asarray(obs, dtype=np.float64)
    N, C = obs.shape[:2]
    P = [np.asarray(K[c]) @ np.hstack([np.asarray(R[c]), np.asarray(t[c]).reshape(3, 1)]) for c in range(C)]
    X = np.full((N, 3), np.nan)
    part0, seen = participating(obs, np.zeros((N, 3)))
    for p in np.nonzero(part0)[0]:
        rows = []
        for c in np.nonzero(seen[p])[0]:
            u, v = obs[p, c]
            rows += [v * P[c][2] - P[c][1], P[c][0] - u * P[c][2]]
        A = np.array(rows)
        vec = np.linalg.eigh(A.T @ A)[1][:, 0]
        x = vec[:3] / vec[3]
        if np.isfinite(x).all() and all((P[c][2, :3] @ x + P[c][2, 3]) > 0 for c in np.nonzero(seen[p])[0]):
            X[p] = x
    return X


def solve(obs, R, t, K, fscale=None, focal=False, huber=0.0, ftol=1e-10, max_iter=50, progress=None):
    """mocap_ba_joint_solve in plain doubles -> (R, t, fscale, X, info).  progress(R, t, cost) once per accepted step."""
    obs = np.asarray(obs, dtype=np.float64)
    N, C = obs.shape[:2]
    R0, t0 = np.array(R, dtype=np.float64).reshape(C, 3, 3), np.array(t, dtype=np.float64).reshape(C, 3)
    R, t = R0.copy(), t0.copy()
    s = np.ones(C) if not focal or fscale is None else np.array(fscale, dtype=np.float64)
    s0 = s.copy()
    n_c = n_cam_params(C, focal)
    X = dlt_start(obs, R, t, K)
    lam = 1e-3
    lin = linearise(obs, R, t, K, X, s, focal, huber, lam)
    part = lin["part"]
    info = {"passes": 0, "accepted": 0, "cost0": float(lin["cost"]), "cost": float(lin["cost"]), "participating": int(part.sum()),
            "excluded": int(N - part.sum()), "down_weighted": lin["down"], "status": lin["status"] & ~ST_BAD_DEPTH, "costs": []}
    run = not info["status"] & (ST_CAMERA_UNSEEN | ST_NO_POINTS)
    stale = False
    while run:
        if lam > 1e12:
            info["status"] |= ST_LAMBDA
            break
        if info["passes"] >= max_iter:
            info["status"] |= ST_MAX_ITER
            break
        info["passes"] += 1
        if stale:
            lin = linearise(obs, R, t, K, X, s, focal, huber, lam)
            stale = False
        ok = True
        try:
            Lc = np.linalg.cholesky(lin["S"])
            delta = np.linalg.solve(Lc.T, np.linalg.solve(Lc, lin["rhs"]))
            ok = bool(np.isfinite(delta).all())
        except np.linalg.LinAlgError:
            ok = False
        if not ok:
            info["status"] |= ST_SINGULAR
        lam_t = max(lam / 10.0, 1e-12)
        if ok:
            J, (l00, l10, l20, l11, l21, l22) = lin["J"], lin["L"]
            y = J[:, :, n_c] + J[:, :, :n_c] @ delta
            x2 = y[:, 2] / l22
            x1 = (y[:, 1] - l21 * x2) / l11
            x0 = ((y[:, 0] - l10 * x1) - l20 * x2) / l00
            move = part & lin["ok"]
            Xt = X.copy()
            Xt[move] = X[move] - np.stack([x0, x1, x2], axis=1)[move]
            Rt, tt, st = R.copy(), t.copy(), s.copy()
            for c in range(1, C):
                Rt[c] = rotate(delta[6 * (c - 1):6 * (c - 1) + 3], R[c])
                tt[c] = t[c] + delta[6 * (c - 1) + 3:6 * (c - 1) + 6]
            if focal:
                st = s * (1.0 + delta[6 * (C - 1):])
            trial = linearise(obs, Rt, tt, K, Xt, st, focal, huber, lam_t)
            ok = bool(np.isfinite(trial["cost"])) and trial["skipped"] == 0 and trial["cost"] < info["cost"]
        if not ok:
            lam *= 10.0
            stale = True
            continue
        before = info["cost"]
        R, t, s, X, lin, lam = Rt, tt, st, Xt, trial, lam_t
        info["cost"] = float(trial["cost"])
        info["down_weighted"] = trial["down"]
        info["status"] |= trial["status"] & ST_POINT_SINGULAR
        info["accepted"] += 1
        info["costs"].append(info["cost"])
        if progress is not None:
            progress(R.copy(), t.copy(), info["cost"])
        if before - info["cost"] <= ftol * before:
            break
    info["lambda"] = lam
    scale = 1.0
    if run:
        n_in, n_out = np.linalg.norm(t0[1]), np.linalg.norm(t[1])
        if np.isfinite(n_in) and np.isfinite(n_out) and n_in > 0 and n_out > 0:
            scale = n_in / n_out
    Xo = np.where(part[:, None], X * scale, np.nan)
    if not (run and info["accepted"]):
        return R0, t0, s0, Xo, info
    t = t * scale
    R[0], t[0] = R0[0], t0[0]
    return R, t, s, Xo, info


# ------------------------------------------------------------------------------------------------------------------- measures
def pose_errors(R, t, rig):
    """Largest rotation error (rad) and largest translation error relative to |t_1| against the planted rig, after the gauge
    (both are scaled to |t_1| = the rig's)."""
    R, t = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3), np.asarray(t, dtype=np.float64).reshape(-1, 3)
    k = np.linalg.norm(rig["t"][1]) / np.linalg.norm(t[1])
    rot = 0.0
    for c in range(len(R)):
        d = R[c] @ rig["R"][c].T
        skew = 0.5 * np.array([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]])
        rot = max(rot, math.atan2(np.linalg.norm(skew), 0.5 * (np.trace(d) - 1.0)))
    tr = np.abs(t * k - rig["t"]).max() / np.linalg.norm(rig["t"][1])
    return rot, float(tr)


# ---------------------------------------------------------------------------------------------------------------------- cases
def planted_case(C, N, noise_px=0.0, seed=6, start_seed=1, calibrated=False, dropout=0.05, rot_sigma=0.02, trans_sigma=0.05):
    """A planted rig, its observations and perturbed start poses: synth.ring_rig / make_ba_observations / perturb_rig."""
    from mocap_core import synth
    rig = synth.calibrated_ring_rig(C, seed=0) if calibrated else synth.ring_rig(C)
    obs, X0 = synth.make_ba_observations(rig, N, seed=seed, noise_px=noise_px, dropout=dropout)
    start = synth.perturb_rig(rig, np.random.default_rng(start_seed), rot_sigma=rot_sigma, trans_sigma=trans_sigma)
    return rig, obs, X0, start


def outlier_case():
    """The Huber input: ring_rig(4), 200 points, 0.3 px noise, 5 % of the observations moved by +-U(20, 50) px per coordinate
    (rng seed 3).  -> (rig, clean obs, obs with outliers, number moved, start poses)."""
    rig, obs, _, start = planted_case(4, 200, noise_px=0.3)
    rng = np.random.default_rng(3)
    seen = np.argwhere(~np.isnan(obs[..., 0]))
    pick = seen[rng.choice(len(seen), int(round(0.05 * len(seen))), replace=False)]
    bad = obs.copy()
    for p, c in pick:
        bad[p, c] += rng.choice([-1.0, 1.0], 2) * rng.uniform(20.0, 50.0, 2)
    return rig, obs, bad, len(pick), start
