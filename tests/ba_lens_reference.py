"""The "lens calibration" section of include/mocap_core.h as plain Python / NumPy: the lens, the view with its 14 parameters per
camera, linearisation, Schur complement, Levenberg-Marquardt loop, and the Newton inverse of the lens.  The number kinds, the exact
Gram, the DLT start, Rodrigues and the pose measures are tests/ba_joint_reference.py's (FLOAT: NumPy doubles; MP: mpmath at 50
digits per view; FIXED: integers scaled by 2^200 for the per-point algebra).

linearise_mp = MP views -> FIXED algebra -> mpmath numbers: the 50-digit S, rhs and cost the device is compared with."""
import mpmath
import numpy as np

import ba_joint_reference as bj
from ba_joint_reference import FIXED, FLOAT, MP, pose_errors, rel_errors  # noqa: F401  (re-exported)

DPS = bj.DPS
MAX_CAMERAS, MAX_POINTS = 16, 65536
NEWTON = 8
FOCAL, CENTRE, RADIAL, TANGENTIAL = 1, 2, 4, 8
ALL = 15
ST_CAMERA_UNSEEN, ST_NO_POINTS, ST_SINGULAR, ST_POINT_SINGULAR, ST_LAMBDA, ST_MAX_ITER, ST_BAD_DEPTH = 1, 2, 4, 8, 16, 32, 64
PAR = 14      # omega 3, t 3, fx, fy, cx, cy, k1, k2, p1, p2


def n_unknowns(flags):
    return 2 * bin(flags & ALL).count("1")


def n_cam_params(C, flags):
    return 6 * (C - 1) + n_unknowns(flags) * C


def columns(C, c, flags):
    """The 14 parameters of camera c -> their columns of the reduced system, -1 = not an unknown."""
    q, idx, r = n_unknowns(flags), [6 * (c - 1) + k if c else -1 for k in range(6)], 0
    for pair in range(4):
        for _ in range(2):
            if flags >> pair & 1:
                idx.append(6 * (C - 1) + q * c + r)
                r += 1
            else:
                idx.append(-1)
    return idx


def check_args(C, N, K, dist, flags, huber_px=0.0, ftol=0.0, max_iter=1, lam=0.0):
    """The MOCAP_E_ARG rules: None when the call is taken, else the reason."""
    K, dist = np.asarray(K, dtype=np.float64).reshape(-1, 3, 3), np.asarray(dist, dtype=np.float64).reshape(-1, 5)
    if not 2 <= C <= MAX_CAMERAS:
        return "cameras"
    if not 1 <= N <= MAX_POINTS:
        return "points"
    if flags & ~ALL:
        return "unknown flag bits"
    if flags and C < 3:
        return "intrinsics need 3 cameras"
    if not bj.plain_K(K):
        return "K is not plain"
    if not (np.isfinite(K).all() and (K[:, 0, 0] > 0).all() and (K[:, 1, 1] > 0).all() and np.isfinite(dist).all()):
        return "intrinsics not finite or a focal length not > 0"
    for v in (huber_px, ftol, lam):
        if not (np.isfinite(v) and v >= 0):
            return "negative or non-finite"
    if max_iter < 1:
        return "max_iter"
    return None


# ----------------------------------------------------------------------------------------------------------------------- lens
def lens(x, y, k):
    """(x, y) normalised, k = k1 k2 p1 p2 k3 -> dict(r2, kr, xd, yd, Jxx, Jxy, Jyy), in the header's order; any number kind."""
    k1, k2, p1, p2, k3 = k
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = (x * kr + ((2 * p1) * x) * y) + p2 * (r2 + (2 * x) * x)
    yd = (y * kr + p1 * (r2 + (2 * y) * y)) + ((2 * p2) * x) * y
    dk = ((3 * k3) * r2 + 2 * k2) * r2 + k1
    dk2 = 2 * dk
    Jxx = (kr + (dk2 * x) * x) + ((2 * p1) * y + (6 * p2) * x)
    Jxy = (dk2 * x) * y + ((2 * p1) * x + (2 * p2) * y)
    Jyy = (kr + (dk2 * y) * y) + ((6 * p1) * y + (2 * p2) * x)
    return {"r2": r2, "kr": kr, "xd": xd, "yd": yd, "Jxx": Jxx, "Jxy": Jxy, "Jyy": Jyy}


def undistort(points, K, dist):
    """mocap_undistort_points in NumPy doubles: [N][C][2] raw pixels -> ideal pinhole pixels."""
    pts = np.asarray(points, dtype=np.float64)
    K, dist = np.asarray(K, dtype=np.float64).reshape(-1, 3, 3), np.asarray(dist, dtype=np.float64).reshape(-1, 5)
    out = np.empty_like(pts)
    with np.errstate(all="ignore"):
        for c in range(K.shape[0]):
            u, v = pts[:, c, 0], pts[:, c, 1]
            if not dist[c].any():
                uo, vo = u.copy(), v.copy()
            else:
                fx, fy, cx, cy = K[c, 0, 0], K[c, 1, 1], K[c, 0, 2], K[c, 1, 2]
                x0, y0 = (u - cx) / fx, (v - cy) / fy
                x, y = x0, y0
                for _ in range(NEWTON):
                    L = lens(x, y, dist[c])
                    ex, ey = L["xd"] - x0, L["yd"] - y0
                    det = L["Jxx"] * L["Jyy"] - L["Jxy"] * L["Jxy"]
                    x, y = x - (L["Jyy"] * ex - L["Jxy"] * ey) / det, y - (L["Jxx"] * ey - L["Jxy"] * ex) / det
                uo, vo = fx * x + cx, fy * y + cy
            nan = np.isnan(u) | np.isnan(v)
            out[:, c, 0] = np.where(nan, np.nan, uo)
            out[:, c, 1] = np.where(nan, np.nan, vo)
    return out


# ---------------------------------------------------------------------------------------------------------------------- views
def view_terms(F, R, t, intr, X, u, v, huber):
    """One camera's view of the points X (three arrays over the points, numbers of kind F), in the header's order.
    intr = fx fy cx cy k1 k2 p1 p2 k3 (scalars of kind F).  Nothing is masked here except the division by a depth that is not > 0."""
    fx, fy, cx, cy = intr[:4]
    P = [(X[0] * R[i][0] + X[1] * R[i][1]) + X[2] * R[i][2] for i in range(3)]
    Y = [P[i] + t[i] for i in range(3)]
    pos = (Y[2] > 0).astype(bool)
    if F is FLOAT:
        pos &= np.isfinite(Y[2])
    Y2 = np.where(pos, Y[2], F.one)
    x, y = Y[0] / Y2, Y[1] / Y2
    L = lens(x, y, intr[4:9])
    ru, rv = (L["xd"] * fx + cx) - u, (L["yd"] * fy + cy) - v
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
    gu, gv = sw * (fx / Y2), sw * (fy / Y2)
    du0, du1 = gu * L["Jxx"], gu * L["Jxy"]
    du2 = -(du0 * x + du1 * y)
    dv0, dv1 = gv * L["Jxy"], gv * L["Jyy"]
    dv2 = -(dv0 * x + dv1 * y)
    Bu = [(du0 * R[0][j] + du1 * R[1][j]) + du2 * R[2][j] for j in range(3)]
    Bv = [(dv0 * R[0][j] + dv1 * R[1][j]) + dv2 * R[2][j] for j in range(3)]
    zero = du0 * 0
    sfx, sfy = sw * fx, sw * fy
    r2 = L["r2"]
    xr, yr, xy2 = x * r2, y * r2, (2 * x) * y
    Au = [du2 * P[1] - du1 * P[2], du0 * P[2] - du2 * P[0], du1 * P[0] - du0 * P[1], du0, du1, du2,
          sfx * L["xd"], zero, sw + zero, zero, sfx * xr, sfx * (xr * r2), sfx * xy2, sfx * (r2 + (2 * x) * x)]
    Av = [dv2 * P[1] - dv1 * P[2], dv0 * P[2] - dv2 * P[0], dv1 * P[0] - dv0 * P[1], dv0, dv1, dv2,
          zero, sfy * L["yd"], zero, sw + zero, sfy * yr, sfy * (yr * r2), sfy * (r2 + (2 * y) * y), sfy * xy2]
    return {"pos": pos, "down": down, "rho": rho, "ru": sw * ru, "rv": sw * rv, "Bu": Bu, "Bv": Bv, "Au": Au, "Av": Av}


def intrinsics(K, dist):
    """[C][9]: fx fy cx cy k1 k2 p1 p2 k3."""
    K, dist = np.asarray(K, dtype=np.float64).reshape(-1, 3, 3), np.asarray(dist, dtype=np.float64).reshape(-1, 5)
    return np.concatenate([K[:, 0, 0, None], K[:, 1, 1, None], K[:, 0, 2, None], K[:, 1, 2, None], dist], axis=1)


def view_stage(F, obs, R, t, intr, X, huber):
    """Every view of every point: arrays [C][...][N] of kind F, zero where the view is not used."""
    obs = np.asarray(obs, dtype=np.float64)
    N, C = obs.shape[:2]
    part, seen = bj.participating(obs, X)
    seen = seen & part[:, None]
    Xs = np.where(part[:, None], np.asarray(X, dtype=np.float64), 0.0)
    Xl = [F.lift(Xs[:, k]) for k in range(3)]
    out = {"part": part, "seen": seen, "used": np.zeros((C, N), bool), "down": np.zeros((C, N), bool), "views": []}
    lift1 = (lambda x: float(x)) if F is FLOAT else (lambda x: mpmath.mpf(float(x)))
    for c in range(C):
        o = np.where(seen[:, c, None], obs[:, c], 0.0)
        Rc = [[lift1(R[c][i][j]) for j in range(3)] for i in range(3)]
        tcam = [lift1(t[c][i]) for i in range(3)]
        v = view_terms(F, Rc, tcam, [lift1(a) for a in intr[c]], Xl, F.lift(o[:, 0]), F.lift(o[:, 1]), huber)
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


# ---------------------------------------------------------------------------------------------------------------------- Schur
def schur_stage(F, vs, C, flags, lam):
    """The per-point algebra and the reduced camera system from the views `vs` (numbers of kind F; lam a number of kind F)."""
    N = len(vs["part"])
    n_c = n_cam_params(C, flags)
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
        idx = columns(C, c, flags)
        for k in range(PAR):
            if idx[k] < 0:
                continue
            w = [F.mul(v["Au"][k], v["Bu"][j]) + F.mul(v["Av"][k], v["Bv"][j]) for j in range(3)]
            for r, e in enumerate(fwd(*w)):
                J[:, r, idx[k]] = e
            for k2 in range(k, PAR):
                if idx[k2] < 0:
                    continue
                u = (F.mul(v["Au"][k], v["Au"][k2]) + F.mul(v["Av"][k], v["Av"][k2])).sum()
                if k2 == k:
                    u = u + F.mul(u, lam)
                S[idx[k], idx[k2]] = S[idx[k2], idx[k]] = u
            rhs[idx[k]] = -((F.mul(v["Au"][k], v["ru"]) + F.mul(v["Av"][k], v["rv"])).sum())
    Jm = J.reshape(3 * N, n_c + 1)
    G = bj._gram_fixed(Jm) if F is FIXED else Jm.T @ Jm
    S = S - G[:n_c, :n_c]
    rhs = rhs + G[:n_c, n_c]
    return {"S": S, "rhs": rhs, "cost": rho.sum(), "rho": rho, "J": J, "L": (l00, l10, l20, l11, l21, l22), "ok": ok,
            "singular": int(singular.sum())}


def linearise(obs, R, t, K, dist, X, flags=0, huber=0.0, lam=0.0, intr=None):
    """mocap_ba_lens_normal_eq in plain doubles -> dict(S, rhs, cost, ...)."""
    C = len(R)
    vs = view_stage(FLOAT, obs, R, t, intrinsics(K, dist) if intr is None else intr, X, huber)
    sch = schur_stage(FLOAT, vs, C, flags, float(lam))
    sch.update(part=vs["part"], seen=vs["seen"], down=int(vs["down"].sum()), skipped=vs["skipped"], status=bj._status(vs, sch))
    return sch


_mp_views = {}


def linearise_mp(obs, R, t, K, dist, X, flags=0, huber=0.0, lam=0.0, algebra=FIXED):
    """The same at 50 digits -> dict(S, rhs, cost) of mpmath numbers.  The views (independent of lam and of flags) are kept per input."""
    C = len(R)
    with mpmath.workdps(DPS):
        key = tuple(np.asarray(a, dtype=np.float64).tobytes() for a in (obs, R, t, K, dist, X)) + (float(huber), algebra.name)
        if key not in _mp_views:
            if len(_mp_views) > 3:
                _mp_views.clear()
            vs = view_stage(MP, obs, R, t, intrinsics(K, dist), X, huber)
            cost = sum((v["rho"].sum() for v in vs["views"]), mpmath.mpf(0))
            _mp_views[key] = (bj.views_to_fixed(vs) if algebra is FIXED else vs, cost)
        vs, cost = _mp_views[key]
        if algebra is FIXED:
            sch = schur_stage(FIXED, vs, C, flags, FIXED.from_float(lam))
            return {"S": FIXED.to_mp(sch["S"]), "rhs": FIXED.to_mp(sch["rhs"]), "cost": cost}
        sch = schur_stage(MP, vs, C, flags, mpmath.mpf(float(lam)))
        return {"S": sch["S"], "rhs": sch["rhs"], "cost": cost}


# ----------------------------------------------------------------------------------------------------------------------- loop
def solve(obs, R, t, K, dist, flags=FOCAL | CENTRE | RADIAL, huber=0.0, ftol=1e-10, max_iter=100):
    """mocap_ba_lens_solve in plain doubles -> (R, t, K, dist, X, info)."""
    obs = np.asarray(obs, dtype=np.float64)
    N, C = obs.shape[:2]
    R0, t0 = np.array(R, dtype=np.float64).reshape(C, 3, 3), np.array(t, dtype=np.float64).reshape(C, 3)
    K0, dist0 = np.array(K, dtype=np.float64).reshape(C, 3, 3), np.array(dist, dtype=np.float64).reshape(C, 5)
    R, t = R0.copy(), t0.copy()
    a = intrinsics(K0, dist0)
    n_c, q = n_cam_params(C, flags), n_unknowns(flags)
    cols = [columns(C, c, flags) for c in range(C)]
    X = bj.dlt_start(obs, R, t, K0)
    lam = 1e-3
    lin = linearise(obs, R, t, None, None, X, flags, huber, lam, intr=a)
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
            lin = linearise(obs, R, t, None, None, X, flags, huber, lam, intr=a)
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
            Rt, tt, at = R.copy(), t.copy(), a.copy()
            for c in range(1, C):
                Rt[c] = bj.rotate(delta[6 * (c - 1):6 * (c - 1) + 3], R[c])
                tt[c] = t[c] + delta[6 * (c - 1) + 3:6 * (c - 1) + 6]
            for c in range(C):
                for k in range(8):
                    if cols[c][6 + k] >= 0:
                        d = delta[cols[c][6 + k]]
                        at[c, k] = a[c, k] * (1.0 + d) if k < 2 else a[c, k] + d
            ok = bool((at[:, :2] > 0).all())      # a focal length that is not > 0: rejected before it is linearised
        if ok:
            J, (l00, l10, l20, l11, l21, l22) = lin["J"], lin["L"]
            y = J[:, :, n_c] + J[:, :, :n_c] @ delta
            x2 = y[:, 2] / l22
            x1 = (y[:, 1] - l21 * x2) / l11
            x0 = ((y[:, 0] - l10 * x1) - l20 * x2) / l00
            move = part & lin["ok"]
            Xt = X.copy()
            Xt[move] = X[move] - np.stack([x0, x1, x2], axis=1)[move]
            trial = linearise(obs, Rt, tt, None, None, Xt, flags, huber, lam_t, intr=at)
            ok = bool(np.isfinite(trial["cost"])) and trial["skipped"] == 0 and trial["cost"] < info["cost"]
        if not ok:
            lam *= 10.0
            stale = True
            continue
        before = info["cost"]
        R, t, a, X, lin, lam = Rt, tt, at, Xt, trial, lam_t
        info["cost"] = float(trial["cost"])
        info["down_weighted"] = trial["down"]
        info["status"] |= trial["status"] & ST_POINT_SINGULAR
        info["accepted"] += 1
        info["costs"].append(info["cost"])
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
        return R0, t0, K0, dist0, Xo, info
    t = t * scale
    R[0], t[0] = R0[0], t0[0]
    Ko, do = K0.copy(), dist0.copy()
    Ko[:, 0, 0], Ko[:, 1, 1], Ko[:, 0, 2], Ko[:, 1, 2] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    do[:, :4] = a[:, 4:8]
    return R, t, Ko, do, Xo, info


# ------------------------------------------------------------------------------------------------------------------- measures
def lens_errors(K, dist, rig):
    """Largest relative focal error, principal-point error (px) and k1 error against the planted lenses."""
    K, dist = np.asarray(K).reshape(-1, 3, 3), np.asarray(dist).reshape(-1, 5)
    f = max(np.abs(K[:, 0, 0] / rig["K"][:, 0, 0] - 1).max(), np.abs(K[:, 1, 1] / rig["K"][:, 1, 1] - 1).max())
    c = max(np.abs(K[:, 0, 2] - rig["K"][:, 0, 2]).max(), np.abs(K[:, 1, 2] - rig["K"][:, 1, 2]).max())
    return float(f), float(c), float(np.abs(dist[:, 0] - rig["dist"][:, 0]).max())


# ---------------------------------------------------------------------------------------------------------------------- cases
def planted_lenses(C, seed=0):
    """calibrated_ring_rig(C, seed) with a lens per camera: REFERENCE_DISTORTION, every coefficient scaled by its own factor in
    [0.7, 1.3], k3 = 0 (k3 is never an unknown: a start of zeros can reach these lenses exactly)."""
    from mocap_core import synth
    rig = synth.calibrated_ring_rig(C, seed=seed)
    rng = np.random.default_rng([int(seed), 0x1E45])
    d = np.array([synth.REFERENCE_DISTORTION] * C) * rng.uniform(0.7, 1.3, (C, 5))
    d[:, 4] = 0.0
    rig["dist"] = d
    return rig


def planted_case(C, N, noise_px=0.0, seed=6, start_seed=1, half_extent=1.3, dropout=0.05, rot_sigma=0.02, trans_sigma=0.05):
    """A planted rig with lenses, a RAW capture of N wand positions that fills the images (half_extent 1.3), and the start a user
    has: perturbed poses, the nominal K, zero distortion.  -> (rig, obs, X0, start); obs is NaN where the ideal or the distorted
    pixel leaves the picture."""
    from mocap_core import synth
    rig = planted_lenses(C)
    ideal, X0 = synth.make_ba_observations(rig, N, seed=seed, noise_px=0.0, dropout=dropout, half_extent=half_extent)
    rng = np.random.default_rng([int(seed), 0x0B5])
    obs = np.full_like(ideal, np.nan)
    w, h = rig["image_size"]
    for c in range(C):
        u, v = synth.distort_pixels(ideal[:, c, 0], ideal[:, c, 1], rig["K"][c], rig["dist"][c])
        u, v = u + rng.normal(0, noise_px, N), v + rng.normal(0, noise_px, N)
        seen = ~np.isnan(u) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
        obs[seen, c, 0], obs[seen, c, 1] = u[seen], v[seen]
    start = synth.perturb_rig(rig, np.random.default_rng(start_seed), rot_sigma=rot_sigma, trans_sigma=trans_sigma)
    start["K"] = np.repeat(np.array(synth.DEFAULT_K)[None], C, axis=0)
    start["dist"] = np.zeros((C, 5))
    return rig, obs, X0, start
