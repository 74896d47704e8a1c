"""The statement of "predicted precision" (include/mocap_core.h): plain NumPy, lanes over points, every operation in the order the
header pins -- NumPy's elementwise double operations are IEEE and never fused, so the core's results are compared with this BIT
FOR BIT.  Beside it, a 50-digit mpmath evaluation of the same quantities (an exact symmetric eigen-decomposition, not Jacobi): what the
statement itself is measured against."""
import numpy as np

MAX_POINTS, MAX_VOXELS, MAX_DIM, SUMMARY, SWEEPS = 1 << 24, 1 << 27, 1024, 72, 16
OK, BAD_POINT, BAD_VIEW, FEW_VIEWS, DEGENERATE = 1, 2, 4, 8, 16
ST_SKIP = 1 | 2 | 4       # MOCAP_ST_ROOT_OVERFLOW | CAND_OVERFLOW | HIT_OVERFLOW
INF = float("inf")


def camera_table(K, R, t):
    """P_c = K_c [R_c | t_c] as mocap_set_cameras builds it: each entry summed left to right."""
    K, R, t = np.asarray(K, dtype=np.float64), np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    C = K.shape[0]
    RT = np.concatenate([R.reshape(C, 3, 3), t.reshape(C, 3, 1)], axis=2)
    P = np.empty((C, 3, 4))
    for i in range(3):
        for j in range(4):
            P[:, i, j] = K[:, i, 0] * RT[:, 0, j] + K[:, i, 1] * RT[:, 1, j] + K[:, i, 2] * RT[:, 2, j]
    return P


def fold(P, frame):
    """P' = P [[A, a], [0, 1]]; frame None: P itself."""
    P = np.asarray(P, dtype=np.float64)
    if frame is None:
        return P.copy()
    f = np.asarray(frame, dtype=np.float64).reshape(3, 4)
    out = np.empty_like(P)
    for j in range(3):
        out[:, :, j] = (P[:, :, 0] * f[0, j] + P[:, :, 1] * f[1, j]) + P[:, :, 2] * f[2, j]
    out[:, :, 3] = ((P[:, :, 0] * f[0, 3] + P[:, :, 1] * f[1, 3]) + P[:, :, 2] * f[2, 3]) + P[:, :, 3]
    return out


def validate_common(sigma_px, frame):
    if not (np.isfinite(sigma_px) and sigma_px > 0):
        return "sigma_px"
    if frame is not None and not np.all(np.isfinite(np.asarray(frame, dtype=np.float64))):
        return "frame"
    return None


def validate_vis(width, height, near, far):
    if width < 1 or height < 1:
        return "image"
    if not (np.isfinite(near) and near >= 0):
        return "near"
    if not far > near:
        return "far"
    return None


def validate_points(N):
    return None if 1 <= N <= MAX_POINTS else "N"


def validate_frames(n_frames, K_max):
    if n_frames < 0 or K_max < 1:
        return "size"
    return "size" if n_frames > MAX_POINTS // K_max else None


def validate_map(nx, ny, nz, min_views, max_sigma):
    if not all(1 <= n <= MAX_DIM for n in (nx, ny, nz)):
        return "dims"
    if nx * ny * nz > MAX_VOXELS:
        return "voxels"
    if min_views < 0:
        return "min_views"
    return "max_sigma" if max_sigma != max_sigma else None


def _finite(x):
    with np.errstate(invalid="ignore"):
        return (x - x) == 0.0


def normal(P, xyz, named=None, vis=None):
    """H [N][6], n_views [N], seen [N] u64, bad_view [N].  named [N][C] bool, or vis = (width, height, near, far)."""
    N, C = xyz.shape[0], P.shape[0]
    X, Y, Z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    H = np.zeros((N, 6))
    n = np.zeros(N, dtype=np.int32)
    seen = np.zeros(N, dtype=np.uint64)
    bad = np.zeros(N, dtype=bool)
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    with np.errstate(all="ignore"):
        for c in range(C):
            p = P[c]
            a = p[0, 0] * X + p[0, 1] * Y + p[0, 2] * Z + p[0, 3]
            b = p[1, 0] * X + p[1, 1] * Y + p[1, 2] * Z + p[1, 3]
            w = p[2, 0] * X + p[2, 1] * Y + p[2, 2] * Z + p[2, 3]
            pu, pv = a / w, b / w
            good_w = _finite(w) & (w > 0.0)
            if named is None:
                width, height, near, far = (np.float64(v) for v in vis)
                view = good_w & (w >= near) & (w <= far) & (pu >= 0.0) & (pu < width) & (pv >= 0.0) & (pv < height)
            else:
                view = named[:, c]
            n += view
            seen |= np.where(view, np.uint64(1) << np.uint64(c), np.uint64(0))
            bad |= view & ~good_w
            ju = [(p[0, k] - pu * p[2, k]) / w for k in range(3)]
            jv = [(p[1, k] - pv * p[2, k]) / w for k in range(3)]
            for e, (i, j) in enumerate(pairs):
                h = H[:, e] + ju[i] * ju[j]
                h = h + jv[i] * jv[j]
                H[:, e] = np.where(view, h, H[:, e])
    return H, n, seen, bad


def jacobi3(H):
    """-> lam [N][3] (A's diagonal as the iteration left it), V [N][3][3], sweeps [N] begun."""
    N = H.shape[0]
    A = np.empty((N, 3, 3))
    idx = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    for i in range(3):
        for j in range(3):
            A[:, i, j] = H[:, idx[(min(i, j), max(i, j))]]
    V = np.zeros((N, 3, 3))
    for i in range(3):
        V[:, i, i] = 1.0
    done = np.zeros(N, dtype=bool)
    sweeps = np.zeros(N, dtype=np.int32)
    with np.errstate(all="ignore"):
        for sweep in range(SWEEPS):
            off = (np.abs(A[:, 0, 1]) + np.abs(A[:, 0, 2])) + np.abs(A[:, 1, 2])
            done |= off == 0.0
            if done.all():
                break
            sweeps += ~done
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = A[:, p, q].copy()
                act = ~done & ~(apq == 0.0)
                g = 100.0 * np.abs(apq)
                app, aqq = A[:, p, p].copy(), A[:, q, q].copy()
                zero = act & (sweep > 3) & (np.abs(app) + g == np.abs(app)) & (np.abs(aqq) + g == np.abs(aqq))
                rot = act & ~zero
                theta = (aqq - app) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                cs = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * cs
                A[:, p, p] = np.where(rot, app - t * apq, app)
                A[:, q, q] = np.where(rot, aqq + t * apq, aqq)
                A[:, p, q] = A[:, q, p] = np.where(act, 0.0, apq)
                for k in range(3):
                    if k != p and k != q:
                        akp, akq = A[:, k, p].copy(), A[:, k, q].copy()
                        A[:, k, p] = A[:, p, k] = np.where(rot, cs * akp - sn * akq, akp)
                        A[:, k, q] = A[:, q, k] = np.where(rot, sn * akp + cs * akq, akq)
                    vkp, vkq = V[:, k, p].copy(), V[:, k, q].copy()
                    V[:, k, p] = np.where(rot, cs * vkp - sn * vkq, vkp)
                    V[:, k, q] = np.where(rot, sn * vkp + cs * vkq, vkq)
    lam = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1)
    return lam, V, sweeps


def _cas(lam, V, i, j):
    with np.errstate(invalid="ignore"):
        sw = lam[:, i] > lam[:, j]
    li, lj = lam[:, i].copy(), lam[:, j].copy()
    lam[:, i], lam[:, j] = np.where(sw, lj, li), np.where(sw, li, lj)
    vi, vj = V[:, :, i].copy(), V[:, :, j].copy()
    V[:, :, i], V[:, :, j] = np.where(sw[:, None], vj, vi), np.where(sw[:, None], vi, vj)


def evaluate(Pp, xyz, sigma_px, named=None, vis=None):
    """The per-point statement on the folded table Pp -> dict with cov, sig, axis, n_views, info, seen, sweeps."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    N = xyz.shape[0]
    H, n, seen, bad = normal(Pp, xyz, named, vis)
    flags = np.zeros(N, dtype=np.int32)
    flags |= np.where(~(_finite(xyz[:, 0]) & _finite(xyz[:, 1]) & _finite(xyz[:, 2])), BAD_POINT, 0).astype(np.int32)
    flags |= np.where(bad, BAD_VIEW, 0).astype(np.int32)
    flags |= np.where(n < 2, FEW_VIEWS, 0).astype(np.int32)
    lam, V, sweeps = jacobi3(H)
    _cas(lam, V, 0, 1)
    _cas(lam, V, 1, 2)
    _cas(lam, V, 0, 1)
    s = np.float64(sigma_px)
    with np.errstate(all="ignore"):
        ok = _finite(lam[:, 0]) & _finite(lam[:, 1]) & _finite(lam[:, 2]) & ~(lam[:, 0] <= lam[:, 2] * 2.0 ** -40)
        sig = np.stack([s / np.sqrt(lam[:, 2]), s / np.sqrt(lam[:, 1]), s / np.sqrt(lam[:, 0])], axis=1)
        v = V[:, :, 0]
        big = v[:, 0].copy()
        big = np.where(np.abs(v[:, 1]) > np.abs(big), v[:, 1], big)
        big = np.where(np.abs(v[:, 2]) > np.abs(big), v[:, 2], big)
        axis = np.where((big < 0.0)[:, None], -v, v)
        s2 = s * s
        d = [s2 / lam[:, k] for k in range(3)]
        cov = np.stack([((V[:, i, 0] * V[:, j, 0]) * d[0] + (V[:, i, 1] * V[:, j, 1]) * d[1]) + (V[:, i, 2] * V[:, j, 2]) * d[2]
                        for i in range(3) for j in range(i, 3)], axis=1)
    clean = flags == 0
    info = np.where(clean, np.where(ok, OK, DEGENERATE), flags).astype(np.int32)
    good = info == OK
    nan = np.float64("nan")
    return {"cov": np.where(good[:, None], cov, nan), "sig": np.where(good[:, None], sig, nan), "axis": np.where(good[:, None], axis, nan),
            "n_views": n, "info": info, "seen": seen, "sweeps": np.where(clean, sweeps, 0)}


def named_from_bits(seen, C):
    seen = np.asarray(seen, dtype=np.uint64)
    return np.stack([((seen >> np.uint64(c)) & np.uint64(1)).astype(bool) for c in range(C)], axis=1)


def point_precision(P, xyz, seen=None, image_size=None, near=0.0, far=INF, sigma_px=1.0, frame=None):
    Pp = fold(P, frame)
    if seen is None:
        return evaluate(Pp, xyz, sigma_px, vis=(image_size[0], image_size[1], near, far))
    return evaluate(Pp, xyz, sigma_px, named=named_from_bits(seen, P.shape[0]))


def frame_precision(P, xyz, corr, n_pts, status=None, sigma_px=1.0, frame=None):
    xyz = np.asarray(xyz, dtype=np.float64)
    F, K = xyz.shape[:2]
    C = P.shape[0]
    n_pts = np.asarray(n_pts).reshape(F)
    st = np.zeros(F, dtype=np.int64) if status is None else np.asarray(status).reshape(F)
    skip = ((st & ST_SKIP) != 0) | (n_pts < 0) | (n_pts > K)
    live = (~skip[:, None] & (np.arange(K)[None, :] < n_pts[:, None])).reshape(-1)
    r = evaluate(fold(P, frame), xyz.reshape(-1, 3), sigma_px, named=np.asarray(corr).reshape(F * K, C) >= 0)
    out = {}
    for k in ("cov", "sig", "axis"):
        out[k] = np.where(live[:, None], r[k], np.float64("nan")).reshape(F, K, -1)
    for k in ("n_views", "info"):
        out[k] = np.where(live, r[k], 0).astype(np.int32).reshape(F, K)
    return out


def grid_points(shape, origin, e0, e1, e2):
    nx, ny, nz = shape
    o, e0, e1, e2 = (np.asarray(v, dtype=np.float64).reshape(3) for v in (origin, e0, e1, e2))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    i, j, k = (v.reshape(-1).astype(np.float64) for v in (i, j, k))
    return np.stack([((o[d] + i * e0[d]) + j * e1[d]) + k * e2[d] for d in range(3)], axis=1)


def coverage_map(P, shape, origin, e0, e1, e2, image_size, near=0.0, far=INF, sigma_px=1.0, frame=None, min_views=2, max_sigma=INF):
    nx, ny, nz = shape
    x = grid_points(shape, origin, e0, e1, e2)
    r = evaluate(fold(P, frame), x, sigma_px, vis=(image_size[0], image_size[1], near, far))
    sig_max = r["sig"][:, 2]
    with np.errstate(invalid="ignore"):
        good = (r["info"] == OK) & (r["n_views"] >= min_views) & (sig_max <= np.float64(max_sigma))
    summary = np.zeros(SUMMARY, dtype=np.int64)
    summary[:65] = np.bincount(r["n_views"], minlength=65)
    summary[65] = good.sum()
    lin = np.nonzero(good)[0]
    idx = (lin % nx, (lin // nx) % ny, lin // (nx * ny))
    for d, n in enumerate((nx, ny, nz)):
        summary[66 + 2 * d] = idx[d].min() if lin.size else n
        summary[67 + 2 * d] = idx[d].max() if lin.size else -1
    return {"n_views": r["n_views"].astype(np.uint8).reshape(nz, ny, nx), "sig_max": sig_max.astype(np.float32).reshape(nz, ny, nx),
            "seen": r["seen"].reshape(nz, ny, nx), "summary": summary, "sig": r["sig"].reshape(nz, ny, nx, 3), "info": r["info"].reshape(nz, ny, nx)}


def world_frame(T):
    """frame = the inverse of the world transform  x_w = swap_yz(dehom(T [diag(-1,-1,1) X; 1]))  (what the helpers build); ValueError
    for a T whose last row is not (0, 0, 0, k), k != 0, or whose linear part is singular."""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    if not np.all(np.isfinite(T)) or T[3, 0] != 0 or T[3, 1] != 0 or T[3, 2] != 0 or T[3, 3] == 0:
        raise ValueError("not affine")
    S = np.array([[1.0, 0, 0], [0, 0, 1.0], [0, 1.0, 0]])
    M = S @ (T[:3, :3] / T[3, 3]) @ np.diag([-1.0, -1.0, 1.0])
    m = S @ (T[:3, 3] / T[3, 3])
    if abs(np.linalg.det(M)) < 1e-300 or np.linalg.cond(M) > 1e12:
        raise ValueError("singular")
    A = np.linalg.inv(M)
    return np.concatenate([A, (-A @ m)[:, None]], axis=1)


# ----------------------------------------------------------------------------- 50 digits
def exact(Pp, x, views, sigma_px):
    """sig [3] ascending, axis [3], cov [6] at one point from an exact eigen-decomposition in 50-digit arithmetic (mpmath floats)."""
    import mpmath as mp
    mp.mp.dps = 50
    X = [mp.mpf(float(v)) for v in x]
    H = mp.zeros(3, 3)
    for c in views:
        p = [[mp.mpf(float(v)) for v in row] for row in Pp[c]]
        a, b, w = (p[r][0] * X[0] + p[r][1] * X[1] + p[r][2] * X[2] + p[r][3] for r in range(3))
        pu, pv = a / w, b / w
        for row, pr in ((p[0], pu), (p[1], pv)):
            J = [(row[k] - pr * p[2][k]) / w for k in range(3)]
            for i in range(3):
                for j in range(3):
                    H[i, j] += J[i] * J[j]
    E, Q = mp.eigsy(H)
    order = sorted(range(3), key=lambda k: E[k])
    lam = [E[k] for k in order]
    s = mp.mpf(float(sigma_px))
    sig = [s / mp.sqrt(lam[2]), s / mp.sqrt(lam[1]), s / mp.sqrt(lam[0])]
    v = [Q[i, order[0]] for i in range(3)]
    m = max(range(3), key=lambda i: (abs(v[i]), -i))
    if v[m] < 0:
        v = [-c for c in v]
    cov = (s * s) * mp.inverse(H)
    return sig, v, [cov[i, j] for i in range(3) for j in range(i, 3)]
