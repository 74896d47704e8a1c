"""The "point refinement" contract (include/mocap_core.h) as a plain Python statement: every number is a Python float (an IEEE
double), every operation one rounding, in the order the header pins -- no NumPy arithmetic, no BLAS.  The start point is an
argument: on the GPU it is what mocap_triangulate gives for the same observations, in the CPU tests dlt_start below."""
import math

import numpy as np

MAX_ITERS = 16
RF_REFINED, RF_FEW_VIEWS, RF_BAD_INDEX, RF_BAD_OBS, RF_BAD_START, RF_STEPS_SHIFT = 1, 2, 4, 8, 16, 8
STATUS_SKIP = 1 | 2 | 4          # MOCAP_ST_ROOT_OVERFLOW | CAND_OVERFLOW | HIT_OVERFLOW
LAMBDA0 = 1e-3


def camera_table(K, R, t):
    """P_c = K_c [R_c | t_c] with each camera's own K: P[i][j] = K[i][0] RT[0][j] + K[i][1] RT[1][j] + K[i][2] RT[2][j], left to
    right.  -> list of C lists of 12 floats (row-major 3 x 4)."""
    out = []
    for Kc, Rc, tc in zip(np.asarray(K, dtype=np.float64), np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)):
        k = [[float(v) for v in row] for row in Kc.reshape(3, 3)]
        rt = [[float(Rc.reshape(3, 3)[i][j]) for j in range(3)] + [float(tc.reshape(3)[i])] for i in range(3)]
        out.append([k[i][0] * rt[0][j] + k[i][1] * rt[1][j] + k[i][2] * rt[2][j] for i in range(3) for j in range(4)])
    return out


def _div(a, b):
    """IEEE division where Python raises."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def evaluate(P, views, X, grad=True):
    """views: [(camera, u, v)] ascending.  -> (cost, H[6] as 00 01 02 11 12 22, g[3], valid)."""
    x, y, z = X
    cost, H, g, valid = 0.0, [0.0] * 6, [0.0] * 3, True
    for c, u, v in views:
        p = P[c]
        a = p[0] * x + p[1] * y + p[2] * z + p[3]
        b = p[4] * x + p[5] * y + p[6] * z + p[7]
        w = p[8] * x + p[9] * y + p[10] * z + p[11]
        valid = valid and math.isfinite(w) and w > 0.0
        pu, pv = _div(a, w), _div(b, w)
        ru, rv = pu - u, pv - v
        cost = cost + ru * ru
        cost = cost + rv * rv
        if grad:
            ju = [_div(p[k] - pu * p[8 + k], w) for k in range(3)]
            jv = [_div(p[4 + k] - pv * p[8 + k], w) for k in range(3)]
            e = 0
            for i in range(3):
                for j in range(i, 3):
                    H[e] = H[e] + ju[i] * ju[j]
                    H[e] = H[e] + jv[i] * jv[j]
                    e += 1
            for k in range(3):
                g[k] = g[k] + ju[k] * ru
                g[k] = g[k] + jv[k] * rv
    return cost, H, g, valid


def _pos(d):
    return math.isfinite(d) and d > 0.0


def refine(P, views, start, iters):
    """`iters` Levenberg-Marquardt steps from `start`.  -> (X, cost, accepted) or None when the start is not finite or not valid."""
    X = [float(v) for v in start]
    cost, H, g, valid = evaluate(P, views, X, iters > 0)
    if not (valid and all(math.isfinite(v) for v in X)):
        return None
    lam, accepted = LAMBDA0, 0
    for it in range(iters):
        d0 = H[0] + lam * H[0]
        a11 = H[3] + lam * H[3]
        a22 = H[5] + lam * H[5]
        l10, l20 = _div(H[1], d0), _div(H[2], d0)
        d1 = a11 - l10 * H[1]
        t21 = H[4] - l20 * H[1]
        l21 = _div(t21, d1)
        d2 = (a22 - l20 * H[2]) - l21 * t21
        z0 = -g[0]
        z1 = -g[1] - l10 * z0
        z2 = (-g[2] - l20 * z0) - l21 * z1
        y0, y1, y2 = _div(z0, d0), _div(z1, d1), _div(z2, d2)
        e2 = y2
        e1 = y1 - l21 * e2
        e0 = (y0 - l10 * e1) - l20 * e2
        T = [X[0] + e0, X[1] + e1, X[2] + e2]
        tc, tH, tg, tv = evaluate(P, views, T, it + 1 < iters)
        if _pos(d0) and _pos(d1) and _pos(d2) and tv and tc < cost:
            X, cost, H, g = T, tc, tH, tg
            lam = lam / 10.0
            accepted += 1
        else:
            lam = lam * 10.0
    return X, cost, accepted


def refine_views(P, views, start, iters):
    """One group whose views are all usable.  -> (X or None, err or None, info)."""
    r = refine(P, views, start, iters)
    if r is None:
        return None, None, RF_BAD_START
    X, cost, accepted = r
    return X, cost / float(2 * len(views)), RF_REFINED | (accepted << RF_STEPS_SHIFT)


def obs_views(row):
    """A row of the observation form, [C][2] with NaN for unseen -> (views, flags)."""
    views, flags = [], 0
    for c, (u, v) in enumerate(np.asarray(row, dtype=np.float64)):
        if math.isnan(u) or math.isnan(v):
            continue
        views.append((c, float(u), float(v)))
        if not (math.isfinite(u) and math.isfinite(v)):
            flags |= RF_BAD_OBS
    if len(views) < 2:
        flags |= RF_FEW_VIEWS
    return views, flags


def triangulate_refined(P, obs, starts, iters):
    """mocap_triangulate_refined: obs [N][C][2], starts [N][3] (mocap_triangulate's xyz) -> xyz [N][3], err [N], info [N]."""
    obs = np.asarray(obs, dtype=np.float64)
    N = obs.shape[0]
    xyz, err, info = np.full((N, 3), np.nan), np.full(N, np.nan), np.zeros(N, dtype=np.int32)
    for i in range(N):
        views, flags = obs_views(obs[i])
        if not flags:
            X, e, flags = refine_views(P, views, starts[i], iters)
            if X is not None:
                xyz[i], err[i] = X, e
        info[i] = flags
    return xyz, err, info


def corr_views(blobs_f, counts_f, row):
    """A row of corr against the frame's blobs [C][M][2] (float32) and counts [C] -> (views, flags)."""
    M = blobs_f.shape[1]
    views, flags, v = [], 0, 0
    for c, j in enumerate(row):
        j = int(j)
        if j < 0:
            continue
        v += 1
        if j >= int(counts_f[c]) or j >= M:
            flags |= RF_BAD_INDEX
            continue
        x, y = float(blobs_f[c, j, 0]), float(blobs_f[c, j, 1])
        if not (math.isfinite(x) and math.isfinite(y)):
            flags |= RF_BAD_OBS
        views.append((c, x, y))
    if v < 2:
        flags |= RF_FEW_VIEWS
    return views, flags


def store_point(W, X):
    """The frame path's store (csrc/frame_common.hpp): plain, or through the world epilogue, in its order and unfused."""
    if W is None:
        return [X[0], X[1], X[2]]
    w = [float(v) for v in np.asarray(W, dtype=np.float64).reshape(16)]
    x, y, z = -X[0], -X[1], X[2]
    h = [w[4 * i] * x + w[4 * i + 1] * y + w[4 * i + 2] * z + w[4 * i + 3] for i in range(4)]
    return [_div(h[0], h[3]), _div(h[2], h[3]), _div(h[1], h[3])]


def refine_frames(P, blobs, counts, xyz, err, corr, n_pts, status, start_of, iters, world=None):
    """mocap_refine_points.  start_of(views) -> the start of a group (camera-0 coordinates).  The inputs are not touched.
    -> {"xyz", "err", "info"}."""
    xyz, err = np.array(xyz, dtype=np.float64), np.array(err, dtype=np.float64)
    F, K_max = err.shape
    info = np.zeros((F, K_max), dtype=np.int32)
    for f in range(F):
        n, st = int(n_pts[f]), 0 if status is None else int(status[f])
        if (st & STATUS_SKIP) or n < 0 or n > K_max:
            continue
        for k in range(n):
            views, flags = corr_views(blobs[f], counts[f], corr[f, k])
            if not flags:
                X, e, flags = refine_views(P, views, start_of(views), iters)
                if X is not None:
                    xyz[f, k], err[f, k] = store_point(world, X), e
            info[f, k] = flags
    return {"xyz": xyz, "err": err, "info": info}


def views_to_obs(views, C):
    row = np.full((C, 2), np.nan)
    for c, u, v in views:
        row[c] = (u, v)
    return row


# ---------------------------------------------------------------- helpers of the tests (NumPy allowed from here on)
def dlt_start(K, R, t, views):
    """The reference's DLT point (helpers.py:293-327) with its quirk: the intrinsics of view number j, the pose of camera c."""
    rows = []
    for j, (c, u, v) in enumerate(views):
        Pm = np.asarray(K[j], dtype=np.float64) @ np.hstack([np.asarray(R[c]), np.asarray(t[c]).reshape(3, 1)])
        rows += [v * Pm[2] - Pm[1], Pm[0] - u * Pm[2]]
    vt = np.linalg.svd(np.array(rows))[2]
    return vt[-1, :3] / vt[-1, 3]


def project(K, R, t, X):
    """Pixels of X [3] in every camera, each with its own K -> [C][2], depth [C]."""
    pc = np.einsum("cij,j->ci", R, X) + t
    h = np.einsum("cij,cj->ci", K, pc)
    return h[:, :2] / h[:, 2:3], pc[:, 2]


def random_groups(rig, N, rng, noise=0.3, integer=False, min_views=2, max_views=None):
    """N points around the rig's centre seen by min_views .. max_views random cameras -> obs [N][C][2] (NaN unseen), truth [N][3]."""
    K, R, t = rig["K"], rig["R"], rig["t"]
    C = len(K)
    max_views = C if max_views is None else max_views
    obs, truth = np.full((N, C, 2), np.nan), np.zeros((N, 3))
    for i in range(N):
        X = rig["centre"] + rng.uniform(-0.7, 0.7, 3)
        px, _ = project(K, R, t, X)
        px = px + rng.normal(0, noise, px.shape)
        if integer:
            px = np.trunc(px)
        seen = rng.choice(C, size=int(rng.integers(min_views, max_views + 1)), replace=False)
        obs[i, seen] = px[seen]
        truth[i] = X
    return obs, truth
