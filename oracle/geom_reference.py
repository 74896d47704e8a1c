"""TEST INFRASTRUCTURE ONLY (oracle/) -- never imported by the product path.

High-precision (mpmath, 50 digits) references of the FP64 geometry core (csrc/mocap_device.hpp), one sample at a time.
Everything works on the float64 inputs as given: a float64 is an exact rational, and what is computed from it here is
exact to 50 digits.

    rsqrt_exact, recip_exact, div_exact     1/sqrt(d), 1/b, a/b rounded to the nearest float64; ulp_distance
    eig4_exact                              eigenvalues, unit eigenvector of the smallest, gap = (lam2 - lam1) / lam4
    trace_inv_exact, shifted_exact          trace(B^-1);  M^T B M with M = [[I, c], [0, 1]]
    triangulate_exact                       the DLT matrix of helpers.py:315-321 summed exactly, its null vector, the point
    reprojection_exact                      helpers.py:214-241 with OpenCV's `z ? 1/z : 1` and the two float32 roundings
    numpy_model_eigvec4                     the loop of smallest_eigvec4 restated in plain float64 NumPy: which path a
                                            matrix takes (number of factorisations), never a reference for a value

THE GAP RULE.  The eigenvector of lam1 moves by (rounding error of B, ~ eps * lam4) / (lam2 - lam1): vector errors are
compared after multiplication by gap = (lam2 - lam1) / lam4 and only where gap >= GAP_MIN; backward errors and the
bounds on lam1 need no gap.

The strata of test matrices (eig_strata, two_view_groups) and the inputs of the public-API comparison (api_case) live here so that the CPU test of this module
and the GPU test of the kernels see the same samples.
"""
import functools
from fractions import Fraction

import mpmath as mp
import numpy as np

DPS = 50
GAP_MIN = 1e-6
ULP = 2.220446049250313e-16
SIDX = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]   # mocap::sidx


def pack(B):
    """Symmetric 4 x 4 -> the 10 packed entries of mocap::sidx."""
    B = np.asarray(B, dtype=np.float64)
    return np.array([B[i, j] for i, j in SIDX])


def unpack(a):
    B = np.zeros((4, 4))
    for k, (i, j) in enumerate(SIDX):
        B[i, j] = B[j, i] = a[k]
    return B


def _f64(x):
    """mp number -> nearest float64 (ties to even), for results in the normal range."""
    with mp.workprec(53):
        return float(+x)


def _mpm(B):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(B, dtype=np.float64)])


# ----------------------------------------------------------------------------- scalar primitives
def rsqrt_exact(d):
    with mp.workdps(DPS):
        return _f64(1 / mp.sqrt(mp.mpf(float(d))))


def recip_exact(b):
    with mp.workdps(DPS):
        return _f64(1 / mp.mpf(float(b)))


def div_exact(a, b):
    with mp.workdps(DPS):
        return _f64(mp.mpf(float(a)) / mp.mpf(float(b)))


def ulp_distance(got, kind, *operands):
    """|got - exact| in units of the spacing of float64 at the exact value; kind: "rsqrt", "recip" or "div"."""
    with mp.workdps(DPS):
        ops = [mp.mpf(float(v)) for v in operands]
        exact = 1 / mp.sqrt(ops[0]) if kind == "rsqrt" else 1 / ops[0] if kind == "recip" else ops[0] / ops[1]
        spacing = float(np.spacing(abs(_f64(exact))))
        return float(abs(mp.mpf(float(got)) - exact) / mp.mpf(spacing))


def fma(a, b, c):
    """The correctly rounded a * b + c of float64 operands (Fraction -> float rounds to nearest even)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


# ----------------------------------------------------------------------------- symmetric 4 x 4
def eig4_exact(B):
    """-> (lam [4] mp numbers ascending, v: unit eigenvector of lam[0] as 4 mp numbers, gap: float)."""
    with mp.workdps(DPS):
        E, Q = mp.eigsy(_mpm(B))
        order = sorted(range(4), key=lambda i: E[i])
        lam = [E[i] for i in order]
        v = [Q[r, order[0]] for r in range(4)]
        n = mp.sqrt(sum(x * x for x in v))
        v = [x / n for x in v]
        gap = float((lam[1] - lam[0]) / lam[3]) if lam[3] != 0 else 0.0
        return lam, v, gap


def vector_error(x, v):
    """Distance of x / |x| from the unit mp vector v, up to sign."""
    with mp.workdps(DPS):
        x = [mp.mpf(float(t)) for t in x]
        n = mp.sqrt(sum(t * t for t in x))
        if n == 0:
            return float("inf")
        x = [t / n for t in x]
        dm = mp.sqrt(sum((a - b) ** 2 for a, b in zip(x, v)))
        dp = mp.sqrt(sum((a + b) ** 2 for a, b in zip(x, v)))
        return float(min(dm, dp))


def backward_error(B, x, lam):
    """|B x - lam1 x| / (lam4 |x|) with the exact eigenvalues lam of the float64 matrix B."""
    with mp.workdps(DPS):
        M = _mpm(B)
        x = [mp.mpf(float(t)) for t in x]
        n = mp.sqrt(sum(t * t for t in x))
        if n == 0 or lam[3] == 0:
            return float("inf")
        r = [sum(M[i, j] * x[j] for j in range(4)) - lam[0] * x[i] for i in range(4)]
        return float(mp.sqrt(sum(t * t for t in r)) / (abs(lam[3]) * n))


def trace_inv_exact(B):
    """trace(B^-1) of the float64 (or mp) matrix B, as an mp number."""
    with mp.workdps(DPS):
        M = B if isinstance(B, mp.matrix) else _mpm(B)
        inv = mp.inverse(M)
        return +sum(inv[i, i] for i in range(4))


def shifted_exact(B, c):
    """M^T B M with M = [[I, c], [0, 1]] (the world origin moved to c), exact, as an mp matrix."""
    with mp.workdps(DPS):
        M = mp.eye(4)
        for i in range(3):
            M[i, 3] = mp.mpf(float(c[i]))
        return M.T * _mpm(B) * M


def eig4_exact_mp(Bm):
    """eig4_exact's eigenvalues for a matrix that is already mp (shifted_exact's)."""
    with mp.workdps(DPS):
        E, _ = mp.eigsy(Bm)
        return sorted(E[i] for i in range(4))


# ----------------------------------------------------------------------------- DLT and reprojection
def _seen(obs):
    return [c for c in range(len(obs)) if not np.isnan(obs[c][0])]


def _proj_exact(K, R, t):
    """K @ [R | t] exactly: 3 x 4 mp numbers."""
    K, R, t = np.asarray(K, dtype=np.float64), np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3)
    Rt = [[mp.mpf(float(R[i, j])) for j in range(3)] + [mp.mpf(float(t[i]))] for i in range(3)]
    return [[sum(mp.mpf(float(K[i, k])) * Rt[k][j] for k in range(3)) for j in range(4)] for i in range(3)]


def triangulate_exact(obs, Ks, R, t):
    """helpers.py:293-327 exactly.  obs (C, 2) float64, NaN = unseen; the view at compacted position j takes Ks[j]
    (helpers.py:296-298, 305-307).  -> (X float64 [3], gap, v3 = |last component of the unit null vector|), or None
    when fewer than two cameras see the point."""
    seen = _seen(obs)
    if len(seen) <= 1:
        return None
    with mp.workdps(DPS):
        B = mp.zeros(4, 4)
        for j, c in enumerate(seen):
            P = _proj_exact(Ks[j], R[c], t[c])
            x, y = mp.mpf(float(obs[c][0])), mp.mpf(float(obs[c][1]))
            ra = [y * P[2][k] - P[1][k] for k in range(4)]
            rb = [P[0][k] - x * P[2][k] for k in range(4)]
            for i in range(4):
                for k in range(4):
                    B[i, k] += ra[i] * ra[k] + rb[i] * rb[k]
        E, Q = mp.eigsy(B)
        order = sorted(range(4), key=lambda i: E[i])
        v = [Q[r, order[0]] for r in range(4)]
        n = mp.sqrt(sum(q * q for q in v))
        gap = float((E[order[1]] - E[order[0]]) / E[order[3]])
        X = np.array([float(v[k] / v[3]) for k in range(3)])
        return X, gap, float(abs(v[3]) / n)


def _f32_tie_distance(p):
    """Relative distance of the mp number p from the nearest point where rounding to float32 changes its result."""
    if p == 0:
        return 1.0
    f = np.float32(_f64(p))
    lo, hi = (f, np.nextafter(f, np.float32(np.inf))) if mp.mpf(float(f)) <= p else (np.nextafter(f, np.float32(-np.inf)), f)
    mid = (mp.mpf(float(lo)) + mp.mpf(float(hi))) / 2
    return float(abs(p - mid) / abs(p))


def _round_f32(p):
    """mp number -> nearest float32 (as an mp number).  Exact unless p lies within 2^-53 of a tie: see _f32_tie_distance."""
    f = np.float32(_f64(p))
    best = f
    for cand in (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
        if abs(mp.mpf(float(cand)) - p) < abs(mp.mpf(float(best)) - p):
            best = cand
    return mp.mpf(float(best))


def reprojection_exact(obs, X, Ks, R, t, f32_rounding):
    """helpers.py:214-241 exactly: the mean over the 2 v components of (obs - project(X))^2, with cv.projectPoints'
    `z = z ? 1/z : 1` and, when f32_rounding, X rounded to float32 before and the pixel after the projection.
    -> (error float64, smallest relative distance of an exact projection from a float32 rounding tie; 1.0 without
    rounding), or None when fewer than two cameras see the point."""
    seen = _seen(obs)
    if len(seen) <= 1:
        return None
    X = np.asarray(X, dtype=np.float64)
    if f32_rounding:
        X = X.astype(np.float32).astype(np.float64)
    with mp.workdps(DPS):
        Xm = [mp.mpf(float(v)) for v in X]
        total, tie = mp.mpf(0), 1.0
        for j, c in enumerate(seen):
            Rc = np.asarray(R[c], dtype=np.float64)
            tc = np.asarray(t[c], dtype=np.float64).reshape(3)
            cam = [sum(mp.mpf(float(Rc[i, k])) * Xm[k] for k in range(3)) + mp.mpf(float(tc[i])) for i in range(3)]
            z = 1 / cam[2] if cam[2] != 0 else mp.mpf(1)
            K = np.asarray(Ks[j], dtype=np.float64)
            pu = cam[0] * z * mp.mpf(float(K[0, 0])) + mp.mpf(float(K[0, 2]))
            pv = cam[1] * z * mp.mpf(float(K[1, 1])) + mp.mpf(float(K[1, 2]))
            if f32_rounding:
                tie = min(tie, _f32_tie_distance(pu), _f32_tie_distance(pv))
                pu, pv = _round_f32(pu), _round_f32(pv)
            total += (mp.mpf(float(obs[c][0])) - pu) ** 2 + (mp.mpf(float(obs[c][1])) - pv) ** 2
        return _f64(total / (2 * len(seen))), tie


# ----------------------------------------------------------------------------- the loop of smallest_eigvec4 in NumPy
MAX_FACTORISATIONS = 32        # kMaxFactorisations of csrc/mocap_device.hpp (8 before the per-sample tests of the core)


def numpy_model_eigvec4(a, lamcut=np.inf, cap=MAX_FACTORISATIONS):
    """smallest_eigvec4 (csrc/mocap_device.hpp) in plain float64 NumPy: the same loop, cut, convergence test, pivot clamp
    and Laguerre step (sqrt and division where the device takes raw estimates; no fma); cap: factorisations at most.
    -> (vec [4], lam_lb, number of factorisations), or (None, None, 1) when the first factorisation cuts the candidate."""
    a = np.asarray(a, dtype=np.float64)
    tr = (a[0] + a[4]) + (a[7] + a[9])
    fl = tr * 1e-30 + 1e-300
    lam, nfac = 0.0, 0
    with np.errstate(all="ignore"):
        for it in range(cap):
            nfac += 1
            r0 = 1 / np.sqrt(max(a[0] - lam, fl))
            l10, l20, l30 = a[1] * r0, a[2] * r0, a[3] * r0
            r1 = 1 / np.sqrt(max(a[4] - lam - l10 * l10, fl))
            l21, l31 = (a[5] - l20 * l10) * r1, (a[6] - l30 * l10) * r1
            r2 = 1 / np.sqrt(max(a[7] - lam - l20 * l20 - l21 * l21, fl))
            l32 = (a[8] - l30 * l20 - l31 * l21) * r2
            piv3 = max(a[9] - lam - l30 * l30 - l31 * l31 - l32 * l32, fl)
            r3 = 1 / np.sqrt(piv3)
            m10, m21, m32 = -(l10 * r0) * r1, -(l21 * r1) * r2, -(l32 * r2) * r3
            m20 = -(l21 * m10 + l20 * r0) * r2
            m31 = -(l32 * m21 + l31 * r1) * r3
            m30 = -(l32 * m20 + l31 * m10 + l30 * r0) * r3
            M = np.array([[r0, 0, 0, 0], [m10, r1, 0, 0], [m20, m21, r2, 0], [m30, m31, m32, r3]])
            W = M.T @ M
            s1 = np.trace(W)
            if it == 0 and s1 * (2e-12 * tr + lamcut) < 1.0:
                return None, None, 1
            s1_last, lam_last = s1, lam
            s2 = (W * W).sum()
            if not (s1 * s1 - s2 > 1e-3 * s1 * s1):
                break
            disc = max(3 * (4 * s2 - s1 * s1), 1e-300)
            lam = lam + (4 - 2.0 ** -18) / (s1 + np.sqrt(disc))
        x = M[3].copy()
        for _ in range(4):
            x = M.T @ ((M @ x) * piv3)
    return x, lam_last + (1 - 1e-5) / s1_last - 2e-12 * tr, nfac


# ----------------------------------------------------------------------------- test matrices
STRATA = ["generic", "ill_separated", "exhaustion", "near_singular", "two_tiny", "clustered", "spread", "dlt"]
N_PER_STRATUM = 150            # blocks of 64, 64 and 22 lanes


def _spd(rng, eigs):
    Q, _ = np.linalg.qr(rng.standard_normal((4, 4)))
    B = (Q * np.asarray(eigs, dtype=np.float64)) @ Q.T
    return (B + B.T) / 2


PIXEL_K = np.array([[1400.0, 0, 640], [0, 1400.0, 360], [0, 0, 1]])


def _look_at(pos, target):
    z = target - pos
    z = z / np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x = x / np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def dlt_group(rng, views, noise, far=1.0, baseline=None):
    """The float64 DLT matrix (rows and sum as csrc/mocap_device.hpp builds them) of one point seen by `views` pixel-scale
    cameras (f = 1400, principal point (640, 360)) on a ring of radius 4 looking at the origin, observations rounded to
    float32.  baseline: the second camera sits this far from the first and looks the same way (two-view groups only)."""
    X = np.append(rng.uniform(-1, 1, 3) * far, 1.0)
    B = np.zeros((4, 4))
    first = None
    for c in range(views):
        ang = rng.uniform(0, 2 * np.pi)
        pos = np.array([4 * np.cos(ang), 4 * np.sin(ang), rng.uniform(0.5, 2.5)])
        R = _look_at(pos, rng.uniform(-0.3, 0.3, 3))
        if baseline is not None and c == 1:
            R, pos = first[0], first[1] + first[0][0] * baseline       # moved along the first camera's x axis
        if first is None:
            first = (R, pos)
        P = PIXEL_K @ np.c_[R, -R @ pos]
        p = P @ X
        u = float(np.float32(p[0] / p[2] + noise * rng.standard_normal()))
        v = float(np.float32(p[1] / p[2] + noise * rng.standard_normal()))
        ra, rb = v * P[2] - P[1], P[0] - u * P[2]
        B = B + (np.outer(ra, ra) + np.outer(rb, rb))
    return B


DLT_KINDS = [("2 views, 0.5 px noise", 2, 0.5, 1.0), ("2 views, noise-free", 2, 0.0, 1.0), ("8 views, noise-free", 8, 0.0, 1.0),
             ("8 views, 50 px wrong blob", 8, 50.0, 1.0), ("3 views, point 1e3 away", 3, 0.5, 1e3)]


@functools.lru_cache(maxsize=None)
def eig_strata(n=N_PER_STRATUM, seed=2024):
    """name -> float64 [n][4][4]: Q diag(lam) Q^T with random orthogonal Q, symmetrised (read-only, shared)."""
    rngs = {name: np.random.default_rng([seed, k]) for k, name in enumerate(STRATA)}      # one stream per stratum
    ratios = np.concatenate([[0.5, 0.999], rngs["ill_separated"].uniform(0.5, 0.999, n - 2)])

    def draw(name, eigs):
        return [_spd(rngs[name], eigs(i, rngs[name])) for i in range(n)]

    out = {
        "generic": draw("generic", lambda i, r: np.array([1e-2, 1, 2, 5]) * 10 ** r.uniform(-3, 8)),
        "ill_separated": draw("ill_separated", lambda i, r: [ratios[i], 1, 3, 7]),
        "exhaustion": draw("exhaustion", lambda i, r: [1.0 if i % 2 == 0 else 1 - 1e-4, 1, 3, 7]),
        "near_singular": draw("near_singular", lambda i, r: [10 ** -r.uniform(12, 20), 1, 3, 7]),
        "two_tiny": draw("two_tiny", lambda i, r: [1e-18, 1e-17, 3, 7]),
        "clustered": draw("clustered", lambda i, r: 1 + 1e-6 * r.standard_normal(4)),
        "spread": draw("spread", lambda i, r: [1, 1e5, 1e10, 1e16]),
        "dlt": [dlt_group(rngs["dlt"], *DLT_KINDS[i % len(DLT_KINDS)][1:]) for i in range(n)],
    }
    out = {k: np.array(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def two_view_groups(n=N_PER_STRATUM, seed=77):
    """Partial DLT groups of exactly two views: even samples two cameras of the ring, odd samples two cameras 1 cm apart
    looking the same way (the depth is all but unobservable: lam1 is tiny against the trace)."""
    rng = np.random.default_rng(seed)
    out = np.array([dlt_group(rng, 2, 0.5, baseline=None if i % 2 == 0 else 0.01) for i in range(n)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def exact_of(name):
    """[(lam, v, gap)] of the stratum `name` of eig_strata, or of "two_view" (computed once per process)."""
    Bs = two_view_groups() if name == "two_view" else eig_strata()[name]
    return [eig4_exact(B) for B in Bs]


def eigh_yardstick(name):
    """numpy.linalg.eigh on the stratum against the exact values -> (max backward error, max vector error x gap over the
    samples with gap >= GAP_MIN, share of samples below GAP_MIN)."""
    Bs = eig_strata()[name]
    back = vec = 0.0
    below = 0
    for B, (lam, v, gap) in zip(Bs, exact_of(name)):
        w, V = np.linalg.eigh(B)
        x = V[:, 0]
        back = max(back, backward_error(B, x, lam))
        if gap >= GAP_MIN:
            vec = max(vec, vector_error(x, v) * gap)
        else:
            below += 1
    return back, vec, below / len(Bs)


# ----------------------------------------------------------------------------- inputs of the public-API comparison
API_CAMERAS = [2, 3, 5, 6, 7, 9, 13]
API_POINTS = 150
TIE_MIN = 2.0 ** -40


@functools.lru_cache(maxsize=None)
def api_case(C, per_camera_K):
    """synth.ring_rig(C) (per_camera_K: synth.calibrated_ring_rig) with API_POINTS noisy points: point i keeps i % (C + 1)
    of its views, so every view count from 0 to C occurs.  -> (rig, obs [N][C][2] NaN-coded, given points [N][3])."""
    from mocap_core import synth
    rig = synth.calibrated_ring_rig(C, seed=3) if per_camera_K else synth.ring_rig(C)
    obs, X0 = synth.make_ba_observations(rig, API_POINTS, seed=100 + C, noise_px=0.3, dropout=0.0, half_extent=0.4)
    rng = np.random.default_rng([C, int(per_camera_K)])
    for i in range(API_POINTS):
        seen = _seen(obs[i])
        keep = min(len(seen), i % (C + 1))
        for c in rng.permutation(seen)[keep:]:
            obs[i, c] = np.nan
    obs.setflags(write=False)
    X0.setflags(write=False)
    return rig, obs, X0


@functools.lru_cache(maxsize=None)
def api_points_exact(C, per_camera_K):
    """[triangulate_exact(...)] of api_case's observations, and the yardstick: the largest (relative error x gap) of
    mocap_oracle.triangulate_point (NumPy / LAPACK) against it.  Relative error = |dX| / |(X, 1)|."""
    from . import mocap_oracle
    rig, obs, _ = api_case(C, per_camera_K)
    exact = [triangulate_exact(o, rig["K"], rig["R"], rig["t"]) for o in obs]
    worst = 0.0
    for o, e in zip(obs, exact):
        X = mocap_oracle.triangulate_point(o, rig["K"], rig["R"], rig["t"])
        assert (X is None) == (e is None)
        if e is not None:
            worst = max(worst, point_error(X, e[0]) * e[1])
    return exact, worst


def point_error(X, X_exact):
    return float(np.linalg.norm(np.asarray(X) - X_exact) / np.sqrt(1.0 + X_exact @ X_exact))


def api_errors_exact(obs, pts, rig, f32_rounding):
    """[reprojection_exact(..., f32_rounding)] of the given points (None where a point is NaN or has fewer than two views),
    and the yardstick: the largest relative error of mocap_oracle.reprojection_error WITHOUT the float32 roundings against
    reprojection_exact without them, on the same observations and points."""
    from . import cv_restate, mocap_oracle
    args = (rig["K"], rig["R"], rig["t"])
    plain = [None if np.isnan(p[0]) else reprojection_exact(o, p, *args, False) for o, p in zip(obs, pts)]
    exact = plain if not f32_rounding else [None if e is None else reprojection_exact(o, p, *args, True)
                                            for o, p, e in zip(obs, pts, plain)]
    object_dtype = bool(np.isnan(obs).any())
    worst, saved = 0.0, cv_restate.F32_ROUNDING
    cv_restate.F32_ROUNDING = False
    try:
        for o, p, e in zip(obs, pts, plain):
            if e is not None:
                r = mocap_oracle.reprojection_error(o, p, *args, object_dtype=object_dtype)
                worst = max(worst, abs(r - e[0]) / e[0])
    finally:
        cv_restate.F32_ROUNDING = saved
    return exact, worst
