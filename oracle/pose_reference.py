"""TEST INFRASTRUCTURE ONLY (oracle/) -- never imported by the product path.

High-precision (mpmath, 50 digits) references of the three device routines of the initial pose estimation
(csrc/pose_kernels.hpp), one sample / one polynomial / one model at a time:

    seven_point_exact   the fundamental matrices of seven correspondences, and the sample's root gap
    cubic_exact         the distinct real roots of a polynomial of degree <= 3
    score_exact         FMEstimatorCallback::computeError's inlier decision per correspondence

They share no formula with the kernels or with cv_pose_restate.py beyond the definitions: the 7 x 9 system is built
from the raw coordinates (no Hartley normalisation: at 50 digits its conditioning does not matter), its null space comes
from an elimination in mpmath, the cubic det(l f1 + (1 - l) f2) from interpolation of four determinants, its roots
from mpmath.polyroots.

THE GAP RULE.  How many of the cubic's roots are real is a discontinuous function of the sample: where two roots
(nearly) coincide, rounding decides between one model and three, and the matrices move by (rounding error) / gap.
`gap` is the smallest relative distance |r_i - r_j| / max(|r_i|, |r_j|) between two roots of the cubic (for a complex
pair that is its imaginary part, doubled), with f1, f2 an orthonormal basis.  It is the condition number of the root count:
a comparison against this reference asserts counts where gap >= GAP_MIN and scales its tolerance by 1 / gap.
"""
import mpmath as mp
import numpy as np

DPS = 50
GAP_MIN = 1e-6


def _null_space(A):
    """Orthonormal basis (two mp vectors of 9) of the null space of the 7 x 9 mp matrix A; None when rank < 7."""
    M = [[A[r][c] for c in range(9)] for r in range(7)]
    perm = list(range(9))
    scale = max(abs(v) for row in M for v in row)
    for k in range(7):
        best, pr, pc = mp.mpf(-1), k, k
        for r in range(k, 7):
            for c in range(k, 9):
                if abs(M[r][c]) > best:
                    best, pr, pc = abs(M[r][c]), r, c
        if not best > scale * mp.mpf(10) ** (-(DPS - 10)):
            return None
        M[k], M[pr] = M[pr], M[k]
        if pc != k:
            for r in range(7):
                M[r][k], M[r][pc] = M[r][pc], M[r][k]
            perm[k], perm[pc] = perm[pc], perm[k]
        ip = 1 / M[k][k]
        M[k] = [v * ip for v in M[k]]
        for r in range(7):
            if r != k and M[r][k] != 0:
                f = M[r][k]
                M[r] = [a - f * b for a, b in zip(M[r], M[k])]
    basis = []
    for free in (7, 8):
        v = [mp.mpf(0)] * 9
        for i in range(7):
            v[perm[i]] = -M[i][free]
        v[perm[free]] = mp.mpf(1)
        basis.append(v)
    f1, f2 = basis
    n1 = mp.sqrt(sum(a * a for a in f1))
    f1 = [a / n1 for a in f1]
    d = sum(a * b for a, b in zip(f1, f2))
    f2 = [b - d * a for a, b in zip(f1, f2)]
    n2 = mp.sqrt(sum(a * a for a in f2))
    return f1, [a / n2 for a in f2]


def _det3(g):
    return (g[0] * (g[4] * g[8] - g[5] * g[7]) - g[1] * (g[3] * g[8] - g[5] * g[6]) + g[2] * (g[3] * g[7] - g[4] * g[6]))


def _roots(coeffs):
    """All complex roots of the polynomial (highest power first, leading coefficient non-zero)."""
    if len(coeffs) < 2:
        return []
    return mp.polyroots(coeffs, maxsteps=500, extraprec=4 * mp.mp.prec)


def seven_point_exact(ms1, ms2):
    """(7, 2) and (7, 2) image points -> (models, gap): the list of 3 x 3 float64 matrices F with x2^T F x1 = 0 on the
    seven points, det F = 0 and F[2][2] = 1, sorted by F[0][0]; gap as in the module header (inf with fewer than two
    roots).  A sample whose system has rank < 7 gives ([], 0.0)."""
    with mp.workdps(DPS):
        p1 = [[mp.mpf(float(v)) for v in row] for row in np.asarray(ms1)]
        p2 = [[mp.mpf(float(v)) for v in row] for row in np.asarray(ms2)]
        A = [[x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, mp.mpf(1)] for (x0, y0), (x1, y1) in zip(p1, p2)]
        ns = _null_space(A)
        if ns is None:
            return [], 0.0
        f1, f2 = ns

        def p(lam):
            return _det3([lam * a + (1 - lam) * b for a, b in zip(f1, f2)])

        # the cubic through four of its values
        p0, pp, pm, p2v = p(mp.mpf(0)), p(mp.mpf(1)), p(mp.mpf(-1)), p(mp.mpf(2))
        c3 = p0
        c1 = (pp + pm) / 2 - c3
        s = (pp - pm) / 2
        c0 = (p2v - 4 * c1 - c3 - 2 * s) / 6
        c2 = s - c0
        coeffs = [c0, c1, c2, c3]
        top = max(abs(c) for c in coeffs)
        while coeffs and abs(coeffs[0]) < top * mp.mpf(10) ** (-(DPS - 10)):
            coeffs.pop(0)                        # a root at infinity: F = f1 - f2, which no solver returns
        roots = _roots(coeffs)
        gap = mp.inf
        for i in range(len(roots)):
            for j in range(i):
                gap = min(gap, abs(roots[i] - roots[j]) / max(abs(roots[i]), abs(roots[j])))
        models = []
        for r in roots:
            if abs(mp.im(r)) > mp.mpf(10) ** (-(DPS // 2)) * max(1, abs(r)):
                continue
            lam = mp.re(r)
            g = [lam * a + (1 - lam) * b for a, b in zip(f1, f2)]
            g = [v / g[8] for v in g]
            models.append(np.array([float(v) for v in g]).reshape(3, 3))
        models.sort(key=lambda M: M[0, 0])
        return models, float(gap)


def cubic_exact(c):
    """Distinct real roots (ascending, float64) of c[0] x^3 + c[1] x^2 + c[2] x + c[3]; leading zeros reduce the degree,
    a multiple root counts once."""
    with mp.workdps(3 * DPS):                    # a triple root is found to a third of the digits
        coeffs = [mp.mpf(float(v)) for v in c]
        while coeffs and coeffs[0] == 0:
            coeffs.pop(0)
        roots = _roots(coeffs)
        size = max([abs(r) for r in roots] + [mp.mpf(0)])
        tol = size * mp.mpf(10) ** (-DPS // 2)
        real = sorted(mp.re(r) for r in roots if abs(mp.im(r)) <= tol)
        out = []
        for r in real:
            if not out or r - out[-1] > tol:
                out.append(r)
        return [float(r) for r in out]


def _sq_dist(d, a, b):
    """d^2 * (1 / (a^2 + b^2)) under IEEE rules: 1 / 0 = inf, 0 * inf = NaN."""
    den = a * a + b * b
    if den == 0:
        return mp.nan if d == 0 else mp.inf
    return d * d / den


def score_exact(m1, m2, F, t):
    """The inlier mask (bool, one per correspondence) of model F at threshold t = float32(thr * thr):
    err = float32(max(e1, e2)) <= t with std::max's operand order, (e1 < e2) ? e2 : e1 -- a NaN e1 stays, a NaN e2 loses."""
    m1, m2 = np.asarray(m1), np.asarray(m2)
    out = np.zeros(len(m1), dtype=bool)
    with mp.workdps(DPS):
        f = [mp.mpf(float(v)) for v in np.asarray(F, dtype=np.float64).ravel()]
        tt = mp.mpf(float(np.float32(t)))
        for i in range(len(m1)):
            x1, y1, x2, y2 = (mp.mpf(float(v)) for v in (m1[i, 0], m1[i, 1], m2[i, 0], m2[i, 1]))
            a, b, c = f[0] * x1 + f[1] * y1 + f[2], f[3] * x1 + f[4] * y1 + f[5], f[6] * x1 + f[7] * y1 + f[8]
            e2 = _sq_dist(x2 * a + y2 * b + c, a, b)
            a, b, c = f[0] * x2 + f[3] * y2 + f[6], f[1] * x2 + f[4] * y2 + f[7], f[2] * x2 + f[5] * y2 + f[8]
            e1 = _sq_dist(x1 * a + y1 * b + c, a, b)
            e = e2 if e1 < e2 else e1            # comparisons with NaN are false
            if mp.isnan(e):
                continue
            with mp.workprec(24):
                e32 = +e                         # the cast to float (values beyond float's range fail `<= t` either way)
            out[i] = bool(e32 <= tt)
    return out


def probe_point_set():
    """The fixed correspondences of the per-sample tests: cameras 0 and 1 of a three-camera ring, 200 points, 0.5 px noise,
    truncated to whole pixels as the reference's detector delivers them (float32 [n][2] each)."""
    from mocap_core import synth
    rig = synth.ring_rig(3)
    obs, _ = synth.make_ba_observations(rig, 200, seed=20, noise_px=0.5)
    obs = np.trunc(obs)
    a, b = obs[:, 0], obs[:, 1]
    ok = ~(np.isnan(a).any(axis=1) | np.isnan(b).any(axis=1))
    return a[ok].astype(np.float32), b[ok].astype(np.float32)


def probe_samples(p1, p2, count):
    """The first `count` distinct RANSAC subsets of cv::RNG((uint64)-1) on (p1, p2), as getSubset draws them: int32 [count][7]."""
    from oracle import cv_pose_restate as cp
    rng, seen, out = cp.RNG(), set(), []
    while len(out) < count:
        idx = cp.get_subset(p1, p2, rng)
        if tuple(sorted(idx)) not in seen:
            seen.add(tuple(sorted(idx)))
            out.append(idx)
    return np.array(out, dtype=np.int32)


def restatement_error(p1, p2, samples):
    """cv_pose_restate.run_7point (double precision, LAPACK's SVD) against seven_point_exact over `samples`: the
    reference's own yardstick.  Returns a dict:
        refs          per sample (models, gap) of seven_point_exact
        exempt        indices of the samples with gap < GAP_MIN (their root count is not asserted)
        count_equal   per sample: run_7point returns as many models as the reference
        err_gap       max over non-exempt samples and models of (max |F - F_ref| / max |F_ref|) * gap
        constraint    max |x2^T F x1| / max |F| of run_7point's models on their seven points
        det           max |det F| / max |F|^3 of run_7point's models"""
    from oracle import cv_pose_restate as cp
    refs, exempt, equal, err_gap, con, det = [], [], [], 0.0, 0.0, 0.0
    for s, idx in enumerate(samples):
        models, gap = seven_point_exact(p1[idx], p2[idx])
        got = cp.run_7point(p1[idx], p2[idx])
        refs.append((models, gap))
        equal.append(len(got) == len(models))
        if gap < GAP_MIN:
            exempt.append(s)
        elif equal[-1]:
            for A, B in zip(models, got):
                err_gap = max(err_gap, float(np.abs(A - B).max() / np.abs(A).max()) * gap)
        c, d = model_residuals(p1[idx], p2[idx], got)
        con, det = max(con, c), max(det, d)
    return {"refs": refs, "exempt": exempt, "count_equal": equal, "err_gap": err_gap, "constraint": con, "det": det}


def model_residuals(ms1, ms2, models):
    """(max |x2^T F x1| / max |F| over the seven points, max |det F| / max |F|^3) over `models` (0, 0 for none)."""
    h1 = np.c_[np.asarray(ms1, dtype=np.float64), np.ones(len(ms1))]
    h2 = np.c_[np.asarray(ms2, dtype=np.float64), np.ones(len(ms2))]
    con = det = 0.0
    for F in models:
        F = np.asarray(F, dtype=np.float64).reshape(3, 3)
        top = np.abs(F).max()
        con = max(con, float(np.abs(np.einsum("ni,ij,nj->n", h2, F, h1)).max() / top))
        det = max(det, float(abs(np.linalg.det(F)) / top ** 3))
    return con, det
