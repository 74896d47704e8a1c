"""One linearisation of the bundle adjustment (csrc/ba_kernels.hip) as a plain NumPy statement, no device:

  fd_parameter_sets   the n + 1 parameter vectors of SciPy's 2-point scheme and the steps dx it divides by
                      (scipy/optimize/_numdiff.py _compute_absolute_step / _dense_difference)
  linearise           residuals of those sets -> valid rows, J, scaled residual, loss terms, operation by operation as
                      the comment above `cauchy_terms` lists them (NumPy's promotion rules decide each precision)
  gram_exact          [J|fs]^T [J|fs] in long double and a DERIVED elementwise bound on what any float64 summation of the
                      same products may differ from it

The bound.  Each of the m products a_ki a_kj is rounded once (relative error <= u = 2^-53), and adding m numbers in ANY order
(a serial loop, 64-row partials through a 16-ary tree, the 4-deep accumulation inside a matrix-core instruction) errs by at
most gamma_(m-1) times the sum of their absolute values (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), so
the computed element is within gamma_m sum_k |a_ki a_kj| ~ m 2^-53 |A|^T|A| of the exact one.  B = m 2^-52 |A|^T|A| is twice
that: the factor 2 pays for a matrix-core instruction whose internal order and intermediate roundings are not documented
(at most one more rounding per product).  The long-double reference itself (64-bit significand: products and sums each
rounded at 2^-64) is within (m + 1) 2^-64 |A|^T|A| of the truth, 2^-12 of B."""
import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, (
    "ba_linearise_reference needs an extended-precision np.longdouble (>= 64-bit significand) for its exact Gram matrix; "
    f"this platform's has {np.finfo(np.longdouble).nmant + 1} bits")

EPS64 = float(np.finfo(np.float64).eps)
REL_STEP_F64 = float(np.sqrt(np.finfo(np.float64).eps))
# float32 residuals: SciPy takes the root of the float32 epsilon AND rounds it in float32 (csrc/ba_solve.hip, ba_linearize)
REL_STEP_F32 = float(np.sqrt(np.float32(np.finfo(np.float32).eps)))


def rel_step_for(f32):
    return REL_STEP_F32 if f32 else REL_STEP_F64


def fd_parameter_sets(x0, rel_step):
    """-> (sets [n + 1][n], dx [n]): sets[0] = x0, sets[1 + j] = x0 with entry j moved by
    h_j = rel_step * sign(x_j) * max(1, |x_j|), sign(+-0) = +1; dx_j = (x_j + h_j) - x_j, what the difference is divided by."""
    x0 = np.array(x0, dtype=np.float64).reshape(-1)
    sign = np.where(x0 >= 0.0, 1.0, -1.0)              # -0.0 >= 0.0 is true: +1
    h = rel_step * sign * np.maximum(1.0, np.abs(x0))
    x1 = x0 + h
    dx = x1 - x0
    sets = np.tile(x0, (x0.size + 1, 1))
    sets[np.arange(1, x0.size + 1), np.arange(x0.size)] = x1
    return sets, dx


def linearise(r_sets, dx, f32, cauchy):
    """r_sets [n + 1][N] float64 residuals of fd_parameter_sets' vectors, NaN = the point is dropped (fewer than two views).
    -> dict(rows: indices of the valid points in order, J [m][n] float64, fs [m] float64 (the scaled residual; float32 values in
    the float32 flow), f [m] the residual as the optimizer sees it, rho0 [m] loss values, jscale [m], cost = 0.5 sum rho0 in
    long double)."""
    r_sets = np.asarray(r_sets, dtype=np.float64)
    dx = np.asarray(dx, dtype=np.float64)
    n = dx.size
    assert r_sets.ndim == 2 and r_sets.shape[0] == n + 1
    rows = np.nonzero(~np.isnan(r_sets[0]))[0]
    r = r_sets[:, rows]
    assert not np.isnan(r).any(), "a point is dropped in one parameter set and kept in another"
    if f32:
        r32 = r.astype(np.float32)
        f = r32[0]
        df = r32[1:] - f[None, :]                                  # float32 - float32 -> float32
        assert df.dtype == np.float32
        J = (df.astype(np.float64) / dx[:, None]).T              # float32 array / float64 step -> float64
        z = f * f                                                  # float32
        assert z.dtype == np.float32
        if cauchy:
            t = np.float32(1.0) + z
            rho1 = np.float32(1.0) / t
            rho2 = np.float32(-1.0) / (t * t)
            assert rho1.dtype == np.float32 and rho2.dtype == np.float32
            rho0 = np.log1p(z.astype(np.float64)).astype(np.float32).astype(np.float64)   # float32 log1p, correctly rounded
            js = rho1.astype(np.float64) + (2.0 * rho2.astype(np.float64)) * z.astype(np.float64)
            js = np.sqrt(np.maximum(js, EPS64))
            fs = (f.astype(np.float64) * (rho1.astype(np.float64) / js)).astype(np.float32).astype(np.float64)
        else:
            rho0 = z.astype(np.float64)
            js = np.ones(rows.size)
            fs = f.astype(np.float64)
        f = f.astype(np.float64)
    else:
        f = r[0]
        J = ((r[1:] - f[None, :]) / dx[:, None]).T
        z = f * f
        if cauchy:
            t = 1.0 + z
            rho1 = 1.0 / t
            rho2 = -1.0 / (t * t)
            rho0 = np.log1p(z)
            js = np.sqrt(np.maximum(rho1 + 2.0 * rho2 * z, EPS64))
            fs = f * (rho1 / js)
        else:
            rho0 = z.copy()
            js = np.ones(rows.size)
            fs = f.copy()
    J = np.ascontiguousarray(J * js[:, None])                      # (df / dx) * J_scale
    cost = np.longdouble(0.5) * np.sum(rho0.astype(np.longdouble))
    return {"rows": rows, "J": J, "fs": fs, "f": f, "rho0": rho0, "jscale": js, "cost": cost}


def gram_exact(J, fs):
    """-> (G, B): G = [J|fs]^T [J|fs] in long double [(n+1)][(n+1)], B = m 2^-52 |[J|fs]|^T |[J|fs]| (float64), the bound of the
    module docstring.  J^T J = G[:n, :n], J^T fs = G[:n, n]."""
    J = np.asarray(J, dtype=np.float64)
    fs = np.asarray(fs, dtype=np.float64).reshape(-1)
    assert J.ndim == 2 and J.shape[0] == fs.size
    m = J.shape[0]
    A = np.concatenate([J, fs[:, None]], axis=1).astype(np.longdouble)
    G = A.T @ A
    absA = np.abs(A)
    B = (np.longdouble(m) * np.longdouble(2.0) ** -52 * (absA.T @ absA)).astype(np.float64)
    return G, B


def tree_gram(A, rows_per_leaf=64, fan=16):
    """A^T A in float64 the way the one-launch kernel orders it: partial products of `rows_per_leaf` rows, then a `fan`-ary tree
    that adds each node's records in order.  (An honest order for the CPU check of the bound; not the kernel's bits.)"""
    A = np.asarray(A, dtype=np.float64)
    recs = [A[k:k + rows_per_leaf].T @ A[k:k + rows_per_leaf] for k in range(0, A.shape[0], rows_per_leaf)]
    if not recs:
        return np.zeros((A.shape[1], A.shape[1]))
    while len(recs) > 1:
        nxt = []
        for k in range(0, len(recs), fan):
            s = np.zeros_like(recs[0])
            for rec in recs[k:k + fan]:
                s = s + rec
            nxt.append(s)
        recs = nxt
    return recs[0]
