"""CPU: tests/ba_linearise_reference.py pinned against SciPy's own functions, and its Gram bound against honest and dishonest
float64 summations.  No device."""
import numpy as np
import pytest

import ba_linearise_reference as ref


# ---------------------------------------------------------------------------------------------------------------
# A smooth analytic residual function whose value at x0 is chosen entry by entry: r_i(x) = c_i + sin(b_i . (x - x0)).
X0 = np.array([0.0, -0.0, 534.25, -3.5, 1.0, -1.0, 0.37, -2.5e-4, 1e-9, 2.75])   # zeros of both signs, |x| > 1, |x| = 1, tiny
C0 = np.array([1e-6, 0.03, 0.25, 0.9, 0.999999, 1.0, 1.000001, 1.5, 3.0, 40.0, 0.5, 2.0])   # both sides of 1, one exactly 1.0


def _residual_function(dtype):
    rng = np.random.default_rng(5)
    Bm = rng.normal(0, 1.0, (C0.size, X0.size))
    seen = []

    def fun(x):
        seen.append(np.array(x, dtype=np.float64))
        return (C0 + np.sin(Bm @ (x - X0))).astype(dtype)
    return fun, seen


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("cauchy", [True, False])
def test_reference_is_scipys_own_linearisation(f32, cauchy):
    from scipy.optimize._lsq.common import scale_for_robust_loss_function
    from scipy.optimize._lsq.least_squares import construct_loss_function
    from scipy.optimize._numdiff import approx_derivative
    dtype = np.float32 if f32 else np.float64
    fun, seen = _residual_function(dtype)
    f0 = fun(X0)
    assert f0.dtype == dtype and (f0 == dtype(1.0)).sum() == 1 and (f0 < 1).sum() >= 4 and (f0 > 1).sum() >= 4
    del seen[:]
    J_sp = approx_derivative(fun, X0, method="2-point", f0=f0)
    # the parameter vectors SciPy evaluated are fd_parameter_sets' rows 1.., bit for bit (signed zeros included)
    sets, dx = ref.fd_parameter_sets(X0, ref.rel_step_for(f32))
    assert len(seen) == X0.size
    assert np.array_equal(np.array(seen), sets[1:]) and np.array_equal(sets[0], X0)
    assert np.array_equal(np.signbit(np.array(seen)), np.signbit(sets[1:]))
    assert (dx[:2] > 0).all() and dx[3] < 0 and dx[2] > 100 * dx[0]          # sign(+-0) = +1; max(1, |x|)
    r_sets = np.stack([fun(x).astype(np.float64) for x in sets])
    r_sets = np.insert(r_sets, 4, np.nan, axis=1)                             # one dropped point in the middle
    lin = ref.linearise(r_sets, dx, f32, cauchy)
    assert lin["rows"].tolist() == [0, 1, 2, 3] + list(range(5, C0.size + 1))
    if cauchy:
        rho = construct_loss_function(f0.size, "cauchy", 1.0)(f0)
        cost_sp = 0.5 * np.sum(rho[0])
        J_sp, f_sp = scale_for_robust_loss_function(J_sp, f0.copy(), rho)
        assert f_sp.dtype == dtype
        # exactly 1.0: rho1 + 2 rho2 z = 0.5 - 0.5 = 0 -> the EPS clamp; above 1 negative -> the clamp as well
        assert np.array_equal(lin["jscale"][C0 >= 1.0], np.full((C0 >= 1.0).sum(), np.sqrt(ref.EPS64)))
        assert (lin["jscale"][C0 < 0.99] > 1e-3).all()
    else:
        cost_sp, f_sp = 0.5 * np.dot(f0, f0), f0
        assert np.array_equal(lin["jscale"], np.ones(C0.size))
    assert J_sp.dtype == np.float64
    assert np.array_equal(lin["J"], J_sp)
    assert np.array_equal(lin["fs"], f_sp.astype(np.float64))
    # float32 log1p: the reference rounds correctly, NumPy's loop may differ in the last float32 bit; float64: summation order
    np.testing.assert_allclose(float(lin["cost"]), cost_sp, rtol=2e-7 if f32 else 1e-14)


def test_rel_steps():
    assert ref.REL_STEP_F64 == 2.0 ** -26
    assert ref.REL_STEP_F32 == float(np.float32(np.finfo(np.float32).eps) ** np.float32(0.5))
    assert ref.REL_STEP_F32 != float(np.finfo(np.float32).eps) ** 0.5 and abs(ref.REL_STEP_F32 / 2.0 ** -11.5 - 1) < 1e-7


# ---------------------------------------------------------------------------------------------------------------
M_BOUND, N_BOUND = 16_448, 16          # 257 chunks of 64 rows: a three-level 16-ary tree


@pytest.fixture(scope="module")
def heavy():
    rng = np.random.default_rng(11)
    A = rng.standard_t(3, size=(M_BOUND, N_BOUND + 1)) * np.exp(rng.normal(0, 2.0, (1, N_BOUND + 1)))   # heavy tails, column scales
    G, B = ref.gram_exact(A[:, :N_BOUND], A[:, N_BOUND])
    return A, G, B


def test_bound_admits_honest_float64_orders(heavy):
    A, G, B = heavy
    assert G.dtype == np.longdouble and G.shape == B.shape == (N_BOUND + 1, N_BOUND + 1) and (B > 0).all()
    worst = 0.0
    for got in (A.T @ A, ref.tree_gram(A)):
        ratio = (np.abs(got.astype(np.longdouble) - G) / B).max()
        worst = max(worst, float(ratio))
        assert ratio <= 1.0
    print(f"honest orders: largest error / B = {worst:.3g}")


def test_bound_rejects_a_dropped_chunk(heavy):
    A, G, B = heavy
    for k in (0, 100, 256):
        keep = np.ones(M_BOUND, bool)
        keep[64 * k:64 * k + 64] = False
        got = A[keep].T @ A[keep]
        excess = np.abs(got.astype(np.longdouble) - G) / B
        assert (excess > 1.0).all(), (k, float(excess.min()))
        assert excess.min() > 1e4


def test_gram_exact_small_case_by_hand():
    J = np.array([[1.0, 2.0], [3.0, -4.0]])
    fs = np.array([0.5, -0.25])
    G, B = ref.gram_exact(J, fs)
    assert np.array_equal(G.astype(np.float64), [[10.0, -10.0, -0.25], [-10.0, 20.0, 2.0], [-0.25, 2.0, 0.3125]])
    assert np.array_equal(B, 2 * 2.0 ** -52 * np.array([[10.0, 14.0, 1.25], [14.0, 20.0, 2.0], [1.25, 2.0, 0.3125]]))
