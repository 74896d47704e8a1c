"""The high-precision reference of the geometry core (oracle/geom_reference.py) is itself checked here, on the CPU: against
NumPy / LAPACK and the oracle's own restatement on well-conditioned inputs, and each stratum of test matrices against the
float64 model of smallest_eigvec4's loop, which proves that the stratum reaches the path it is named after.  The figures
printed here are the yardsticks tests/test_gpu_geom_kernels.py derives its tolerances from (its docstring records them)."""
import mpmath as mp
import numpy as np
import pytest

from oracle import geom_reference as gr
from oracle import mocap_oracle


def test_scalar_references_agree_with_numpy():
    rng = np.random.default_rng(1)
    a = rng.standard_normal(200) * 10 ** rng.uniform(-30, 30, 200)
    b = rng.standard_normal(200) * 10 ** rng.uniform(-30, 30, 200)
    for x, y in zip(a, b):
        assert gr.div_exact(x, y) == x / y                       # IEEE division is correctly rounded
        assert gr.recip_exact(y) == 1.0 / y
        d = abs(y)
        assert abs(gr.rsqrt_exact(d) - 1.0 / np.sqrt(d)) <= np.spacing(gr.rsqrt_exact(d))     # two roundings in NumPy's
        assert gr.ulp_distance(gr.rsqrt_exact(d), "rsqrt", d) <= 0.5
        assert gr.ulp_distance(x / y, "div", x, y) <= 0.5
    assert gr.rsqrt_exact(4.0) == 0.5 and gr.recip_exact(8.0) == 0.125 and gr.div_exact(1.0, 3.0) == 1.0 / 3.0
    assert gr.ulp_distance(np.nextafter(0.5, 1), "rsqrt", 4.0) == 1.0
    assert gr.fma(2.0 ** 27 + 1, 2.0 ** 27 + 1, -2.0 ** 54) == 2.0 ** 28 + 1       # the product's low bit survives


def test_matrix_references_agree_with_lapack():
    Bs = gr.eig_strata()["generic"][:40]
    for B, (lam, v, gap) in zip(Bs, gr.exact_of("generic")[:40]):
        w, V = np.linalg.eigh(B)
        assert np.allclose([float(x) for x in lam], w, rtol=1e-12)
        assert gr.vector_error(V[:, 0], v) < 1e-13 and gr.backward_error(B, V[:, 0], lam) < 1e-14
        assert abs(gap - (w[1] - w[0]) / w[3]) < 1e-12
        assert abs(float(gr.trace_inv_exact(B)) / np.trace(np.linalg.inv(B)) - 1) < 1e-12
        c = np.array([0.3, -2.0, 1.5])
        M = np.eye(4)
        M[:3, 3] = c
        S = gr.shifted_exact(B, c)
        assert np.allclose(np.array(S.tolist(), dtype=np.float64), M.T @ B @ M, rtol=1e-12, atol=1e-12 * np.trace(B))
    assert [gr.pack(gr.unpack(np.arange(10.0)))[k] for k in range(10)] == list(range(10))


def test_strata_reach_the_paths_they_are_named_after():
    S = gr.eig_strata()
    nfac = {name: np.array([gr.numpy_model_eigvec4(gr.pack(B))[2] for B in S[name]]) for name in gr.STRATA}
    nfac8 = {name: np.array([gr.numpy_model_eigvec4(gr.pack(B), cap=8)[2] for B in S[name]]) for name in ("ill_separated", "exhaustion")}
    assert np.all(nfac["generic"] == 2)
    assert np.all(nfac["near_singular"] == 1)
    # exhaustion: every sample uses up the 8 factorisations the loop had when these tests were written.  With today's 32
    # the half with lam1 / lam2 = 1 - 1e-4 converges at the tenth; the double eigenvalue climbs until rounding ends it
    # (28 or more: the clamped pivot, or the cap).
    assert np.all(nfac8["exhaustion"] == 8)
    assert np.all(nfac["exhaustion"][1::2] == 10) and np.all(nfac["exhaustion"][0::2] >= 24)
    # ill-separated: 3 to 7 factorisations below lam1 / lam2 = 0.9975; the last quarter per cent of the range (the end point
    # 0.999 among it) needs the eighth.  Every count from 3 to 7 occurs.
    ratio = np.array([float(lam[0] / lam[1]) for lam, _, _ in gr.exact_of("ill_separated")])
    assert ratio.min() == pytest.approx(0.5, abs=1e-12) and ratio.max() == pytest.approx(0.999, abs=1e-12)
    assert np.array_equal(nfac["ill_separated"], nfac8["ill_separated"])
    assert np.all((nfac["ill_separated"] >= 3) & (nfac["ill_separated"] <= 8))
    assert np.all(nfac["ill_separated"][ratio < 0.9975] <= 7) and np.mean(nfac["ill_separated"] <= 7) >= 0.98
    assert set(range(3, 8)) <= set(nfac["ill_separated"].tolist())
    print("\nfactorisations per stratum (float64 model): " + ", ".join(f"{k} {v.min()}..{v.max()}" for k, v in nfac.items()))
    # the model's own lam_lb is a lower bound everywhere, also where the loop runs out (cap = 8 on the exhaustion stratum)
    for name in gr.STRATA:
        for B, (lam, _, _) in zip(S[name], gr.exact_of(name)):
            assert mp.mpf(gr.numpy_model_eigvec4(gr.pack(B))[1]) <= lam[0], name
            if name == "exhaustion":
                assert mp.mpf(gr.numpy_model_eigvec4(gr.pack(B), cap=8)[1]) <= lam[0]
    # the cut: a candidate whose lam1 is far above lamcut is dropped after one factorisation
    assert gr.numpy_model_eigvec4(gr.pack(S["generic"][0]), 0.0)[0] is None


def test_eigh_yardsticks_and_gap_caps():
    print()
    for name in gr.STRATA:
        back, vec, below = gr.eigh_yardstick(name)
        print(f"numpy.linalg.eigh vs exact, {name:14s}: backward error {back:.2e}, vector error x gap {vec:.2e}, "
              f"below the gap {100 * below:.1f} %")
        assert 0 < back < 2e-15 and vec < 2e-15
        # exhaustion, two_tiny and clustered are degenerate on purpose; the spread stratum's gap is (1e5 - 1) / 1e16 by
        # construction: its vector is judged by the backward error alone
        if name not in ("exhaustion", "two_tiny", "clustered", "spread"):
            assert below <= 0.02, name


@pytest.mark.parametrize("per_camera_K", [False, True])
@pytest.mark.parametrize("C", [2, 5, 9])
def test_api_references_agree_with_the_restatement(C, per_camera_K):
    rig, obs, X0 = gr.api_case(C, per_camera_K)
    views = (~np.isnan(obs[:, :, 0])).sum(axis=1)
    assert set(views.tolist()) == set(range(C + 1))              # every view count, 0 and 1 included
    exact, yard = gr.api_points_exact(C, per_camera_K)
    assert all((e is None) == (v < 2) for e, v in zip(exact, views))
    assert 0 < yard < 1e-13
    line = f"\nC = {C}, per-camera K = {per_camera_K}: triangulate_point vs exact, relative error x gap = {yard:.2e}"
    for f32 in (False, True):
        ex, y = gr.api_errors_exact(obs, X0, rig, f32)
        ties = sum(1 for e in ex if e is not None and e[1] < gr.TIE_MIN)
        assert ties <= 0.02 * len(obs)
        assert 0 < y < 1e-11
        line += f"; reprojection_error without float32 roundings, relative error {y:.2e}" if not f32 else ""
        line += f"; f32_rounding = {f32}: {ties} points near a float32 tie"
    print(line)


def test_reprojection_exact_depth_zero_takes_the_z_equals_one_branch():
    K = np.array([[300.0, 0, 160], [0, 300.0, 120], [0, 0, 1]])
    R = np.array([np.eye(3), np.eye(3)])
    t = np.array([[0.0, 0, 0], [0.5, 0, 2.0]])
    X = np.array([0.25, -0.5, 0.0])
    obs = np.array([[235.0, -30.0], [272.5, 45.0]])
    # camera 0: z = 0 -> z := 1 -> pixel (0.25 * 300 + 160, -0.5 * 300 + 120) = (235, -30); camera 1: (0.75, -0.5, 2) ->
    # (272.5, 45): both residuals vanish
    for f32 in (False, True):
        err, _ = gr.reprojection_exact(obs, X, [K, K], R, t, f32)
        assert err == 0.0
        assert mocap_oracle.reprojection_error(obs, X, [K, K], R, t) == 0.0
    assert gr.reprojection_exact(np.array([[1.0, 2.0], [np.nan, np.nan]]), X, [K, K], R, t, True) is None
    assert gr.triangulate_exact(np.array([[1.0, 2.0], [np.nan, np.nan]]), [K, K], R, t) is None
