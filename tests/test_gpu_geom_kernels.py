"""The FP64 geometry core (csrc/mocap_device.hpp: rsqrt_pos, recip_refined, div_by, smallest_eigvec4, eigcut_s1,
eigcut_s1_shifted, solve_point, and score_point / reproject_sq through the public API), one sample at a time, against the
50-digit references of oracle/geom_reference.py -- the rest of the suite sees the core only through whole frames and through
core.triangulate on well-separated data, where every lane takes exactly two factorisations.  The device functions are
reached through the test-only probe tests/native/libmocap_geomprobe.so, which includes the product's header.

WHERE THE TOLERANCES COME FROM.  Claims the code makes are asserted as made: div_by bit-equal to IEEE division, rsqrt_pos
and recip_refined within 1 ulp of the exact value, lam_lb and 1/s1 - 2e-12 tr below the exact lam1 with NO tolerance (the
functions charge their own allowance).  Everything else is 16 x the distance of a correct double-precision implementation
(NumPy / LAPACK, the oracle's restatement) from the exact value ON THE SAME INPUTS, floor 4 ulp = 8.9e-16, recomputed in each
test (tests/test_geom_reference_cpu.py prints the same figures).  A wrong sign or a dropped term gives 1e-3 .. 1.

Yardsticks (numpy.linalg.eigh against exact, 150 matrices per stratum) and, next to them, smallest_eigvec4 on an MI355X:

    stratum         backward error           vector error x gap       below the gap   factorisations (float64 model)
                    eigh       device        eigh       device
    generic         3.93e-16   1.94e-16      2.06e-16   7.21e-17        0 %           2
    ill_separated   4.45e-16   1.46e-16      1.62e-16   3.21e-17        0 %           3..8 (8 only above lam1/lam2 = 0.9975)
    exhaustion      3.69e-16   4.92e-16      1.71e-16   2.49e-17       50 %           10 (lam1/lam2 = 1 - 1e-4), >= 24 (double eigenvalue); 8 = all there were until this test
    near_singular   3.99e-16   4.39e-16      2.56e-16   4.13e-16        0 %           1
    two_tiny        3.33e-16   2.14e-15      --         --            100 %           1..32
    clustered       6.31e-16   4.11e-17      4.07e-16   2.97e-22       73 %           3..8
    spread          3.04e-16   2.80e-16      --         --            100 %           1
    dlt             4.26e-16   1.79e-16      2.46e-16   1.05e-16        0 %           1..2

The gap rule (oracle/geom_reference.py): vector errors are compared where gap = (lam2 - lam1) / lam4 >= 1e-6; at most 2 % of
a stratum may fall below, except the strata that are degenerate on purpose (exhaustion, two_tiny, clustered) and `spread`,
whose gap is (1e5 - 1) / 1e16 by construction: there the vector is judged by its backward error alone.

Measured on an MI355X besides the table:
    div_by            0 of 250 quotients differ from IEEE division
    recip_refined     max 0.500 ulp: every one of the 250 correctly rounded
    rsqrt_pos         max 0.750 ulp (at d = 0x1.fffffffffffffp+851)
    lam_lb - lam1     <= -2.0e-12 x trace in every stratum, no sample above lam1
    eigcut            (1/s1 - 2e-12 tr - lam1) / tr <= -2.0e-12 everywhere; tr bit-equal to its formula (0 ulp); s1 relative error
                      3.0e-14 (np.trace(np.linalg.inv) 1.8e-14) on generic, 1.7e-11 (3.8e-11) on the 35 DLT matrices with cond <= 1e6
    solve_point       relative error x |v3| x gap 6.3e-17 (eigh's vector error x gap 2.5e-16)
    core.triangulate  relative error x gap <= 7.9e-17 over the 28 cases (triangulate_point 1.6e-16 .. 1.6e-15)
    errors            the restatement's own bits in all 28 cases (relative error against exact up to 9.3e-12 on triangulated points,
                      where the residuals cancel to 0.1 px; the same figure for the restatement); 2 cases drop one point near a tie

WHAT THIS TEST FOUND (on the device, header of the parent commit, stratum `exhaustion`).  With the loop's former 8 factorisations
lam_lb lay ABOVE the exact lam1 on all 150 samples, by up to 2.41e-6 x trace = 2.9e-5 x lam1 (the bound paired the advanced shift
with the s1 of the previous one), and the half with lam1 / lam2 = 1 - 1e-4 came back with a backward error of 9.2e-6: the loop ran
out before the shift separated the two eigenvalues and the inverse iteration returned a mixture of their vectors.  Fixed in
csrc/mocap_device.hpp (lam_last; kMaxFactorisations = 32); every other stratum is unchanged to the bit.
"""
import ctypes
import functools
import os

import mpmath as mp
import numpy as np
import pytest

from oracle import geom_reference as gr
from oracle import mocap_oracle

pytestmark = pytest.mark.gpu

N = gr.N_PER_STRATUM               # 150: blocks of 64, 64 and 22 lanes
FACTOR = 16.0
FLOOR = 4 * gr.ULP
FILL = -7.25
_vp = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(_vp)


def tolerance(yardstick):
    return max(FACTOR * yardstick, FLOOR)


@pytest.fixture(scope="module")
def probe(core):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "tests", "native", "libmocap_geomprobe.so")
    assert os.path.exists(path), "build it with `make -C tests/native` (__graft_entry__.build does)"
    lib = ctypes.CDLL(path)
    for name, nargs in (("geomprobe_rsqrt", 2), ("geomprobe_recip", 2), ("geomprobe_div", 3), ("geomprobe_eigvec4", 5),
                        ("geomprobe_eigcut", 4), ("geomprobe_solve_point", 2)):
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [ctypes.c_int] + [_vp] * nargs
    return lib


def packed(Bs):
    return np.ascontiguousarray([gr.pack(B) for B in Bs])


def eigvec4(lib, Bs, lamcut):
    """-> vec [n][4], lam_lb [n], ok [n]; what the kernel does not write keeps FILL / -99."""
    a = packed(Bs)
    n = len(a)
    lamcut = np.ascontiguousarray(np.broadcast_to(lamcut, n), dtype=np.float64)
    vec, lam_lb, ok = np.full((n, 4), FILL), np.full(n, FILL), np.full(n, -99, dtype=np.int32)
    assert lib.geomprobe_eigvec4(n, _p(a), _p(lamcut), _p(vec), _p(lam_lb), _p(ok)) == 0
    assert np.all((ok == 0) | (ok == 1))
    return vec, lam_lb, ok


# ------------------------------------------------------------------------------------------- scalar primitives
def _edge_mantissas(rng, n, lo, hi):
    """n positive doubles with exponents in [lo, hi]: a quarter each powers of two, mantissa 0x000..1, mantissa 0xFFF..F, random."""
    e = rng.integers(lo, hi + 1, n)
    kind = np.arange(n) % 4
    frac = np.where(kind == 0, 0, np.where(kind == 1, 1, np.where(kind == 2, (1 << 52) - 1, rng.integers(0, 1 << 52, n))))
    return ((e + 1023).astype(np.uint64) << np.uint64(52) | frac.astype(np.uint64)).view(np.float64)


@functools.lru_cache(maxsize=None)
def div_operands():
    """250 pairs with operands AND quotient inside 2^-500 .. 2^500, both signs, the mantissa edges, a == b."""
    rng = np.random.default_rng(11)
    n = 250
    b = _edge_mantissas(rng, n, -499, 498)
    eb = np.floor(np.log2(b)).astype(int)
    ea = np.array([rng.integers(max(-499, e - 498), min(498, e + 498) + 1) for e in eb])     # |ea - eb| <= 498
    a = np.roll(_edge_mantissas(rng, n, 0, 0), 1) * 2.0 ** ea                                # another edge kind than b's
    a *= rng.choice([-1.0, 1.0], n)
    b *= rng.choice([-1.0, 1.0], n)
    a[::10] = b[::10]
    q = np.abs(a / b)
    assert np.all((np.abs(a) >= 2.0 ** -500) & (np.abs(a) <= 2.0 ** 500) & (np.abs(b) >= 2.0 ** -500) & (np.abs(b) <= 2.0 ** 500))
    assert np.all((q >= 2.0 ** -500) & (q <= 2.0 ** 500)) and np.sum(a == b) >= 10 and np.sum(a < 0) > 50 and np.sum(b < 0) > 50
    return a, b


def test_div_by_has_the_bits_of_ieee_division(probe):
    a, b = div_operands()
    out = np.full(len(a), FILL)
    assert probe.geomprobe_div(len(a), _p(a), _p(b), _p(out)) == 0
    wrong = np.flatnonzero(out != a / b)
    print(f"\ndiv_by vs IEEE division: {len(wrong)} of {len(a)} quotients differ")
    assert len(wrong) == 0, [(a[i].hex(), b[i].hex(), out[i].hex(), (a[i] / b[i]).hex()) for i in wrong[:5]]


def test_recip_refined_within_one_ulp(probe):
    _, b = div_operands()
    out = np.full(len(b), FILL)
    assert probe.geomprobe_recip(len(b), _p(b), _p(out)) == 0
    ulps = np.array([gr.ulp_distance(o, "recip", x) for o, x in zip(out, b)])
    print(f"\nrecip_refined vs exact: max {ulps.max():.3f} ulp, {np.sum(out != 1.0 / b)} of {len(b)} not correctly rounded")
    assert ulps.max() <= 1.0


def test_rsqrt_pos_within_one_ulp(probe):
    rng = np.random.default_rng(12)
    d = np.concatenate([_edge_mantissas(rng, 245, -900, 899), [2.0 ** 900, 2.0 ** -900]])
    assert d.min() >= 2.0 ** -900 and d.max() <= 2.0 ** 900
    # the pivot floor of the Cholesky factorisations: tr * 1e-30 + 1e-300 for tr -> 0, tr = 1 and tr = 1e14
    d = np.concatenate([d, [1e-300, 1.0 * 1e-30 + 1e-300, 1e14 * 1e-30 + 1e-300]])
    assert len(d) == 250
    out = np.full(len(d), FILL)
    assert probe.geomprobe_rsqrt(len(d), _p(d), _p(out)) == 0
    ulps = np.array([gr.ulp_distance(o, "rsqrt", x) for o, x in zip(out, d)])
    print(f"\nrsqrt_pos vs exact: max {ulps.max():.3f} ulp at d = {d[ulps.argmax()].hex()}")
    assert ulps.max() <= 1.0


# ------------------------------------------------------------------------------------------- smallest_eigvec4
_runs = {}


def eig_run(probe, name):
    """smallest_eigvec4 with lamcut = +inf on the stratum (one launch per stratum and session)."""
    if name not in _runs:
        out = eigvec4(probe, gr.eig_strata()[name], np.inf)
        for a in out:
            a.setflags(write=False)
        _runs[name] = out
    return _runs[name]


@pytest.mark.parametrize("name", gr.STRATA)
def test_eigvec4_vector_against_exact(probe, name):
    Bs, exact = gr.eig_strata()[name], gr.exact_of(name)
    vec, lam_lb, ok = eig_run(probe, name)
    assert np.all(ok == 1) and np.all(np.isfinite(vec)) and np.all(np.isfinite(lam_lb))
    y_back, y_vec, below = gr.eigh_yardstick(name)
    if name not in ("exhaustion", "two_tiny", "clustered", "spread"):
        assert below <= 0.02
    back = max(gr.backward_error(B, x, lam) for B, x, (lam, _, _) in zip(Bs, vec, exact))
    errs = [gr.vector_error(x, v) * gap for x, (_, v, gap) in zip(vec, exact) if gap >= gr.GAP_MIN]
    worst = max(errs) if errs else 0.0
    print(f"\nsmallest_eigvec4, {name}: backward error {back:.2e} (eigh {y_back:.2e}), vector error x gap {worst:.2e} "
          f"(eigh {y_vec:.2e}) over {len(errs)} of {len(Bs)} samples")
    assert back <= tolerance(y_back)
    assert worst <= tolerance(y_vec)


@pytest.mark.parametrize("name", gr.STRATA)
def test_eigvec4_lam_lb_is_a_lower_bound_and_not_a_useless_one(probe, name):
    Bs, exact = gr.eig_strata()[name], gr.exact_of(name)
    _, lam_lb, ok = eig_run(probe, name)
    assert np.all(ok == 1)
    with mp.workdps(gr.DPS):
        over = [float((mp.mpf(float(lb)) - lam[0]) / mp.mpf(float(np.trace(B)))) for B, lb, (lam, _, _) in zip(Bs, lam_lb, exact)]
        rel = [float((mp.mpf(float(lb)) - lam[0]) / abs(lam[0])) for lb, (lam, _, _) in zip(lam_lb, exact)]
        worst = int(np.argmax(over))
        print(f"\nlam_lb - lam1, {name}: max {over[worst]:.3e} x trace = {rel[worst]:.3e} x lam1; {sum(o > 0 for o in over)} of {len(Bs)} above lam1")
        for B, lb, (lam, _, _) in zip(Bs, lam_lb, exact):
            assert mp.mpf(float(lb)) <= lam[0]                       # no tolerance: the function charges its own allowance
        tight = 0
        for B, lb, (lam, _, gap) in zip(Bs, lam_lb, exact):
            if gap >= 1e-2:
                tight += 1
                # converged: 1/s1 is within ~1e-3 of lam1 - lam; the allowance takes 1e-5 relative plus 2e-12 tr
                assert mp.mpf(float(lb)) >= mp.mpf("0.99") * lam[0] - mp.mpf("4e-12") * mp.mpf(float(np.trace(B)))
    if name in ("generic", "near_singular"):
        assert tight == len(Bs)


@pytest.mark.parametrize("name", ["generic", "ill_separated", "dlt"])
def test_eigvec4_cut(probe, name):
    Bs, exact = gr.eig_strata()[name], gr.exact_of(name)
    vec_inf, lb_inf, _ = eig_run(probe, name)
    for factor in (0.5, 1.0, 1.0 + 1e-6, 2.0):
        with mp.workdps(gr.DPS):
            lamcut = np.array([float(lam[0] * mp.mpf(factor)) for lam, _, _ in exact])
            if factor == 1.0:                                      # the nearest double may lie below lam1: take the one above
                lamcut = np.array([c if mp.mpf(float(c)) >= lam[0] else np.nextafter(c, np.inf) for c, (lam, _, _) in zip(lamcut, exact)])
            must = np.array([mp.mpf(float(c)) >= lam[0] for c, (lam, _, _) in zip(lamcut, exact)])
        vec, lam_lb, ok = eigvec4(probe, Bs, lamcut)
        print(f"\ncut, {name}, lamcut = {factor} x lam1: {int(ok.sum())} of {len(Bs)} kept, {int(must.sum())} must be")
        assert np.all(ok[must] == 1)
        if factor >= 1.0 and name != "dlt":                        # (a noise-free DLT matrix may have lam1 <= 0)
            assert must.all()
        if name == "generic" and factor == 0.5:
            assert np.all(ok == 0)                                 # 1/s1 >= lam1 / 1.03 there
        cut = ok == 0
        assert np.all(vec[cut] == FILL) and np.all(lam_lb[cut] == FILL)      # a dropped candidate writes nothing
        assert vec[~cut].tobytes() == vec_inf[~cut].tobytes() and lam_lb[~cut].tobytes() == lb_inf[~cut].tobytes()


# ------------------------------------------------------------------------------------------- eigcut_s1 / eigcut_s1_shifted
def _tr_formula(a, c):
    """The code's own tr in float64 (correctly rounded fma where the code has one)."""
    f = gr.fma
    tra = (a[0] + a[4]) + (a[7] + a[9])
    if c is None:
        return tra
    b3 = f(a[0], c[0], f(a[1], c[1], f(a[2], c[2], a[3])))
    b6 = f(a[1], c[0], f(a[4], c[1], f(a[5], c[2], a[6])))
    b8 = f(a[2], c[0], f(a[5], c[1], f(a[7], c[2], a[8])))
    b9 = f(c[0], b3 + a[3], f(c[1], b6 + a[6], f(c[2], b8 + a[8], a[9])))
    c2 = f(c[0], c[0], f(c[1], c[1], f(c[2], c[2], 1.0)))
    return ((a[0] + a[4]) + (a[7] + b9)) + 2.0 * c2 * tra


@pytest.mark.parametrize("shift", [None, 0.0, 1.0, 30.0, 1e4])
@pytest.mark.parametrize("name", ["generic", "near_singular", "spread", "dlt", "two_view"])
def test_eigcut_bound_is_safe_and_accurate(probe, name, shift):
    Bs = gr.two_view_groups() if name == "two_view" else gr.eig_strata()[name]
    a = packed(Bs)
    rng = np.random.default_rng(int(shift or 0) + 5)
    c = None
    if shift is not None:
        c = rng.standard_normal((N, 3))
        c = np.ascontiguousarray(c / np.linalg.norm(c, axis=1)[:, None] * shift)
    s1, tr = np.full(N, FILL), np.full(N, FILL)
    assert probe.geomprobe_eigcut(N, _p(a), None if c is None else _p(c), _p(s1), _p(tr)) == 0
    assert np.all(np.isfinite(s1)) and np.all(s1 > 0) and np.all(np.isfinite(tr))
    worst_tr = worst_s1 = yard = 0.0
    worst_margin, checked = -np.inf, 0
    with mp.workdps(gr.DPS):
        for i in range(N):
            ci = None if c is None else c[i]
            want = _tr_formula(a[i], ci)
            worst_tr = max(worst_tr, abs(tr[i] - want) / np.spacing(abs(want)))
            Bm = gr.shifted_exact(Bs[i], ci if ci is not None else np.zeros(3))
            lam = gr.eig4_exact_mp(Bm)
            margin = (1 / mp.mpf(float(s1[i])) - mp.mpf("2e-12") * mp.mpf(float(tr[i])) - lam[0]) / mp.mpf(float(tr[i]))
            worst_margin = max(worst_margin, float(margin))
            assert margin <= 0, (name, shift, i)                   # no tolerance
            if lam[0] > 0 and lam[3] / lam[0] <= 1e6:
                checked += 1
                ref = gr.trace_inv_exact(Bm)
                worst_s1 = max(worst_s1, float(abs(mp.mpf(float(s1[i])) - ref) / ref))
                M = np.eye(4)
                if ci is not None:
                    M[:3, 3] = ci
                yard = max(yard, float(abs(mp.mpf(float(np.trace(np.linalg.inv(M.T @ Bs[i] @ M)))) - ref) / ref))
    print(f"\neigcut, {name}, shift {shift}: (1/s1 - 2e-12 tr - lam1) / tr <= {worst_margin:.3e}; tr within {worst_tr:.1f} ulp; "
          f"s1 relative error {worst_s1:.2e} (trace(inv) in NumPy {yard:.2e}) over {checked} samples with cond <= 1e6")
    assert worst_tr <= 4
    assert worst_s1 <= tolerance(yard)
    if name == "generic" and (shift is None or shift <= 1.0):
        assert checked > 0


# ------------------------------------------------------------------------------------------- solve_point
def test_solve_point_on_dlt_matrices(probe):
    """X = v[:3] / v[3]: with x = v + e, |e| <= T / gap, first order gives |dX| <= |e| |(X, 1)| / |v3|, i.e. the error relative to
    |(X, 1)| is the eigenvector tolerance over |v3|; the two roundings of div_by are below the 4 ulp floor of T."""
    Bs, exact = gr.eig_strata()["dlt"], gr.exact_of("dlt")
    X = np.full((N, 3), FILL)
    assert probe.geomprobe_solve_point(N, _p(packed(Bs)), _p(X)) == 0
    assert np.all(np.isfinite(X))
    _, y_vec, _ = gr.eigh_yardstick("dlt")
    worst = 0.0
    with mp.workdps(gr.DPS):
        for i, (lam, v, gap) in enumerate(exact):
            assert gap >= gr.GAP_MIN
            ref = [v[k] / v[3] for k in range(3)]
            err = mp.sqrt(sum((mp.mpf(float(X[i, k])) - ref[k]) ** 2 for k in range(3))) / mp.sqrt(1 + sum(r * r for r in ref))
            worst = max(worst, float(err * abs(v[3]) * gap))
    print(f"\nsolve_point vs exact: relative error x |v3| x gap = {worst:.2e} (eigh's vector error x gap {y_vec:.2e})")
    assert worst <= tolerance(y_vec)
    # the same arithmetic as smallest_eigvec4 followed by IEEE division
    vec, _, _ = eig_run(probe, "dlt")
    assert np.array_equal(X, vec[:, :3] / vec[:, 3:4])


# ------------------------------------------------------------------------------------------- through the public API
def _check_errors(err, obs, pts, rig, f32, what):
    exact, yard = gr.api_errors_exact(obs, pts, rig, f32)
    near_tie = [i for i, e in enumerate(exact) if e is not None and e[1] < gr.TIE_MIN]
    assert len(near_tie) <= 0.02 * len(obs)
    worst = 0.0
    for i, e in enumerate(exact):
        if e is None:
            assert np.isnan(err[i]), (what, i)
        elif i not in near_tie:
            assert np.isfinite(err[i]), (what, i)
            worst = max(worst, abs(err[i] - e[0]) / e[0])
    print(f"  {what}: relative error {worst:.2e} (restatement without roundings {yard:.2e}), {len(near_tie)} points near a float32 tie")
    assert worst <= tolerance(yard)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("per_camera_K", [False, True])
@pytest.mark.parametrize("C", gr.API_CAMERAS)
def test_triangulate_and_reproject_against_exact(core, C, per_camera_K, f32):
    rig, obs, X0 = gr.api_case(C, per_camera_K)
    views = (~np.isnan(obs[:, :, 0])).sum(axis=1)
    assert set(views.tolist()) == set(range(C + 1))
    exact, yard = gr.api_points_exact(C, per_camera_K)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.set_options(f32_rounding=f32)
    try:
        xyz, err = core.triangulate(obs)
        err_given = core.reproject(obs, X0)
    finally:
        core.set_options(f32_rounding=True)
    worst = 0.0
    for i, e in enumerate(exact):
        if e is None:
            assert np.all(np.isnan(xyz[i])) and np.isnan(err[i]) and np.isnan(err_given[i]), i      # fewer than two views
        else:
            assert np.all(np.isfinite(xyz[i])), i
            worst = max(worst, gr.point_error(xyz[i], e[0]) * e[1])
    print(f"\nC = {C}, per-camera K = {per_camera_K}, f32_rounding = {f32}:\n  points: relative error x gap {worst:.2e} "
          f"(triangulate_point {yard:.2e})")
    assert worst <= tolerance(yard)
    _check_errors(err, obs, xyz, rig, f32, "error of the triangulated points")
    _check_errors(err_given, obs, X0, rig, f32, "error of given points")


@pytest.mark.parametrize("f32", [False, True])
def test_reproject_depth_zero_takes_opencv_z_equals_one(core, f32):
    rig, obs, X0 = gr.api_case(3, False)
    assert np.array_equal(rig["R"][0], np.eye(3)) and np.all(rig["t"][0] == 0)          # camera 0 is [I | 0]
    pts = np.array(X0) * 0.1
    pts[:, 2] = 0.0                                                                       # depth 0 in camera 0
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.set_options(f32_rounding=f32)
    try:
        err = core.reproject(obs, pts)
    finally:
        core.set_options(f32_rounding=True)
    seen0 = ~np.isnan(obs[:, 0, 0]) & ((~np.isnan(obs[:, :, 0])).sum(axis=1) >= 2)
    assert seen0.sum() > 20 and np.all(np.isfinite(err[seen0]))
    print(f"\ndepth 0 in camera 0, f32_rounding = {f32}:")
    _check_errors(err, obs, pts, rig, f32, "error of points with Z = 0")
    # and the restatement takes the same branch
    o = np.array(obs[np.flatnonzero(seen0)[0]])
    p = pts[np.flatnonzero(seen0)[0]]
    assert np.isfinite(mocap_oracle.reprojection_error(o, p, rig["K"], rig["R"], rig["t"]))
