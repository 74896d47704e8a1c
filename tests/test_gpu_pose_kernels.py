"""The device routines of the initial pose estimation (csrc/pose_kernels.hpp: real_cubic_roots, seven_point_kernel,
score_kernel / fm_inlier), one sample, one polynomial and one model at a time, against the 50-digit references of
oracle/pose_reference.py -- tests/test_gpu_pose.py sees only the winner of a whole RANSAC run.  The kernels are reached
through the test-only probe tests/native/libmocap_poseprobe.so, which includes the product's header and uses its launchers.
The last group drives the host replay's batch edges through the public find_fundamental.

WHERE THE TOLERANCES COME FROM.  The yardstick is the reference's own distance to a correct double-precision
implementation: cv_pose_restate.run_7point (LAPACK SVD) against seven_point_exact on the 48 fixed samples
(tests/test_pose_reference_cpu.py prints it; restatement_error() recomputes it here, once per session).  Measured:

    error x gap  9.35e-13     (max |F - F_ref| / max |F_ref|) x gap, no sample exempted, smallest gap 2.5e-2
    constraint   2.85e-14     max |x2^T F x1| / max |F| on the seven points
    det          3.24e-18     |det F| / max |F|^3

(seven_point_kernel itself, on an MI355X: 2.70e-13, 7.82e-14, 2.15e-18.)
The kernel finds the null space by elimination, the restatement by SVD: two bases that condition the cubic differently by
a small factor, hence 16 x these values (model accuracy: 16 x 9.35e-13 / gap of the sample).  A dropped term, a wrong sign
or a wrong de-normalisation gives 1e-3 .. 1.  Root counts are asserted wherever gap >= 1e-6 (the gap rule, see
oracle/pose_reference.py); at most 2 % of the samples may fall below.

real_cubic_roots: per case 4 x the relative error of cp.real_cubic_roots (the same formulas in NumPy) against cubic_exact,
floor 4 ulp (8.9e-16).  Those errors, relative to the largest root, in the order of CUBIC_CASES: see the table there.

score_kernel: integers -- counts per model and the mask byte by byte equal score_exact's.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from mocap_core import synth
from oracle import cv_pose_restate as cp
from oracle import pose_reference as pr

pytestmark = pytest.mark.gpu

N_UNIQUE = 48
N_SLOTS = 150                      # blocks of 64, 64 and 22 lanes
FACTOR = 16.0
F_FILL, NF_FILL, CNT_FILL, MASK_FILL = -7.25, -99, -77, 0xAB
_vp = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(_vp)


@pytest.fixture(scope="module")
def probe(core):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "tests", "native", "libmocap_poseprobe.so")
    assert os.path.exists(path), "build it with `make -C tests/native` (__graft_entry__.build does)"
    lib = ctypes.CDLL(path)
    lib.poseprobe_seven_point.restype = ctypes.c_int
    lib.poseprobe_seven_point.argtypes = [ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp]
    lib.poseprobe_score.restype = ctypes.c_int
    lib.poseprobe_score.argtypes = [ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_float, _vp, _vp]
    lib.poseprobe_cubic.restype = ctypes.c_int
    lib.poseprobe_cubic.argtypes = [ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]
    lib.poseprobe_mask_guard.restype = ctypes.c_int
    return lib


def seven_point(lib, p1, p2, idx, n_slots):
    """-> F [n_slots][3][3][3], nF [n_slots]; slots the kernel does not write keep F_FILL / NF_FILL."""
    p1, p2 = np.ascontiguousarray(p1, dtype=np.float32), np.ascontiguousarray(p2, dtype=np.float32)
    idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, 7)
    F = np.full((n_slots, 3, 3, 3), F_FILL)
    nF = np.full(n_slots, NF_FILL, dtype=np.int32)
    assert lib.poseprobe_seven_point(0, len(p1), _p(p1), _p(p2), len(idx), _p(idx), n_slots, _p(F), _p(nF)) == 0
    return F, nF


def score(lib, p1, p2, F, nF, t, with_mask):
    """-> count [n_models], mask [N + guard] or None; what the kernel does not write keeps CNT_FILL / MASK_FILL."""
    p1, p2 = np.ascontiguousarray(p1, dtype=np.float32), np.ascontiguousarray(p2, dtype=np.float32)
    F = np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9)
    count = np.full(len(F), CNT_FILL, dtype=np.int32)
    mask = np.full(len(p1) + lib.poseprobe_mask_guard(), MASK_FILL, dtype=np.uint8) if with_mask else None
    if nF is not None:
        nF = np.ascontiguousarray(nF, dtype=np.int32)
        assert len(nF) == (len(F) + 2) // 3
    rc = lib.poseprobe_score(0, len(p1), _p(p1), _p(p2), len(F), _p(F), None if nF is None else _p(nF),
                             ctypes.c_float(float(np.float32(t))), _p(count), None if mask is None else _p(mask))
    assert rc == 0
    return count, mask


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------- seven-point models
@functools.lru_cache(maxsize=None)
def seven_set():
    """The fixed samples, their exact models and gaps, and the restatement's measured error (read-only, shared)."""
    p1, p2 = pr.probe_point_set()
    samples = pr.probe_samples(p1, p2, N_UNIQUE)
    m = pr.restatement_error(p1, p2, samples)
    assert len(m["exempt"]) <= 0.02 * N_UNIQUE and 0 < m["err_gap"] < 1e-9
    slot_sample = np.random.default_rng(7).permutation(np.arange(N_SLOTS) % N_UNIQUE)     # every sample in >= 3 lanes
    for a in (p1, p2, samples, slot_sample):
        a.setflags(write=False)
    return p1, p2, samples, m, slot_sample


@pytest.fixture(scope="module")
def seven_run(probe):
    p1, p2, samples, m, slot_sample = seven_set()
    F, nF = seven_point(probe, p1, p2, samples[slot_sample], N_SLOTS)
    F.setflags(write=False)
    nF.setflags(write=False)
    return F, nF


def test_seven_point_counts_and_models_match_exact_reference(seven_run):
    p1, p2, samples, m, slot_sample = seven_set()
    F, nF = seven_run
    worst_ratio = worst_err_gap = 0.0
    for slot in range(N_SLOTS):
        s = slot_sample[slot]
        models, gap = m["refs"][s]
        if s in m["exempt"]:
            continue
        assert nF[slot] == len(models), (slot, s, gap)
        for k, ref in enumerate(models):
            err = np.abs(F[slot, k] - ref).max() / np.abs(ref).max()
            worst_err_gap = max(worst_err_gap, err * gap)
            worst_ratio = max(worst_ratio, err / (FACTOR * m["err_gap"] / gap))
    print(f"\nseven_point_kernel vs exact: error x gap = {worst_err_gap:.3e} (restatement {m['err_gap']:.3e}), "
          f"worst error / tolerance = {worst_ratio:.3f}")
    assert worst_ratio <= 1.0


def test_seven_point_models_satisfy_constraint_and_rank(seven_run):
    p1, p2, samples, m, slot_sample = seven_set()
    F, nF = seven_run
    con = det = 0.0
    for slot in range(N_SLOTS):
        idx = samples[slot_sample[slot]]
        assert 0 <= nF[slot] <= 3
        c, d = pr.model_residuals(p1[idx], p2[idx], F[slot, :nF[slot]])
        con, det = max(con, c), max(det, d)
    print(f"\nseven_point_kernel: constraint = {con:.3e} (restatement {m['constraint']:.3e}), "
          f"det = {det:.3e} (restatement {m['det']:.3e})")
    assert con <= FACTOR * m["constraint"]
    assert det <= FACTOR * m["det"]


def test_seven_point_is_lane_independent(seven_run):
    _, _, _, _, slot_sample = seven_set()
    F, nF = seven_run
    for s in range(N_UNIQUE):
        slots = np.flatnonzero(slot_sample == s)
        assert len(slots) >= 3
        for slot in slots[1:]:
            assert nF[slot] == nF[slots[0]]
            assert same_bits(F[slot, :nF[slot]], F[slots[0], :nF[slot]])
    # model slots beyond nF are never written
    for slot in range(N_SLOTS):
        assert np.all(F[slot, nF[slot]:] == F_FILL)


@pytest.mark.parametrize("n_samples", [1, 63, 64, 65, 128, 129, 150])
def test_seven_point_is_batch_size_independent(probe, seven_run, n_samples):
    p1, p2, samples, _, slot_sample = seven_set()
    F150, nF150 = seven_run
    cap = N_SLOTS + 10
    F, nF = seven_point(probe, p1, p2, samples[slot_sample[:n_samples]], cap)
    assert same_bits(nF[:n_samples], nF150[:n_samples])
    assert same_bits(F[:n_samples], F150[:n_samples])
    assert np.all(nF[n_samples:] == NF_FILL) and np.all(F[n_samples:] == F_FILL)


def test_seven_point_degenerate_samples_give_no_model_and_no_junk(probe, seven_run):
    p1, p2, samples, _, slot_sample = seven_set()
    F150, nF150 = seven_run
    n = len(p1)
    # seven correspondences that share one point of image 1 (scale < FLT_EPSILON), appended to the point set
    q1 = np.vstack([p1, np.tile(np.float32([[101, 57]]), (7, 1))])
    q2 = np.vstack([p2, p2[:7] + np.float32(3)])
    same_point = np.arange(n, n + 7, dtype=np.int32)
    repeated = samples[0].copy()
    repeated[6] = repeated[0]                                  # two identical rows: the 7 x 9 system has rank 6
    assert pr.seven_point_exact(q1[repeated], q2[repeated]) == ([], 0.0)
    idx = np.vstack([samples[slot_sample[:5]], same_point[None], samples[slot_sample[5:9]], repeated[None],
                     samples[slot_sample[9:12]]])
    F, nF = seven_point(probe, q1, q2, idx, len(idx) + 2)
    good = [0, 1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13]
    assert same_bits(nF[good], nF150[:12]) and same_bits(F[good], F150[:12])
    for bad in (5, 10):
        assert nF[bad] == 0
        assert np.all(F[bad] == F_FILL)
    assert np.all(nF[len(idx):] == NF_FILL) and np.all(F[len(idx):] == F_FILL)


# ------------------------------------------------------------------------------------------- real_cubic_roots
# (name, coefficients c0..c3, kernel's root count, relative error of cp.real_cubic_roots against cubic_exact)
CUBIC_CASES = [
    ("three distinct roots",           (1.0, -6.0, 11.0, -6.0),                3, 0.0),
    ("three distinct, not integer",    (2.5, -1.75, -7.125, 3.0625),           3, 5.3e-16),
    ("one real root, R > 0",           (1.0, 1.0, 1.0, 3.0),                   1, 0.0),
    ("one real root, R < 0",           (1.0, 1.0, 1.0, -3.0),                  1, 0.0),
    ("(x-1)^2 (x+2): d == 0",          (1.0, 0.0, -3.0, 2.0),                  2, 0.0),
    ("triple root (x-1)^3",            (1.0, -3.0, 3.0, -1.0),                 2, 0.0),
    ("c0 = 0, two roots",              (0.0, 1.0, -5.0, 6.0),                  2, 0.0),
    ("c0 = 0, double root",            (0.0, 1.0, -2.0, 1.0),                  1, 0.0),
    ("c0 = 0, no root",                (0.0, 1.0, 0.0, 1.0),                   0, 0.0),
    ("c0 = c1 = 0, linear",            (0.0, 0.0, 2.0, 3.0),                   1, 0.0),
    ("c0 = c1 = c2 = 0",               (0.0, 0.0, 0.0, 5.0),                   0, 0.0),
    ("three roots x 1e+100",           (1e100, -6e100, 11e100, -6e100),        3, 7.4e-16),
    ("three roots x 1e-100",           (1e-100, -6e-100, 11e-100, -6e-100),    3, 0.0),
    ("one root x 1e+100",              (1e100, 1e100, 1e100, 3e100),           1, 0.0),
    ("one root x 1e-100",              (1e-100, 1e-100, 1e-100, -3e-100),      1, 0.0),
]
ULP = 2.220446049250313e-16


def _set_error(got, ref):
    """Distance of two root sets relative to the largest reference root (inf when one is empty and the other is not)."""
    if not len(ref) or not len(got):
        return 0.0 if len(ref) == len(got) else np.inf
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.abs(got[:, None] - ref[None, :])
    size = np.abs(ref).max()
    return float(max(d.min(axis=1).max(), d.min(axis=0).max()) / (size if size > 0 else 1.0))


def test_real_cubic_roots_by_branch(probe):
    n = 2 * 64 + 1                                             # two full blocks and one lane of a third, one call
    case_of = np.arange(n) % len(CUBIC_CASES)
    coeffs = np.array([CUBIC_CASES[c][1] for c in case_of], dtype=np.float64)
    roots = np.full((n, 3), F_FILL)
    nroots = np.full(n, NF_FILL, dtype=np.int32)
    assert probe.poseprobe_cubic(0, n, _p(coeffs), _p(roots), _p(nroots)) == 0
    refs = [pr.cubic_exact(c[1]) for c in CUBIC_CASES]
    lines = []
    for i in range(n):
        name, c, count, _ = CUBIC_CASES[case_of[i]]
        ref = refs[case_of[i]]
        with np.errstate(all="ignore"):
            restated = cp.real_cubic_roots(c)
        tol = max(4 * _set_error(restated, ref), 4 * ULP)
        err = _set_error(roots[i, :max(nroots[i], 0)], ref)
        if i < len(CUBIC_CASES):
            lines.append(f"  {name:32s} count {nroots[i]}  error {err:.2e}  restatement {_set_error(restated, ref):.2e}  tol {tol:.2e}")
    print("\nreal_cubic_roots vs cubic_exact:\n" + "\n".join(lines))
    for i in range(n):
        name, c, count, _ = CUBIC_CASES[case_of[i]]
        ref = refs[case_of[i]]
        with np.errstate(all="ignore"):
            restated = cp.real_cubic_roots(c)
        assert nroots[i] == count == len(restated), (name, i)
        assert np.all(roots[i, count:] == F_FILL), (name, i)               # nothing written past the count
        assert _set_error(roots[i, :count], ref) <= max(4 * _set_error(restated, ref), 4 * ULP), (name, i)
        assert same_bits(roots[i], roots[case_of[i]]), (name, i)           # the same polynomial in another lane / block


# ------------------------------------------------------------------------------------------- score_kernel
SCORE_N = [15, 63, 64, 65, 255, 256, 257, 1000]
SCORE_MODELS = [1, 3, 7, 384]
N_UNIQUE_MODELS = 12


@functools.lru_cache(maxsize=None)
def score_set():
    """1000 correspondences of the rig of the seven-point samples with 30 % gross outliers, 12 exact models of that rig,
    their exact inlier masks [12][1000] at thr = 1 (computed once; every case below is a prefix), and which of the 12
    sits in each of the 384 model slots."""
    rig = synth.ring_rig(3)
    obs, _ = synth.make_ba_observations(rig, 1100, seed=77, noise_px=0.5, dropout=0.0)
    obs = np.trunc(obs)
    ok = ~np.isnan(obs[:, :2]).any(axis=(1, 2))
    p1, p2 = obs[ok, 0][:1000].astype(np.float32), obs[ok, 1][:1000].astype(np.float32)
    assert len(p1) == 1000
    rng = np.random.default_rng(11)
    bad = rng.random(1000) < 0.3
    p2[bad] = rng.uniform(0, 320, (int(bad.sum()), 2)).astype(int)
    _, _, _, m, _ = seven_set()
    models = [M for models, _ in m["refs"] for M in models][:N_UNIQUE_MODELS]
    assert len(models) == N_UNIQUE_MODELS
    t = np.float32(1.0)
    exact = np.array([pr.score_exact(p1, p2, M, t) for M in models])
    assert 100 < exact[:, :].sum(axis=1).max() < 1000          # a real mix of inliers and outliers
    slot_model = rng.permutation(np.arange(384) % N_UNIQUE_MODELS)
    for a in (p1, p2, exact, slot_model):
        a.setflags(write=False)
    return p1, p2, np.array(models), exact, slot_model, t


@pytest.mark.parametrize("n_models", SCORE_MODELS)
@pytest.mark.parametrize("N", SCORE_N)
def test_score_counts_gating_and_mask(probe, N, n_models):
    p1, p2, models, exact, slot_model, t = score_set()
    p1, p2 = p1[:N], p2[:N]
    which = slot_model[:n_models]
    F = models[which]
    want = exact[which, :N].sum(axis=1).astype(np.int32)
    guard = probe.poseprobe_mask_guard()
    # every slot scored; the mask is model 0's, bytes past N untouched
    count, mask = score(probe, p1, p2, F, None, t, True)
    assert np.array_equal(count, want)
    assert np.array_equal(mask[:N], exact[which[0], :N].astype(np.uint8))
    assert guard >= 8 and np.all(mask[N:] == MASK_FILL)
    # the three slots of sample j gated by nF[j] = 0, 1, 2, 3, 0, ...: slot k >= nF counts 0 and is not scored
    nF = np.arange((n_models + 2) // 3, dtype=np.int32) % 4
    gated = np.where(np.arange(n_models) % 3 < nF[np.arange(n_models) // 3], want, 0)
    count, mask = score(probe, p1, p2, F, nF, t, True)
    assert np.array_equal(count, gated)
    assert np.all(mask == MASK_FILL)                           # model 0 is gated off (nF[0] = 0): no mask at all
    # the other phase of the pattern scores model 0, and no mask buffer is a valid call
    nF = (np.arange((n_models + 2) // 3, dtype=np.int32) + 3) % 4
    gated = np.where(np.arange(n_models) % 3 < nF[np.arange(n_models) // 3], want, 0)
    count, _ = score(probe, p1, p2, F, nF, t, False)
    assert np.array_equal(count, gated)


ROWS_F = np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])        # pure x translation: both distances are (y2 - y1)^2


def test_score_boundary_is_less_or_equal(probe):
    # integers: |dy| = 0, 1, 2 at thr = 1 -> in, in (err == t), out
    dy = np.array([0, 1, -1, 2, -2, 1, 0, -2, 1] * 8, dtype=np.float32)
    n = len(dy)
    p1 = np.stack([np.arange(n) % 17, 40 + np.arange(n) % 5], axis=1).astype(np.float32)
    p2 = np.stack([p1[:, 0] + 6, p1[:, 1] + dy], axis=1).astype(np.float32)
    want = np.abs(dy) <= 1
    assert np.array_equal(pr.score_exact(p1, p2, ROWS_F, np.float32(1.0)), want)
    count, mask = score(probe, p1, p2, ROWS_F, None, np.float32(1.0), True)
    assert count[0] == want.sum() and np.array_equal(mask[:n], want.astype(np.uint8))
    # after the float cast: thr * thr < dy^2 in double, yet float(thr * thr) == float(dy^2) -> err <= t holds
    d = np.float32(1.1)
    d2 = float(d) * float(d)                                   # exact in double (24-bit factors)
    thr = np.sqrt(d2) * (1 - 1e-9)
    assert thr * thr < d2 and np.float32(thr * thr) == np.float32(d2)
    q1 = np.array([[3, 0], [4, 0], [5, 0]], dtype=np.float32)
    q2 = np.array([[9, d], [1, -d], [2, np.nextafter(d, np.float32(2))]], dtype=np.float32)
    want = np.array([True, True, False])
    assert np.array_equal(pr.score_exact(q1, q2, ROWS_F, np.float32(thr * thr)), want)
    count, mask = score(probe, q1, q2, ROWS_F, None, np.float32(thr * thr), True)
    assert count[0] == 2 and np.array_equal(mask[:3], want.astype(np.uint8))


def test_score_nan_and_infinity_follow_std_max(probe):
    """F = [e]x, e = (3, 4, 1): both epipoles are e.  x2 = e makes e1 = 0 * inf = NaN: std::max(e1, e2) = (e1 < e2) ? e2 : e1
    keeps the NaN and the point is an outlier although e2 = 0; x1 = e makes e2 NaN, and e1 decides."""
    e = (3.0, 4.0, 1.0)
    F = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
    n = 70
    rng = np.random.default_rng(3)
    p1 = rng.integers(0, 40, (n, 2)).astype(np.float32)
    p2 = rng.integers(0, 40, (n, 2)).astype(np.float32)
    p1[::3] = p2[::3] * 2 - np.float32([3, 4])                 # collinear with e: x1 = e + 2 (x2 - e) -> both distances 0
    p2[0], p1[0] = (3, 4), (6, 8)                              # x2 is the epipole
    p2[66], p1[66] = (3, 4), (20, 1)
    p1[1], p2[1] = (3, 4), (9, 12)                             # x1 is the epipole
    p1[65], p2[65] = (3, 4), (30, 7)
    p1[2], p2[2] = (3, 4), (3, 4)                              # both
    want = pr.score_exact(p1, p2, F, np.float32(1.0))
    assert not want[0] and not want[66] and want[1] and want[65] and not want[2] and 10 < want.sum() < n - 10
    with np.errstate(all="ignore"):
        assert np.array_equal(cp.compute_error(p1, p2, F) <= np.float32(1.0), want)
    count, mask = score(probe, p1, p2, np.stack([F, F, F]), None, np.float32(1.0), True)
    assert np.array_equal(mask[:n], want.astype(np.uint8))
    assert count.tolist() == [want.sum()] * 3


# ------------------------------------------------------------------------------------------- batch edges of the replay
@functools.lru_cache(maxsize=None)
def outlier_set():
    """The 30 %-outlier set of test_gpu_pose.test_find_fundamental_long_run_many_batches."""
    rng = np.random.default_rng(5)
    rig = synth.ring_rig(2)
    obs, _ = synth.make_ba_observations(rig, 300, seed=30, dropout=0.0)
    obs = np.trunc(obs)
    bad = rng.random(300) < 0.3
    obs[bad, 1] = rng.uniform(0, 320, (bad.sum(), 2)).astype(int)
    a, b = obs[:, 0], obs[:, 1]
    ok = ~(np.isnan(a).any(axis=1) | np.isnan(b).any(axis=1))
    p1, p2 = a[ok].astype(np.float32), b[ok].astype(np.float32)
    p1.setflags(write=False)
    p2.setflags(write=False)
    return p1, p2


def _same_as_sequential_loop(core, p1, p2, thr, conf, max_iters, oracle_args=None):
    F, mask, info = core.find_fundamental(p1, p2, thr, conf, max_iters)
    a = (thr, conf, max_iters) if oracle_args is None else oracle_args
    Fr, maskr, infor = cp.find_fundamental_mat(p1, p2, cp.FM_RANSAC, a[0], a[1], a[2], return_info=True)
    assert info == infor
    assert np.array_equal(mask, maskr.ravel())
    np.testing.assert_allclose(F, Fr, rtol=1e-6, atol=1e-9 * np.abs(Fr).max())
    return info


@pytest.mark.parametrize("max_iters", [1, 2, 127, 128, 129, 300])
def test_replay_max_iters_around_the_batch_size(core, max_iters):
    p1, p2 = outlier_set()
    info = _same_as_sequential_loop(core, p1, p2, 1.0, 0.99999, max_iters)
    assert info["iterations"] == max_iters                    # this set needs more than 300 iterations: the cap binds


def test_replay_smallest_accepted_set(core):
    from mocap_core.capi import MocapError
    p1, p2 = pr.probe_point_set()
    _same_as_sequential_loop(core, p1[:15], p2[:15], 1.0, 0.99999, 1000)
    with pytest.raises(MocapError):
        core.find_fundamental(p1[:14], p2[:14], 1.0, 0.99999, 1000)


@pytest.mark.parametrize("thr,conf", [(0.0, 0.99999), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)])
def test_replay_argument_defaults(core, thr, conf):
    """thr <= 0 becomes 3, a confidence outside (0, 1) becomes 0.99: the oracle called with those values outright."""
    p1, p2 = outlier_set()
    _same_as_sequential_loop(core, p1, p2, thr, conf, 1000,
                             oracle_args=(3.0 if thr <= 0 else thr, conf if 0 < conf < 1 else 0.99, 1000))


SHRINK_SEED = 0          # the first seed with the property asserted below (searched with shrinking_case alone)
SHRINK_CONF = 0.9


def shrinking_case(seed):
    """-> (p1, p2, it_final, winner's inliers, best inliers among the samples [it_final, 128) of the RNG stream)."""
    rig = synth.ring_rig(3)
    obs, _ = synth.make_ba_observations(rig, 120, seed=seed, noise_px=0.4, dropout=0.0)
    obs = np.trunc(obs)
    ok = ~np.isnan(obs[:, :2]).any(axis=(1, 2))
    p1, p2 = obs[ok, 0].astype(np.float32), obs[ok, 1].astype(np.float32)
    _, _, info = cp.find_fundamental_mat(p1, p2, cp.FM_RANSAC, 1.0, SHRINK_CONF, 1000, return_info=True)
    rng, later = cp.RNG(), 0
    for it in range(128):
        idx = cp.get_subset(p1, p2, rng)
        if it >= info["iterations"]:
            for F in cp.run_7point(p1[idx], p2[idx]):
                later = max(later, int((cp.compute_error(p1, p2, F) <= np.float32(1.0)).sum()))
    return p1, p2, info["iterations"], info["inliers"], later


def test_replay_stops_inside_a_batch_when_the_count_shrinks(core):
    """The sequential loop stops at it_final < 128 although a later sample of the same first GPU batch has strictly more
    inliers than the winner: the replay must not look at it (`it < niters` inside a batch)."""
    p1, p2, it_final, inliers, later = shrinking_case(SHRINK_SEED)
    assert it_final < 128 and later > inliers, (it_final, inliers, later)
    info = _same_as_sequential_loop(core, p1, p2, 1.0, SHRINK_CONF, 1000)
    assert info["iterations"] == it_final and info["inliers"] == inliers
