"""The high-precision reference of the pose kernels (oracle/pose_reference.py) is itself checked here, on the CPU: against
the double-precision restatement of OpenCV's run7Point on the fixed sample set of tests/test_gpu_pose_kernels.py, and
against answers known by hand.  The figures printed by test_seven_point_exact_agrees_with_the_restatement are the
reference's own error scale; the GPU test derives its tolerances from them (its module docstring records them)."""
import numpy as np

from oracle import cv_pose_restate as cp
from oracle import pose_reference as pr

N_UNIQUE = 48          # as in tests/test_gpu_pose_kernels.py


def test_seven_point_exact_agrees_with_the_restatement():
    p1, p2 = pr.probe_point_set()
    samples = pr.probe_samples(p1, p2, N_UNIQUE)
    m = pr.restatement_error(p1, p2, samples)
    share = len(m["exempt"]) / N_UNIQUE
    gaps = [g for _, g in m["refs"]]
    print(f"\nrun_7point vs seven_point_exact over {N_UNIQUE} samples: error x gap = {m['err_gap']:.3e}, "
          f"constraint = {m['constraint']:.3e}, det = {m['det']:.3e}, smallest gap = {min(gaps):.3e}, "
          f"exempted share = {100 * share:.1f} %")
    assert share <= 0.02
    for s in range(N_UNIQUE):
        if s not in m["exempt"]:
            assert m["count_equal"][s], (s, gaps[s])
    assert sum(len(models) for models, _ in m["refs"]) > N_UNIQUE        # some samples have three models
    # double precision against 50 digits on these samples: far below anything a wrong term would cause (1e-3 .. 1)
    assert 0 < m["err_gap"] < 1e-9 and m["constraint"] < 1e-11 and m["det"] < 1e-14
    # the reference's models solve the problem they are defined by, to double rounding of their own entries
    for idx, (models, _) in zip(samples, m["refs"]):
        con, det = pr.model_residuals(p1[idx], p2[idx], models)
        assert con < 1e-9 and det < 1e-14


def test_seven_point_exact_rank_deficient_sample_has_no_model():
    p1, p2 = pr.probe_point_set()
    idx = pr.probe_samples(p1, p2, 1)[0].copy()
    idx[6] = idx[0]                                                     # one correspondence twice: rank 6
    assert pr.seven_point_exact(p1[idx], p2[idx]) == ([], 0.0)


def test_cubic_exact_hand_known():
    assert pr.cubic_exact([1, 0, -3, 2]) == [-2.0, 1.0]                 # (x - 1)^2 (x + 2)
    assert pr.cubic_exact([0, 1, 0, 1]) == []                           # x^2 + 1
    assert pr.cubic_exact([1, 0, 1, 0]) == [0.0]                        # x (x^2 + 1)
    assert pr.cubic_exact([1, -6, 11, -6]) == [1.0, 2.0, 3.0]
    assert pr.cubic_exact([1, -3, 3, -1]) == [1.0]                      # (x - 1)^3
    assert pr.cubic_exact([0, 0, 2, 4]) == [-2.0]
    assert pr.cubic_exact([0, 0, 0, 5]) == [] and pr.cubic_exact([0, 0, 0, 0]) == []
    assert pr.cubic_exact([2.0 ** 332, 0, -3 * 2.0 ** 332, 2.0 ** 333]) == [-2.0, 1.0]


def test_score_exact_hand_known_and_restatement_max_order():
    # F of a pure x translation: the epipolar lines are the image rows, both distances are (y2 - y1)^2 exactly
    F = np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]])
    y1 = np.array([5, 5, 5, 5, 5], dtype=np.float32)
    y2 = np.array([5, 6, 4, 7, 3], dtype=np.float32)
    m1 = np.stack([np.arange(5, dtype=np.float32), y1], axis=1)
    m2 = np.stack([np.arange(5, dtype=np.float32) + 9, y2], axis=1)
    assert pr.score_exact(m1, m2, F, np.float32(1.0)).tolist() == [True, True, True, False, False]
    assert pr.score_exact(m1, m2, F, np.float32(4.0)).all()
    assert cp.compute_error(m1, m2, F).tolist() == [0.0, 1.0, 1.0, 4.0, 4.0]
    # F = [e]x for the integer epipole e = (3, 4, 1): F x = 0 and F^T x = 0 at x = e.
    #   x2 = e: e1 = 0 * inf = NaN, max(e1, e2) = NaN -> outlier whatever e2 is
    #   x1 = e: e2 = NaN, e1 finite -> (e1 < NaN) is false -> e1 decides
    e = (3.0, 4.0, 1.0)
    F = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
    m1 = np.array([[6, 8], [3, 4], [10, 2]], dtype=np.float32)
    m2 = np.array([[3, 4], [9, 12], [17, 0]], dtype=np.float32)
    # row 0: x2 = e.  row 1: x1 = e and x2 = (9, 12), on no line through e but d1 = x1 . (F^T x2) = 0 -> e1 = 0.
    # row 2: ordinary; (10, 2), (17, 0) and e are collinear: x2 . (e x x1) = 0 -> both distances 0
    got = pr.score_exact(m1, m2, F, np.float32(1.0))
    assert got.tolist() == [False, True, True]
    with np.errstate(all="ignore"):
        assert (cp.compute_error(m1, m2, F) <= np.float32(1.0)).tolist() == got.tolist()
