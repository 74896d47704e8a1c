"""Trajectories without a GPU: the plain statement of the contract (tests/track_smooth_reference.py) on exact polynomials, against
its own 50-digit evaluation, at the edge of every rule, and the four C-ABI symbols (declared, exported, bound)."""
import os
import re
import subprocess

import numpy as np
import pytest

import track_smooth_reference as ts
from conftest import ROOT

INF = float("inf")

# The accuracy of the float64 statement against the 50-digit fit, in the scaled measure of ts.scaled_errors, over ACCURACY_CASES
# with the seeds fixed below: measured pos 3.43e-14, vel 6.62e-13, acc 3.86e-12, all three at degree 3; the largest condition number
# of a Gram matrix was 3.2e4 (degree 3, W = 8, a lopsided window).  Asserted with the 4x margin for the spread between seeds.
MEASURED = {"pos": 3.43e-14, "vel": 6.62e-13, "acc": 3.86e-12}
COND_SEEN = 3.2e4
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
ACCURACY_CASES = [  # degree, W, span, n_min, max_gap
    (1, 1, INF, 2, 1), (1, 8, INF, 3, 4), (2, 4, INF, 3, 4), (2, 8, 0.05, 4, 6), (2, 32, INF, 4, 6), (3, 4, INF, 4, 3),
    (3, 8, INF, 5, 6), (3, 32, 0.2, 5, 6)]
SEEDS = (101, 102)


def regular(F, R=1, dt=1.0 / 128.0):
    """t on a binary grid (differences exact) and a gently curved row."""
    t = 2.0 + dt * np.arange(F)
    traj = np.stack([np.stack([np.sin(t + r), np.cos(2.0 * t + r), 0.5 * t * t], axis=1) for r in range(R)])
    return t, traj


def run(t, traj, d=2, W=4, span=INF, n_min=None, max_gap=0):
    return ts.smooth(t, traj, d, W, span, d + 1 if n_min is None else n_min, max_gap)


def test_vectorised_statement_equals_the_scalar_one_bit_for_bit():
    t, _, traj = ts.make_session(7, 90, 2, dropout=0.15, max_run=5)
    t[40] = t[38]
    t[60] = np.nan
    traj[1, :12] = np.nan
    for d, W, span, n_min, max_gap in ((1, 2, INF, 2, 2), (2, 5, 0.04, 4, 3), (3, 9, INF, 4, 5)):
        out = ts.smooth(t, traj, d, W, span, n_min, max_gap)
        good, pres = ts.good_times(t), ts.present_mask(t, traj)
        for r in range(2):
            for f in range(90):
                pos, vel, acc, res, n, flag = ts.smooth_sample(t, traj, r, f, d, W, span, n_min, max_gap, good, pres)
                assert (n, flag) == (out["n_used"][r, f], out["flag"][r, f]), (d, r, f)
                for k, v in (("pos", pos), ("vel", vel), ("acc", acc), ("res", res)):
                    assert ts.same_bits(out[k][r, f], np.array(v)), (d, r, f, k, out[k][r, f], v)
        assert set(np.unique(out["flag"])) >= {0, ts.SMOOTHED, ts.FILLED, ts.BAD_TIME}


@pytest.mark.parametrize("d", [1, 2, 3])
def test_reproduces_an_exact_polynomial_through_gaps(d):
    """t on a grid of 1/64 and integer coefficients: every x_g is exact, so the least-squares fit IS the polynomial and what is left
    is the statement's own rounding: inside the accuracy bound, in its scaled measure."""
    rng = np.random.default_rng(20 + d)
    F, W = 120, 6
    t = np.cumsum(rng.integers(1, 4, F)) / 64.0
    co = rng.integers(-3, 4, (3, d + 1)).astype(np.float64)
    co[:, d] = [1.0, -2.0, 3.0]
    truth = np.stack([sum(co[k, i] * t ** i for i in range(d + 1)) for k in range(3)], axis=1)
    v_true = np.stack([sum(i * co[k, i] * t ** (i - 1) for i in range(1, d + 1)) for k in range(3)], axis=1)
    a_true = np.stack([sum(i * (i - 1) * co[k, i] * t ** (i - 2) for i in range(2, d + 1)) if d >= 2 else 0 * t for k in range(3)], axis=1)
    traj = truth[None].copy()
    for lo, hi in ((10, 13), (40, 46), (47, 48), (80, 81)):
        traj[0, lo:hi] = np.nan
    out = run(t, traj, d=d, W=W, n_min=d + 1, max_gap=6)
    assert (out["flag"][0, 40:46] == ts.FILLED).all() and (out["flag"][0, 10:13] == ts.FILLED).all()
    assert set(np.unique(out["flag"])) == {ts.SMOOTHED, ts.FILLED}
    X = np.abs(truth).max()
    h = np.array([max(abs(t[g] - t[f]) for g in range(max(f - W, 0), min(f + W, F - 1) + 1)) for f in range(F)])[:, None]
    assert (np.abs(out["pos"][0] - truth) / X).max() <= BOUND["pos"]
    assert (np.abs(out["vel"][0] - v_true) * h / X).max() <= BOUND["vel"]
    if d >= 2:
        assert (np.abs(out["acc"][0] - a_true) * h * h / X).max() <= BOUND["acc"]
    else:
        assert np.isnan(out["acc"]).all()
    assert out["res"].max() <= BOUND["pos"] * X


def test_accuracy_against_fifty_digits():
    worst = {"pos": 0.0, "vel": 0.0, "acc": 0.0}
    cond = 0.0
    for seed in SEEDS:
        t, _, traj = ts.make_session(seed, 110, 2, dropout=0.1, max_run=6)
        for d, W, span, n_min, max_gap in ACCURACY_CASES:
            ref = ts.smooth(t, traj, d, W, span, n_min, max_gap)
            exact = ts.smooth_mp(t, traj, d, W, span, n_min, max_gap, ref=ref)
            fitted = np.isin(ref["flag"], (ts.SMOOTHED, ts.FILLED))
            assert fitted.sum() > 100 and np.array_equal(fitted, np.isfinite(exact["res"]))
            errs = ts.scaled_errors(ref, exact, d)
            cond = max(cond, float(np.nanmax(exact["cond"])))
            print(f"seed {seed} d {d} W {W:2d} span {span} n_min {n_min} max_gap {max_gap}: fitted {int(fitted.sum())}, "
                  + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f", cond <= {np.nanmax(exact['cond']):.2e}")
            for k, v in errs.items():
                worst[k] = max(worst[k], v)
            res_err = np.abs(ref["res"][fitted] - exact["res"][fitted]).max()
            assert res_err <= BOUND["pos"] * np.nanmax(exact["scale"]), res_err
    print("worst scaled errors", worst, "largest condition number", cond)
    for k in worst:
        assert worst[k] <= BOUND[k], (k, worst[k])
    assert cond <= 4.0 * COND_SEEN          # far inside the 4e5 at which a degree-3 window was expected to stay
    # in metres: a position error of BOUND x (a 3 m room) sits eight orders below the 0.5 mm triangulation noise
    assert BOUND["pos"] * 3.0 < 1e-8 * 0.0005


def test_n_min_edge_and_few():
    t, traj = regular(40)
    traj[0, 20:] = np.nan
    traj[0, 23] = [1.0, 2.0, 3.0]
    out = run(t, traj, d=2, W=3, n_min=4)
    # frame 19 sees 16 .. 19 (4 samples): fitted; frame 23 sees itself only; frame 18: 15 .. 19 = 5
    assert out["n_used"][0, 19] == 4 and out["flag"][0, 19] == ts.SMOOTHED
    assert out["n_used"][0, 23] == 1 and out["flag"][0, 23] == ts.FEW and np.isnan(out["pos"][0, 23]).all()
    out5 = run(t, traj, d=2, W=3, n_min=5)
    assert out5["flag"][0, 19] == ts.FEW and out5["n_used"][0, 19] == 4 and out5["flag"][0, 18] == ts.SMOOTHED
    assert np.isnan(out5["res"][0, 19]) and np.isnan(out5["vel"][0, 19]).all()
    # neither present nor fillable: flag 0, the count still reported
    assert out["flag"][0, 21] == 0 and out["n_used"][0, 21] == 3 and np.isnan(out["pos"][0, 21]).all()


def test_gap_of_max_gap_is_filled_and_one_more_is_not():
    t, traj = regular(60, R=2)
    traj[0, 20:23] = np.nan      # 3 missing
    traj[1, 20:24] = np.nan      # 4 missing
    out = run(t, traj, d=2, W=5, max_gap=3)
    assert (out["flag"][0, 20:23] == ts.FILLED).all() and np.isfinite(out["pos"][0, 20:23]).all()
    assert (out["flag"][1, 20:24] == 0).all() and np.isnan(out["pos"][1, 20:24]).all()
    assert (run(t, traj, d=2, W=5, max_gap=0)["flag"][0, 20:23] == 0).all()
    assert (run(t, traj, d=2, W=5, max_gap=4)["flag"][1, 20:24] == ts.FILLED).all()
    # a filled value interpolates: between its neighbours' positions on this gentle curve
    lo, hi = np.minimum(traj[0, 19], traj[0, 23]), np.maximum(traj[0, 19], traj[0, 23])
    assert ((out["pos"][0, 20:23] >= lo - 1e-3) & (out["pos"][0, 20:23] <= hi + 1e-3)).all()


def test_gaps_at_either_end_of_the_session_are_never_filled():
    t, traj = regular(30)
    traj[0, :2] = np.nan
    traj[0, 28:] = np.nan
    out = run(t, traj, d=1, W=4, max_gap=4)
    assert (out["flag"][0, :2] == 0).all() and (out["flag"][0, 28:] == 0).all()
    assert np.isnan(out["pos"][0, :2]).all() and np.isnan(out["pos"][0, 28:]).all()
    assert (out["flag"][0, 2:28] == ts.SMOOTHED).all() and (out["n_used"][0, :2] > 0).all()


def test_a_sample_exactly_at_span_counts():
    t, traj = regular(30)                      # dt = 1 / 128: differences are exact
    out = run(t, traj, d=1, W=4, span=2.0 / 128.0)
    assert out["n_used"][0, 15] == 5
    below = run(t, traj, d=1, W=4, span=np.nextafter(2.0 / 128.0, 0.0))
    assert below["n_used"][0, 15] == 3
    # a fill needs both neighbours inside the span
    traj[0, 10:12] = np.nan
    assert (run(t, traj, d=1, W=4, span=2.0 / 128.0, n_min=2, max_gap=2)["flag"][0, 10:12] == [ts.FILLED, ts.FILLED]).all()
    assert (run(t, traj, d=1, W=4, span=1.0 / 128.0, n_min=2, max_gap=2)["flag"][0, 10:12] == [0, 0]).all()


def test_equal_decreasing_and_non_finite_time_stamps():
    t, traj = regular(24)
    t[8] = t[7]                 # equal
    t[13] = t[10]               # decreasing
    t[17] = np.inf
    t[20] = np.nan
    good = ts.good_times(t)
    assert [f for f in range(24) if not good[f]] == [8, 13, 17, 20]
    out = run(t, traj, d=1, W=2)
    for f in (8, 13, 17, 20):
        assert out["flag"][0, f] == ts.BAD_TIME and out["n_used"][0, f] == 0 and np.isnan(out["pos"][0, f]).all()
    assert out["n_used"][0, 7] == 4 and out["n_used"][0, 12] == 4 and out["n_used"][0, 15] == 3 and out["n_used"][0, 3] == 5
    assert ts.good_times(np.array([np.nan, np.nan, 1.0, 1.0])).tolist() == [False, False, True, False]
    assert ts.good_times(np.array([3.0, 1.0, 2.0, 3.0, 4.0])).tolist() == [True, False, False, False, True]


def test_a_nan_time_stamp_inside_a_gap():
    t, traj = regular(30)
    traj[0, 10:12] = np.nan
    t[10] = np.nan
    out = run(t, traj, d=1, W=3, max_gap=2)
    assert out["flag"][0, 10] == ts.BAD_TIME and out["flag"][0, 11] == ts.FILLED and np.isfinite(out["pos"][0, 11]).all()
    # a present frame whose time is bad is not present: the gap 9 .. 12 is now three frames long
    traj[0, 9] = traj[0, 8]
    t[9] = t[8]
    assert run(t, traj, d=1, W=3, max_gap=2)["flag"][0, 11] == 0
    assert run(t, traj, d=1, W=3, max_gap=3)["flag"][0, 11] == ts.FILLED


def test_gather_lowest_slot_shared_rows_and_min_hits():
    F, K = 4, 5
    xyz = np.arange(F * K * 3, dtype=np.float64).reshape(F, K, 3)
    ids = np.array([[3, 1, 3, 7, -1], [1, 3, 9, 2, 5], [5, 5, 1, 0, 0], [1, 3, 5, 7, 2]], dtype=np.int32)
    hits = np.array([[5, 5, 5, 5, 0], [1, 9, 9, 9, 9], [1, 3, 3, 3, 3], [9, 9, 9, 9, 9]], dtype=np.int32)
    n_pts = np.array([4, 5, 5, 7], dtype=np.int32)      # frame 3: outside 0 .. K_max, counts as 0
    relabel = np.array([-1, 0, -1, 1, -1, 1, 2, 2], dtype=np.int32)   # ids 3 and 5 share row 1; id 9 is beyond the table
    xyz[1, 1, 2] = np.inf                                # frame 1: id 3 not finite, id 5 (slot 4) takes the shared row
    traj = ts.gather(xyz, n_pts, ids, relabel, 3)
    assert np.array_equal(traj[0, :3], [xyz[0, 1], xyz[1, 0], xyz[2, 2]])
    assert np.array_equal(traj[1, :3], [xyz[0, 0], xyz[1, 4], xyz[2, 0]])       # the lowest slot of the two ids
    assert np.array_equal(traj[2, 0], xyz[0, 3]) and np.isnan(traj[2, 1:]).all() and np.isnan(traj[:, 3]).all()
    held = ts.gather(xyz, n_pts, ids, relabel, 3, hits=hits, min_hits=2)
    assert np.isnan(held[0, 1]).all() and np.array_equal(held[1, 2], xyz[2, 1]) and np.array_equal(held[0, 0], xyz[0, 1])


def test_track_table():
    from mocap_core import helpers
    ids = np.array([[0, 2, -1], [2, 0, 5], [2, -1, -1], [2, 5, 0]], dtype=np.int32)
    relabel, rows = helpers.track_table(ids, min_len=2)
    assert rows.tolist() == [0, 2, 5] and relabel.tolist() == [0, -1, 1, -1, -1, 2] and relabel.dtype == np.int32
    hits = np.array([[1, 1, 0], [2, 2, 1], [3, 0, 0], [4, 2, 3]], dtype=np.int32)
    relabel, rows = helpers.track_table(ids, hits, min_len=2, min_hits=2)
    assert rows.tolist() == [0, 2] and relabel.tolist() == [0, -1, 1, -1, -1, -1]
    relabel, rows = helpers.track_table(np.full((3, 2), -1, dtype=np.int32))
    assert rows.size == 0 and relabel.tolist() == [-1]


def test_the_four_symbols_are_declared_exported_and_bound():
    from mocap_core import capi
    names = {"mocap_gather_tracks": 12, "mocap_gather_tracks_dev": 12, "mocap_smooth_tracks": 16, "mocap_smooth_tracks_dev": 16}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mocap_core.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for n, n_args in names.items():
        assert re.search(r"\bint %s\s*\(" % n, header), n
        assert re.search(r" T %s$" % n, exported, flags=re.M), n
        assert n in capi.SIGNATURES and len(capi.SIGNATURES[n][1]) == n_args
        assert callable(getattr(capi.MocapCore, n[len("mocap_"):]))
    assert "#define MOCAP_TS_MAX_ROWS 1024" in header and "#define MOCAP_TS_MAX_HALF_WINDOW 32" in header
    assert (capi.TS_MAX_ROWS, capi.TS_MAX_HALF_WINDOW) == (1024, 32)
    for name, value in (("SMOOTHED", 1), ("FILLED", 2), ("FEW", 4), ("SINGULAR", 8), ("BAD_TIME", 16)):
        assert re.search(r"MOCAP_TS_%s = %d\b" % (name, value), header) and getattr(capi, "TS_" + name) == value == getattr(ts, name)
