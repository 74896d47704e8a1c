"""Track stitching without a GPU: the plain statement of the contract (tests/track_stitch_reference.py) at the edge of every rule,
its vectorised form against its scalar form, rounds of mutually best pairs against the sorted walk, the tracked flight on which the
GPU test relies, and the two C-ABI symbols (declared, exported, bound)."""
import os
import re
import subprocess

import numpy as np

import marker_track_reference as mt
import track_smooth_reference as ts
import track_stitch_reference as st
from conftest import ROOT

INF = float("inf")
WIDE = dict(fit_frames=4, max_dt=INF, gate=1.0, gate_rate=0.0)


def grid(F, dt=1.0 / 128.0):
    return 2.0 + dt * np.arange(F)              # binary fractions: every difference is exact


def rows_of(F, *spans):
    """One row per span (lo, hi, position at lo [3], velocity per frame [3]): present on lo .. hi - 1, on a straight line."""
    traj = np.full((len(spans), F, 3), np.nan)
    for r, (lo, hi, x, v) in enumerate(spans):
        traj[r, lo:hi] = np.asarray(x, dtype=float) + np.arange(hi - lo)[:, None] * np.asarray(v, dtype=float)
    return traj


def both(t, traj, **kw):
    a, b = st.stitch_scalar(t, traj, **kw), st.stitch(t, traj, **kw)
    assert st.same(a, b) and ts.same_bits(a["table"], b["table"])
    return b


def test_vectorised_statement_equals_the_scalar_one_bit_for_bit():
    linked = 0
    for seed, F, M, fit in ((1, 300, 3, 8), (2, 120, 4, 1), (3, 200, 2, 64)):
        t, _, traj = ts.make_session(seed, F, M, dropout=0.08, max_run=4)
        cuts = [(m, 20 + 11 * m + 40 * k, 2 + 5 * k + m) for m in range(M) for k in range(2)]
        rows, _ = st.cut_session(traj, cuts, seed=seed)
        rows[-1] = np.nan
        t[33] = t[31]                           # equal, then below what came before; NaN; all inside or beside fragment ends
        t[47] = np.nan
        t[76] = t[70]
        for max_dt, gate, rate in ((INF, 0.05, 1.0), (0.1, 0.3, 0.0), (0.05, 10.0, 0.0)):
            a, b = st.stitch_scalar(t, rows, fit, max_dt, gate, rate), st.stitch(t, rows, fit, max_dt, gate, rate)
            assert st.same(a, b) and ts.same_bits(a["table"], b["table"]), (seed, max_dt)
            assert ts.same_bits(np.array([m for m in a["tail"] + a["head"] if m is not None]),
                                np.concatenate([b["tail"], b["head"]])[np.tile(a["ext"][:, 2] != 0, 2)])
            r = st.associate_rounds(b["table"])
            assert np.array_equal(r[0], b["next"]) and np.array_equal(r[1], b["prev"]) and ts.same_bits(r[2], b["cost"])
            linked += int((b["next"] >= 0).sum())
    assert linked >= 10


def test_a_straight_line_is_extrapolated_exactly_and_linked():
    t = grid(40)
    v = np.array([0.25, -0.5, 0.125])
    traj = rows_of(40, (0, 10, [1.0, 2.0, 3.0], v), (20, 40, np.array([1.0, 2.0, 3.0]) + 20 * v, v))
    r = both(t, traj, fit_frames=4, max_dt=INF, gate=1e-6, gate_rate=0.0)
    assert r["next"].tolist() == [1, -1] and r["prev"].tolist() == [-1, 0] and r["cost"][0] == 0.0 and np.isnan(r["cost"][1])
    assert r["chain"].tolist() == [0, 0] and r["row_of"].tolist() == [0, 0] and r["n_chains"] == 1
    assert r["ext"].tolist() == [[0, 9, 10], [20, 39, 20]]
    assert np.array_equal(r["tail"][0][3:6], v * 128.0) and np.array_equal(r["head"][1][:3], traj[1, 20])


def test_strictly_later_never_overlapping():
    t = grid(30)
    at = lambda lo, hi: (lo, hi, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    assert both(t, rows_of(30, at(0, 10), at(10, 20)), **WIDE)["next"].tolist() == [1, -1]       # b_p = 9 = a_q - 1
    r = both(t, rows_of(30, at(0, 11), at(10, 20)), **WIDE)                                      # b_p = 10 = a_q: one frame shared
    assert r["next"].tolist() == [-1, -1] and r["n_chains"] == 2 and r["row_of"].tolist() == [0, 1] and np.isinf(r["table"]).all()
    assert both(t, rows_of(30, at(10, 20), at(0, 10)), **WIDE)["next"].tolist() == [-1, 0]       # the order of the rows is free


def test_max_dt_is_inclusive():
    t = grid(30)
    traj = rows_of(30, (0, 10, [0, 0, 0], [0, 0, 0]), (13, 20, [0, 0, 0], [0, 0, 0]))
    dt = float(t[13] - t[9])
    assert both(t, traj, **{**WIDE, "max_dt": dt})["next"].tolist() == [1, -1]
    assert both(t, traj, **{**WIDE, "max_dt": float(np.nextafter(dt, 0.0))})["next"].tolist() == [-1, -1]


def test_the_gate_is_strict_and_grows_with_dt():
    t = grid(30)
    for x, linked in ((0.25, False), (float(np.nextafter(0.25, 0.0)), True)):
        traj = rows_of(30, (5, 6, [0, 0, 0], [0, 0, 0]), (9, 10, [x, 0, 0], [0, 0, 0]))          # one sample each: c = x * x exactly
        r = both(t, traj, fit_frames=4, max_dt=INF, gate=0.25, gate_rate=0.0)                    # g2 = 0.0625 = 0.25 * 0.25
        assert (r["next"][0] == 1) == linked and (not linked or r["cost"][0] == x * x)
    traj = rows_of(30, (5, 6, [0, 0, 0], [0, 0, 0]), (9, 10, [0.25, 0, 0], [0, 0, 0]))
    assert both(t, traj, fit_frames=4, max_dt=INF, gate=0.125, gate_rate=8.0)["next"][0] == 1    # g = 0.125 + 8 * 4 / 128 = 0.375


def test_one_sample_and_failed_determinants_give_the_sample_itself():
    t = grid(20)
    traj = rows_of(20, (3, 4, [1, 2, 3], [9, 9, 9]), (8, 12, [1, 2, 3], [0.5, 0, 0]))
    r = both(t, traj, **WIDE)
    assert r["tail"][0].tolist() == [1, 2, 3, 0, 0, 0, t[3]] and r["head"][0].tolist() == r["tail"][0].tolist()
    # an equal stamp is no good time: the frame is not present, a window of two frames keeps one sample
    t2 = t.copy()
    t2[10] = t2[9]
    r = both(t2, traj, fit_frames=1, max_dt=INF, gate=1.0, gate_rate=0.0)
    assert r["ext"][1].tolist() == [8, 11, 3] and r["tail"][1].tolist() == [2.5, 2, 3, 0, 0, 0, t[11]]
    # differences that overflow: h = inf, u = NaN, det = NaN
    t3 = np.array([-1.5e308, 1.5e308, 1.6e308])
    r = both(t3, rows_of(3, (0, 2, [1, 1, 1], [1, 0, 0]), (2, 3, [0, 0, 0], [0, 0, 0])), **WIDE)
    assert r["tail"][0].tolist() == [2, 1, 1, 0, 0, 0, 1.5e308] and r["head"][0].tolist() == [1, 1, 1, 0, 0, 0, -1.5e308]


def test_bad_stamps_inside_and_beside_a_fragment_end():
    t = grid(40)
    v = [0.25, 0, 0]
    traj = rows_of(40, (0, 12, [0, 0, 0], v), (20, 40, [5.0, 0, 0], v))
    t[11] = np.nan              # the last sample of row 0 is gone: its end is frame 10
    t[9] = t[7]                 # equal to an earlier one: not a sample of the tail either
    t[20] = t[19] - 1.0         # decreasing: row 1 begins at frame 21
    t[22] = 1e300               # ... and every later frame is below it: row 1 is the frames 21 and 22
    t[30] = INF                 # (not finite: never a good time, and it hides nothing)
    r = both(t, traj, **{**WIDE, "gate": 10.0})
    assert r["ext"].tolist() == [[0, 10, 10], [21, 22, 2]] and r["next"].tolist() == [1, -1]
    assert np.allclose(r["tail"][0][:6], [2.5, 0, 0, 32.0, 0, 0], rtol=1e-14, atol=0.0)
    assert r["head"][1][:6].tolist() == [5.25, 0, 0, 0.25 / 1e300, 0, 0]


def test_equal_costs_fall_to_the_lower_row():
    t = grid(30)
    z = [0, 0, 0]
    two_tails = rows_of(30, (0, 5, [1, 0, 0], z), (0, 6, [1, 0, 0], z), (10, 20, [1.5, 0, 0], z))
    r = both(t, two_tails, **WIDE)
    assert r["table"][0, 2] == r["table"][1, 2] == 0.25 and r["next"].tolist() == [2, -1, -1] and r["n_chains"] == 2
    assert r["row_of"].tolist() == [0, 1, 0]
    two_heads = rows_of(30, (10, 20, [1.5, 0, 0], z), (11, 20, [1.5, 0, 0], z), (0, 5, [1, 0, 0], z))
    r = both(t, two_heads, **WIDE)
    assert r["next"].tolist() == [-1, -1, 0] and r["chain"].tolist() == [2, 1, 2] and r["row_of"].tolist() == [1, 0, 1]


def test_a_triple_where_the_middle_pair_goes_first():
    """A -> B costs 4, B' -> ... : rows at x = 0, 3, 5 in time order, every pair admissible.  Sorted: (1 -> 2) 4, (0 -> 1) 9,
    (0 -> 2) 25: the first takes 2's predecessor, the second still fits, the third finds both ends taken.  In rounds: 0's best successor
    is 1, 1's best predecessor 0: (0 -> 1) and (1 -> 2) are both mutual in round one."""
    t = grid(30)
    z = [0, 0, 0]
    r = both(t, rows_of(30, (0, 5, [0, 0, 0], z), (8, 12, [3, 0, 0], z), (15, 20, [5, 0, 0], z)), **{**WIDE, "gate": 10.0})
    assert r["next"].tolist() == [1, 2, -1] and np.allclose(r["cost"][:2], [9.0, 4.0], rtol=1e-14) and r["chain"].tolist() == [0, 0, 0]
    assert st.associate_rounds(r["table"])[3] == 1
    # 0 and 1 both want 2, and 2 wants 1: 0 has to look again and finds nothing
    r = both(t, rows_of(30, (0, 5, [0, 0, 0], z), (0, 6, [3, 0, 0], z), (15, 20, [5, 0, 0], z)), **{**WIDE, "gate": 10.0})
    assert r["next"].tolist() == [-1, 2, -1] and r["row_of"].tolist() == [0, 1, 1] and r["n_chains"] == 2


def test_rounds_of_mutual_pairs_equal_the_sorted_walk_on_tables_full_of_ties():
    rng = np.random.default_rng(5)
    for n in range(200):
        R = int(rng.integers(1, 12))
        table = rng.integers(0, 6, (R, R)).astype(np.float64)
        table[rng.uniform(size=(R, R)) < 0.4] = INF
        table[np.tril_indices(R)] = INF                            # links run forward
        a, b = st.associate_sorted(table), st.associate_rounds(table)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and ts.same_bits(a[2], b[2]), n


def test_an_empty_row_and_a_single_row():
    t = grid(20)
    traj = rows_of(20, (0, 5, [0, 0, 0], [0, 0, 0]), (0, 0, [0, 0, 0], [0, 0, 0]), (8, 12, [0, 0, 0], [0, 0, 0]))
    r = both(t, traj, **WIDE)
    assert r["ext"][1].tolist() == [-1, -1, 0] and r["next"].tolist() == [2, -1, -1] and r["prev"].tolist() == [-1, -1, 0]
    assert r["chain"].tolist() == [0, 1, 0] and r["row_of"].tolist() == [0, -1, 0] and r["n_chains"] == 1
    r = both(t, traj[:1], **WIDE)
    assert (r["next"][0], r["prev"][0], r["chain"][0], r["row_of"][0], r["n_chains"]) == (-1, -1, 0, 0, 1) and np.isnan(r["cost"][0])
    r = both(t, traj[1:2], **WIDE)
    assert (r["chain"][0], r["row_of"][0], r["n_chains"]) == (0, -1, 0)


def test_the_ladder_commits_one_pair_per_round():
    t, traj = st.ladder(64)
    r = both(t, traj, **st.LADDER)
    assert st.chains_of(r) == [list(range(64))] and st.associate_rounds(r["table"])[3] == 63
    assert (np.diff(r["cost"][:63]) < 0).all()                     # the far end is the cheapest: it commits first


def test_the_tracked_flight_is_stitched_into_its_four_markers():
    """What tests/test_gpu_track_stitch.py relies on: on this session the statement alone recovers every chain, no case excluded."""
    from mocap_core import helpers
    t, xyz, n_pts, slot_of, hidden = st.flight_session()
    mk = mt.Tracker(**st.FLIGHT_TRACKER).run(t, xyz, n_pts)
    truth = st.flight_truth(mk["id"], slot_of)
    assert sorted(len(c) for c in truth) == [2, 2, 3, 3] and sum(len(c) for c in truth) == 4 + len(hidden)   # ids really split
    relabel, rows = helpers.track_table(mk["id"], mk["hits"], **st.FLIGHT_TABLE)
    assert rows.size == 10
    traj = ts.gather(xyz, n_pts, mk["id"], relabel, rows.size, mk["hits"], st.FLIGHT_TABLE["min_hits"])
    r = both(t, traj, **st.FLIGHT_STITCH)
    assert r["n_chains"] == 4 and sorted(rows[c].tolist() for c in st.chains_of(r)) == sorted(truth)
    # the margins: the worst true link against its gate, the best wrong pair against the widest gate
    wide = st.stitch(t, traj, **{**st.FLIGHT_STITCH, "gate": 100.0})["table"]
    wrong = wide[np.isfinite(wide) & ~np.isfinite(r["table"])].min()
    print(f"true links cost {np.nanmax(r['cost']):.2e} at most, wrong pairs {wrong:.2e} at least")
    assert np.nanmax(r["cost"]) < 0.5 * 0.03 ** 2 * 4 and wrong > 1.0
    relabel2 = helpers.stitch_table(relabel, r["row_of"])
    again = ts.gather(xyz, n_pts, mk["id"], relabel2, 4, mk["hits"], 1)
    for row, chain in zip(again, st.chains_of(r)):
        assert np.array_equal(np.isfinite(row[:, 0]), np.isfinite(traj[chain][:, :, 0]).any(axis=0))


def test_stitch_table():
    from mocap_core import helpers
    relabel = np.array([0, -1, 1, 2, -1, 3], dtype=np.int32)
    out = helpers.stitch_table(relabel, np.array([1, 0, -1, 1], dtype=np.int32))
    assert out.tolist() == [1, -1, 0, -1, -1, 1] and out.dtype == np.int32
    assert helpers.stitch_table(np.array([-1], dtype=np.int32), np.array([0], dtype=np.int32)).tolist() == [-1]


def test_the_two_symbols_are_declared_exported_and_bound():
    from mocap_core import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mocap_core.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for n in ("mocap_stitch_tracks", "mocap_stitch_tracks_dev"):
        assert re.search(r"\bint %s\s*\(" % n, header), n
        assert re.search(r" T %s$" % n, exported, flags=re.M), n
        assert n in capi.SIGNATURES and len(capi.SIGNATURES[n][1]) == 16
        assert callable(getattr(capi.MocapCore, n[len("mocap_"):]))
    assert "#define MOCAP_ST_MAX_FIT 64" in header and capi.ST_MAX_FIT == 64
