"""Rigid groups without a GPU: the plain statement of the contract (tests/rigid_groups_reference.py) on a hand-computed case and at
the edge of every rule, its tree against math.fsum, its vectorised form against its scalar form, float64 against 50 digits, the tracked
flight on which the GPU test relies, and the two C-ABI symbols (declared, exported, bound)."""
import math
import os
import re
import subprocess

import numpy as np

import body_learn_reference as bl
import marker_track_reference as mt
import rigid_groups_reference as rg
import track_smooth_reference as ts
import track_stitch_reference as st
from conftest import ROOT

INF = float("inf")
NAN = float("nan")
U = 2.0 ** -53                                     # the unit roundoff of float64
ACCURACY_BOUND = 4.0 * 1.6e-16                     # four times the measured worst (1.58e-16, printed below) of |error| / dist


def both(traj, min_common, tol, max_dist=INF, min_travel=0.0):
    a, b = rg.rigid_groups_scalar(traj, min_common, tol, max_dist, min_travel), rg.rigid_groups(traj, min_common, tol, max_dist, min_travel)
    assert rg.same(a, b)
    return b


def body_rows(F, offsets, seed=1, dropout=0.0):
    """Rows that share one seeded rigid motion: offsets [N][3] in body coordinates."""
    rng = np.random.default_rng(seed)
    Rm, c = rg.rigid_motion(rng, np.arange(F) / 120.0)
    traj = np.einsum("fij,nj->nfi", Rm, np.asarray(offsets, dtype=float)) + c[None]
    traj[rng.uniform(size=traj.shape[:2]) < dropout] = np.nan
    return traj


def test_three_frames_by_hand():
    """Row 0 at the origin, row 1 at distances 3, 5, 3 (3-4-0 triangles), row 2 absent from frame 1."""
    traj = np.array([[[0, 0, 0], [0, 0, 0], [0, 0, 0]],
                     [[3, 0, 0], [3, 4, 0], [0, 0, 3]],
                     [[0, 0, 1], [NAN, 0, 0], [0, 0, 2]]], dtype=float)
    r = both(traj, 2, 1.0)
    assert r["cnt"].tolist() == [[3, 3, 2], [3, 3, 2], [2, 2, 2]]
    mean = (3.0 + 5.0 + 3.0) / 3                   # every partial sum is an integer: the tree's order does not matter here
    assert r["dist"][0, 1] == r["dist"][1, 0] == mean
    e = [3.0 - mean, 5.0 - mean, 3.0 - mean]
    assert r["spread"][0, 1] == math.sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) / 3)       # 0.9428...
    assert r["dist"][0, 2] == 1.5 and r["spread"][0, 2] == 0.5
    assert r["dist"][1, 2] == (math.sqrt(10.0) + 1.0) / 2
    assert (np.diag(r["dist"]) == 0).all() and (np.diag(r["spread"]) == 0).all()
    assert r["travel"].tolist() == [0.0, math.sqrt((9.0 + 16.0) + 9.0), 1.0]
    # tol 1.0: 0 - 1 (0.94) and 0 - 2 (0.5) are edges, 1 - 2 (spread 1.08) is a conflict inside the one group
    assert r["spread"][1, 2] > 1.0
    assert r["n_groups"] == 1 and r["group_of"].tolist() == [0, 0, 0]
    assert (r["gsize"][0], r["ghead"][0], r["gconf"][0]) == (3, 0, 1) and r["gspread"][0] == r["spread"][0, 1]
    assert r["gsize"][1:].tolist() == [-1, -1] and np.isnan(r["gspread"][1:]).all()
    # min_travel 0.5 takes row 0 out: its edges go, 1 - 2 is none: no group
    r = both(traj, 2, 1.0, min_travel=0.5)
    assert r["n_groups"] == 0 and r["group_of"].tolist() == [-1, -1, -1] and r["gsize"].tolist() == [-1, -1, -1]


def test_the_tree_against_fsum_and_its_vectorised_form():
    rng = np.random.default_rng(2)
    for F in (1, 2, 63, 64, 65, 255, 256, 257, 600, 16384, 16385, 16640):
        v = rng.uniform(0.0, 2.0, F)
        v[rng.uniform(size=F) < 0.1] = 0.0
        s = rg.tree_sum_scalar(v.tolist())
        assert rg.same_bits(s, rg.tree_sum(v)), F
        # every value passes through at most 6 + 3 + chunk + 6 additions: |error| <= gamma_depth * sum |v|, gamma_n = n u / (1 - n u)
        depth = 6 + 3 + (((F + 255) // 256 + 63) // 64) + 6
        assert abs(s - math.fsum(v)) <= depth * U / (1 - depth * U) * math.fsum(v), F
    many = rng.uniform(0.0, 1.0, (5, 3, 700))
    assert rg.same_bits(rg.tree_sum(many), [[rg.tree_sum_scalar(r.tolist()) for r in m] for m in many])


def test_vectorised_statement_equals_the_scalar_one_bit_for_bit():
    for seed, F in ((1, 300), (2, 70), (3, 513)):
        traj, owner = rg.make_scene(seed, F, dropout=0.1)
        traj[2, :, :] = np.nan
        traj[3, 5, 1] = INF
        r = both(traj, 30, 0.003)
        assert r["n_groups"] >= 1
    both(rg.chain(12, 40), **rg.CHAIN)


def test_min_common_at_its_edge():
    traj = body_rows(80, [[0, 0, 0], [0.1, 0, 0], [0, 0.2, 0]])
    traj[1, 30:] = np.nan                                                  # rows 0 and 1 share exactly 30 frames
    traj[2, :50] = np.nan                                                  # rows 0 and 2 exactly 30, rows 1 and 2 none
    r = both(traj, 30, 1e-9)
    assert r["cnt"][0, 1] == 30 and r["cnt"][0, 2] == 30 and r["cnt"][1, 2] == 0 and np.isnan(r["dist"][1, 2]) and np.isnan(r["spread"][1, 2])
    assert r["group_of"].tolist() == [0, 0, 0] and r["gconf"][0] == 0      # 1 - 2 share nothing: no evidence, no conflict
    r = both(traj, 31, 1e-9)
    assert r["n_groups"] == 0 and r["group_of"].tolist() == [-1, -1, -1]
    traj[1, 29] = np.nan                                                   # 29 in common (and row 1 itself has 29): below min_common
    r = both(traj, 30, 1e-9)
    assert r["cnt"][0, 1] == 29 and r["group_of"].tolist() == [0, -1, 0]


def test_tol_max_dist_and_min_travel_at_their_edges():
    traj, _ = rg.make_scene(5, 200, bodies=(3,), n_loose=0, n_static=0, dropout=0.0, shuffle=False)
    r = both(traj, 30, 1.0)
    s = float(r["spread"][0, 1])
    assert 0 < s < 0.002
    assert both(traj[:2], 30, s)["group_of"].tolist() == [0, 0]             # spread <= tol: an edge at equality
    assert both(traj[:2], 30, float(np.nextafter(s, 0.0)))["group_of"].tolist() == [-1, -1]
    d = float(r["dist"][0, 1])
    assert both(traj[:2], 30, 1.0, max_dist=d)["group_of"].tolist() == [0, 0]
    assert both(traj[:2], 30, 1.0, max_dist=float(np.nextafter(d, 0.0)))["group_of"].tolist() == [-1, -1]
    tr = float(r["travel"][1])
    assert tr > 0.1
    assert both(traj[:2], 30, 1.0, min_travel=tr)["group_of"].tolist() == ([0, 0] if r["travel"][0] >= tr else [-1, -1])
    lo = float(min(r["travel"][:2]))
    assert both(traj[:2], 30, 1.0, min_travel=lo)["group_of"].tolist() == [0, 0]
    assert both(traj[:2], 30, 1.0, min_travel=float(np.nextafter(lo, INF)))["group_of"].tolist() == [-1, -1]


def test_infinite_coordinates_overflow_and_empty_rows():
    traj = body_rows(64, [[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [0.1, 0.1, 0]])
    traj[1, 7, 2] = INF                                                    # one infinite coordinate: the sample is absent
    traj[2] = np.nan                                                       # an empty row
    traj[3] = 1e200 * np.sign(traj[3])                                     # differences of 1e200: their squares overflow
    traj[3, ::2] *= 0.5
    r = both(traj, 10, 1e-6)
    assert r["cnt"][1, 1] == 63 and r["cnt"][0, 1] == 63
    assert (r["cnt"][2] == 0).all() and np.isnan(r["dist"][2]).all() and np.isnan(r["spread"][2]).all() and np.isnan(r["travel"][2])
    assert r["dist"][0, 3] == INF and np.isnan(r["spread"][0, 3]) and r["cnt"][0, 3] == 64
    assert r["dist"][3, 3] == 0.0 and r["spread"][3, 3] == 0.0 and r["travel"][3] == INF
    assert r["group_of"].tolist() == [0, 0, -1, -1, 0] and r["gconf"][0] == 0 and r["gsize"][0] == 3


def test_one_row_a_group_of_two_and_a_static_pair():
    one = body_rows(40, [[0, 0, 0]])
    r = both(one, 2, 0.01)
    assert r["n_groups"] == 0 and r["group_of"].tolist() == [-1] and r["gsize"].tolist() == [-1] and r["cnt"].tolist() == [[40]]
    two = body_rows(40, [[0, 0, 0], [0.1, 0, 0]])
    r = both(two, 2, 1e-9)
    assert r["n_groups"] == 1 and (r["gsize"][0], r["ghead"][0], r["gconf"][0]) == (2, 0, 0) and r["gspread"][0] == r["spread"][0, 1]
    # what the stage cannot know: two markers that lie still keep their distance; min_travel is the handle
    still = np.tile(np.array([[[0.0, 0, 0]], [[1.0, 2, 3]]]), (1, 40, 1))
    assert both(still, 2, 1e-9)["group_of"].tolist() == [0, 0]
    assert both(still, 2, 1e-9, min_travel=0.01)["group_of"].tolist() == [-1, -1]


def test_the_chain_is_one_group_full_of_conflicts():
    for R in (5, 64):
        traj = rg.chain(R)
        r = both(traj, **rg.CHAIN) if R == 5 else rg.rigid_groups(traj, **rg.CHAIN)
        _, edge = rg.edges_of(r["cnt"], r["dist"], r["spread"], r["travel"], **rg.CHAIN)
        assert edge.sum() == 2 * (R - 1) and all(edge[i, i + 1] for i in range(R - 1))            # consecutive rows only
        assert r["n_groups"] == 1 and (r["group_of"] == 0).all() and r["gsize"][0] == R and r["ghead"][0] == 0
        assert r["gconf"][0] == R * (R - 1) // 2 - (R - 1)                                        # every other pair
        off = r["spread"][~edge & ~np.eye(R, dtype=bool)]
        assert off.min() > 1e-3 and r["gspread"][0] < 1e-12


def test_float64_against_fifty_digits():
    """The pair statistics of the contract in float64 against exact sums of the same inputs, scaled by the pair's distance."""
    worst = 0.0
    for seed, F in ((11, 300), (12, 1000)):
        traj, _ = rg.make_scene(seed, F, bodies=(3,), n_loose=1, n_static=1, dropout=0.1)
        cnt, dist, spread = rg.pair_stats(traj)
        dm, sm = rg.pair_stats_mp(traj)
        for p in range(traj.shape[0]):
            for q in range(p + 1, traj.shape[0]):
                worst = max(worst, float(abs(dist[p, q] - dm[p][q]) / dm[p][q]), float(abs(spread[p, q] - sm[p][q]) / dm[p][q]))
    print(f"float64 against 50 digits, |error| / dist over dist and spread: worst {worst:.2e}")
    assert worst <= ACCURACY_BOUND


def flight_rows():
    """The flight through the reference tracker, the table, the gather, the stitcher and the second gather, all on the CPU."""
    from mocap_core import helpers
    t, xyz, n_pts, slot_of, owner, templates, truth = rg.flight_scene()
    mk = mt.Tracker(**rg.FLIGHT_TRACKER).run(t, xyz, n_pts)
    relabel, rows = helpers.track_table(mk["id"], mk["hits"], **rg.FLIGHT_TABLE)
    traj = ts.gather(xyz, n_pts, mk["id"], relabel, rows.size, mk["hits"], rg.FLIGHT_TABLE["min_hits"])
    s = st.stitch(t, traj, **rg.FLIGHT_STITCH)
    relabel2 = helpers.stitch_table(relabel, s["row_of"])
    again = ts.gather(xyz, n_pts, mk["id"], relabel2, s["n_chains"], mk["hits"], rg.FLIGHT_TABLE["min_hits"])
    # the marker of each row: the one whose sightings the row holds
    marker = [[m for m in range(len(owner)) if np.array_equal(np.isfinite(row[:, 0]), slot_of[m] >= 0)] for row in again]
    return t, xyz, n_pts, mk, rows, relabel2, again, marker, owner, templates


def test_the_flight_on_the_statement_alone():
    """What tests/test_gpu_rigid_groups.py relies on: ids split and are stitched back, every planted pair is rigid with a margin
    of two, every other pair is not with a margin of four, and the learner recovers the planted distances to 0.5 mm."""
    t, xyz, n_pts, mk, rows, relabel2, traj, marker, owner, templates = flight_rows()
    M = len(owner)
    assert rows.size == 2 * M and traj.shape[0] == M                           # every marker was hidden once: two ids each
    assert sorted(m[0] for m in marker) == list(range(M)) and all(len(m) == 1 for m in marker)
    own = np.array([owner[m[0]] for m in marker])
    r = rg.rigid_groups(traj, **rg.FLIGHT_GROUPS)
    tol = rg.FLIGHT_GROUPS["tol"]
    planted = (own[:, None] == own[None, :]) & (own[:, None] >= 0) & ~np.eye(M, dtype=bool)
    other = ~planted & ~np.eye(M, dtype=bool)
    print(f"planted pairs: spread {r['spread'][planted].max():.2e} at most; other pairs: {r['spread'][other].min():.2e} at least")
    assert (r["cnt"] >= rg.FLIGHT_GROUPS["min_common"]).all()
    assert r["spread"][planted].max() <= tol / 2 and r["spread"][other].min() >= 4 * tol
    assert r["n_groups"] == 2 and r["gconf"][:2].tolist() == [0, 0] and sorted(r["gsize"][:2].tolist()) == [4, 5]
    for g, members in enumerate(rg.rows_of_groups(r)):
        assert len({own[i] for i in members}) == 1 and own[members[0]] >= 0
    assert (r["group_of"][own < 0] == -1).all()
    # the learner on the relabelled capture, sel = rows: every pair distance within 0.5 mm of the planted one
    row_id = np.where(mk["id"] >= 0, relabel2[np.clip(mk["id"], 0, relabel2.size - 1)], -1).astype(np.int32)
    for members in rg.rows_of_groups(r):
        q = templates[own[members[0]]]
        mine = [marker[i][0] - (0 if own[members[0]] == 0 else rg.FLIGHT_BODIES[0]) for i in members]
        learned = bl.learn(xyz, n_pts, row_id, members)
        assert learned["status"] == 0 and learned["frames_used"] >= 100
        L = np.asarray(learned["markers"])
        for i in range(len(members)):
            for j in range(i):
                assert abs(np.linalg.norm(L[i] - L[j]) - np.linalg.norm(q[mine[i]] - q[mine[j]])) <= 0.0005, (members, i, j)


def test_groups_that_are_no_body_are_skipped_with_a_reason():
    """learn_session_bodies on groups given by hand: two rows, nine rows and a linkage never reach the learner (no GPU needed)."""
    from mocap_core import helpers
    group = lambda rows, conflicts=0: {"rows": rows, "ids": rows, "size": len(rows), "conflicts": conflicts, "max_spread": 0.0,
                                       "dist": np.zeros((len(rows), len(rows)))}
    capture = {"xyz": np.zeros((4, 2, 3)), "n_pts": np.zeros(4, dtype=np.int32), "id": np.array([[0, 5], [-1, 99], [2, 1], [3, 3]], dtype=np.int32)}
    session = {"relabel": np.array([1, -1, 0, 0], dtype=np.int32)}
    groups = [group([0, 1]), group(list(range(9))), group([0, 1, 2], conflicts=1)]
    learned, skipped = helpers.learn_session_bodies(capture, session, groups)
    assert learned == [] and [g for g, _ in skipped] == groups
    assert "2 rows" in skipped[0][1] and "9 rows" in skipped[1][1] and "not rigid" in skipped[2][1]
    assert capture["id"].tolist() == [[0, 5], [-1, 99], [2, 1], [3, 3]]                # the caller's ids are left alone


def test_the_two_symbols_are_declared_exported_and_bound():
    from mocap_core import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mocap_core.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for n in ("mocap_rigid_groups", "mocap_rigid_groups_dev"):
        assert re.search(r"\bint %s\s*\(" % n, header), n
        assert re.search(r" T %s$" % n, exported, flags=re.M), n
        assert n in capi.SIGNATURES and len(capi.SIGNATURES[n][1]) == 18
        assert callable(getattr(capi.MocapCore, n[len("mocap_"):]))
    assert "#define MOCAP_RG_MAX_ROWS 256" in header and capi.RG_MAX_ROWS == 256
    assert "#define MOCAP_RG_MAX_FRAMES 4194304" in header and capi.RG_MAX_FRAMES == 4194304
    assert capi.MocapCore.RIGID_OUT == ("cnt", "dist", "spread", "travel", "group_of", "gsize", "ghead", "gconf", "gspread", "n_groups")
