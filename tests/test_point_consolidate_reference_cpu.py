"""CPU: the "point consolidation" contract (include/mocap_core.h) as tests/point_consolidate_reference.py states it -- hand-written
frames, the device's rounds against the sorted walk, the three symbols, and what the rule does to the frame path's own points."""
import os
import re
import subprocess

import numpy as np
import pytest

import point_consolidate_reference as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mocap_set_point_consolidation", "mocap_consolidate_points", "mocap_consolidate_points_dev")


def _rows(*rows):
    return np.array(rows, dtype=np.int16)


def _both(err, corr):
    a, b = pc.select_sorted(err, corr), pc.select_rounds(err, corr)
    assert a == b
    return a


# ---------------------------------------------------------------- hand-written frames
def test_chain_a_b_c_keeps_a_and_c():
    # A and B share camera 0's blob 3, B and C camera 1's blob 5; key(A) < key(B) < key(C) by the error
    corr = _rows([3, 1, 0], [3, 5, 1], [4, 5, 2])
    assert _both([0.1, 0.2, 0.3], corr) == [0, 2]
    # ... whatever the order of the slots
    assert _both([0.3, 0.2, 0.1], corr[::-1].copy()) == [0, 2]
    # B first in the order: it suppresses both
    assert _both([0.2, 0.1, 0.3], corr) == [1]


def test_more_views_beat_the_smaller_error():
    two = [7, 2, -1, -1, -1, -1, -1, -1]
    eight = [7, 0, 1, 2, 3, 4, 5, 6]
    assert _both([0.01, 5.0], _rows(two, eight)) == [1]
    assert _both([5.0, 0.01], _rows(eight, two)) == [0]


def test_equal_views_and_error_bits_are_decided_by_index():
    corr = _rows([1, 2, -1], [1, -1, 4], [9, 2, -1])
    assert _both([0.5, 0.5, 0.5], corr) == [0]
    # -0.0 and 0.0 are different bits: 0.0 (all zero) is the smaller unsigned integer
    assert _both([-0.0, 0.0], _rows([1, 2], [1, 3])) == [1]
    assert pc.keys([-0.0, 0.0], _rows([1, 2], [1, 3]))[0][1] == 1 << 63


def test_a_point_without_conflict_is_kept():
    corr = _rows([0, 0, -1], [1, 1, -1], [-1, -1, -1], [0, 2, -1])
    assert _both([0.3, 0.2, 0.1, 0.4], corr) == [0, 1, 2]          # 3 loses blob 0 to 0; 1 and the point with no view conflict with nothing
    assert _both([], np.zeros((0, 3), dtype=np.int16)) == []


def test_all_points_sharing_one_blob_leave_one():
    corr = np.full((9, 4), -1, dtype=np.int16)
    corr[:, 2] = 6
    corr[:, 0] = np.arange(9)
    err = np.linspace(0.9, 0.1, 9)
    assert _both(err, corr) == [8]


def test_compaction_moves_rows_together_and_leaves_the_rest():
    xyz, err, corr, n = pc.random_rows(np.random.default_rng(0), 6, 4, 12, 3)
    status = np.array([0, 1, 2, 4, 8, 0], dtype=np.int32)          # ROUNDED (8) is informational: processed
    n[5] = 13                                                      # more than K_max: untouched
    out = pc.consolidate(xyz, err, corr, n, status)
    assert out["n_in"].tolist() == [int(n[0]), -1, -1, -1, int(n[4]), -1]
    for f in (1, 2, 3, 5):
        assert all(np.array_equal(out[k][f], v[f]) for k, v in (("xyz", xyz), ("err", err), ("corr", corr), ("n_pts", n)))
    for f in (0, 4):
        m, s = int(out["n_pts"][f]), out["src"][f]
        assert 0 < m < n[f] and (np.diff(s[:m]) > 0).all() and (s[m:] == -1).all()
        assert np.array_equal(out["xyz"][f, :m], xyz[f, s[:m]]) and np.array_equal(out["corr"][f, :m], corr[f, s[:m]])
        assert np.array_equal(out["err"][f, m:], err[f, m:]) and np.array_equal(out["corr"][f, m:], corr[f, m:])
        assert not pc.shares_a_blob(out["corr"][f, :m])
    bad = corr.copy()
    bad[0, 0, 0] = 256
    assert pc.consolidate(xyz, err, bad, n, status)["n_in"][0] == -1


# ---------------------------------------------------------------- rounds == sorted walk
@pytest.mark.parametrize("C", [2, 8, 64])
@pytest.mark.parametrize("K", [1, 16, 64, 65, 200])
def test_rounds_equal_the_sorted_walk_on_random_rows(C, K):
    rng = np.random.default_rng(1000 * C + K)
    longest = 0
    for blob_range, levels in ((max(2, K // 2), 0), (max(2, K), 3), (max(2, K // 8), 0)):
        xyz, err, corr, n = pc.random_rows(rng, 3, C, K, blob_range, n_pts=[K, K, max(1, K // 2)], p_none=1.0 - 1.5 / C, err_levels=levels,
                                            chain=12)
        for f in range(3):
            e, r = err[f, :n[f]], corr[f, :n[f]]
            kept, rounds = pc.select_rounds(e, r, want_rounds=True)
            assert kept == pc.select_sorted(e, r)
            assert not pc.shares_a_blob(r[kept])
            longest = max(longest, rounds)
    if K >= 16:
        assert longest >= 4, longest            # chains of length >= 4 occur: the rounds are exercised, not one pass


# ---------------------------------------------------------------- the symbols
def test_the_three_symbols_are_declared_exported_and_bound():
    from mocap_core import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mocap_core.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mocap_[a-z_0-9]+)\s*\(", text))
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    lib = capi.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert re.search(r"\sT\s+%s\b" % name, exported), name
        assert name in capi.SIGNATURES and getattr(lib, name) is not None, name
        args = re.search(name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(capi.SIGNATURES[name][1]) == len(args.split(",")), name
    assert (capi.CONSOLIDATE_OFF, capi.CONSOLIDATE_BLOBS, capi.PC_MAX_POINTS) == (0, 1, pc.MAX_POINTS)
    for name, value in (("MOCAP_CONSOLIDATE_OFF", 0), ("MOCAP_CONSOLIDATE_BLOBS", 1)):
        assert re.search(name + r"\s*=\s*%d\b" % value, text), name
    assert re.search(r"#define\s+MOCAP_PC_MAX_POINTS\s+256\b", text)
    for method in ("set_point_consolidation", "consolidate_points", "consolidate_points_dev"):
        assert callable(getattr(capi.MocapCore, method))
    from mocap_core import helpers
    assert callable(helpers.set_point_consolidation) and helpers._state["consolidate"] == capi.CONSOLIDATE_OFF


# ---------------------------------------------------------------- the purpose, on the Python oracle
def test_no_marker_keeps_two_points_on_the_bench_stream():
    from oracle import mocap_oracle as mo
    rig, blobs, counts, _, markers = pc.drift_stream(24, drift=False)
    Ftab = mo.fundamental_table(rig["K"], rig["R"], rig["t"])
    twins_before = one_after = 0
    for f in range(24):
        r = mo.find_point_correspondance_and_object_points(blobs[f], counts[f], rig["K"], rig["R"], rig["t"], Ftab=Ftab)
        twins_before += int((pc.points_per_marker(r["object_points"], markers[f])[0] >= 2).sum())
        kept = pc.select_sorted(r["errors"], r["corr"])
        at, _ = pc.points_per_marker(r["object_points"][kept], markers[f])
        assert at.max() <= 1, (f, at.tolist())
        assert not pc.shares_a_blob(r["corr"][kept]), f
        one_after += int((at == 1).sum())
    assert twins_before >= 24                   # the input has the problem: at least one doubled marker per frame on average
    assert one_after >= 12 * 24                 # ... and the rule keeps the markers: twelve of sixteen per frame on average
