"""No GPU: the constructed frames of tests/locate_cases.py do what their labels claim, and the restatement
(oracle.mocap_oracle.locate_objects) gives on them what the reference's own function gave
(tests/golden/locate_edges.npz, recorded by oracle/make_golden.py golden_locate_edges)."""
import collections

import numpy as np

import locate_cases as lc
from conftest import load_golden


def test_each_edge_flips_the_object_count():
    """The adjacent doubles on either side of each threshold: 1 object inside, none outside, along every axis and in every index
    order; the pair's order of meeting decides the heading's sign; frames with all y == 0 give droneIndex 1."""
    cs = lc.case_set("exact")
    st = lc.statement(cs)
    assert len(cs["labels"]) == 4 * 2 * 3 * 6
    for f, label in enumerate(cs["labels"]):
        assert st["n_obj"][f] == (1 if "/inside/" in label else 0), label
    inside = [f for f, label in enumerate(cs["labels"]) if "/inside/" in label]
    head = {cs["labels"][f]: st["heading"][f, 0] for f in inside}
    # pairs along y: hx == 0, the reference's arctan2 is +-pi/2 exactly (on the branch `heading > pi/2`), both signs occur
    along_y = [h for label, h in head.items() if label.startswith("pair_") and "/axis1/" in label]
    assert sorted(set(along_y)) == [-np.pi / 2, np.pi / 2] and len(along_y) == 12
    # pairs along x: the reference returns -0.0 for both orders of the pair
    along_x = np.array([h for label, h in head.items() if "/axis0/" in label and not label.startswith("lead_upper")])
    assert len(along_x) == 18 and (along_x == 0).all() and np.signbit(along_x).all()
    for f in inside:
        n = int(cs["n_pts"][f])
        if (cs["xyz"][f, :n, 1] == 0).all():
            assert st["droneIndex"][f, 0] == 1, cs["labels"][f]
    assert set(st["droneIndex"][inside, 0].tolist()) == {0, 1}
    assert {tuple(p) for p in st["pair"][inside, 0].tolist()} == {(0, 1), (0, 2), (1, 2)}      # the smaller index is met first


def edge_shares(name):
    cs = lc.case_set(name)
    st = lc.statement(cs)
    found, frames = collections.Counter(), collections.Counter()
    for f, label in enumerate(cs["labels"]):
        frames[label.split("/")[0]] += 1
        found[label.split("/")[0]] += int(st["n_obj"][f])
    assert (st["n_obj"] <= 1).all()
    return found, frames


def test_shifted_and_turned_edges_are_decided_by_the_last_bit():
    """The "inside" triangles moved off the origin: the distances are inexact and an object is found in some frames, not in others.
    Statement's counts of 200 translations each: lead_lower 199, lead_upper 108, pair_upper 127, pair_lower 200 -- a translation
    leaves the difference along the axis a function of the offset's binade alone (and +-0.0625 adds exactly), so only the two
    upper edges are open to it; of 100 random poses each every edge is (the counts are printed by this test)."""
    found, frames = edge_shares("shifted")
    print("shifted:", dict(found))
    assert all(frames[e] >= 200 for e in lc.EDGES)
    for e in ("lead_upper", "pair_upper"):
        assert 0.25 * frames[e] <= found[e] <= 0.75 * frames[e], (e, found[e])
    found_t, frames_t = edge_shares("turned")
    print("turned:", dict(found_t))
    for e in lc.EDGES:
        assert 0.25 * frames_t[e] <= found_t[e] <= 0.75 * frames_t[e], (e, found_t[e])
    both = sum(found.values()) + sum(found_t.values())
    assert 0.25 <= both / (sum(frames.values()) + sum(frames_t.values())) <= 0.75


def test_shared_and_skipped_points():
    cs = lc.case_set("sharing")
    st = lc.statement(cs)
    by = {label: f for f, label in enumerate(cs["labels"])}
    diamonds = [f for label, f in by.items() if label.startswith("diamond/")]
    assert len(diamonds) == 24
    for f in diamonds:       # two objects on ONE base pair: the pair is never checked against the matched set
        assert st["n_obj"][f] == 2 and np.array_equal(st["pos"][f, 0], st["pos"][f, 1]), cs["labels"][f]
        assert sorted(st["droneIndex"][f, :2].tolist()) == [0, 1]
        assert np.array_equal(st["pair"][f, 0], st["pair"][f, 1])
    # a base point that would itself lead a triangle: skipped once matched, leads when it comes first
    f = by["skip/lead_first"]
    assert st["n_obj"][f] == 1 and st["lead"][f, 0] == 0 and st["pair"][f, 0].tolist() == [1, 2]
    assert st["n_obj"][by["skip/lead_last"]] == 2 and st["n_obj"][by["skip/pair_first"]] == 2
    # the fan: five matches, the rows of the first three fail in full
    f = by["fan/order012345"]
    assert st["n_obj"][f] == 1 and st["lead"][f, 0] == 0 and st["pair"][f, 0].tolist() == [4, 5]
    assert all(st["n_obj"][g] == 1 for label, g in by.items() if label.startswith("fan/"))


def test_chunk_frames_find_exactly_what_was_planted():
    cs = lc.case_set("chunk")
    st = lc.statement(cs)
    assert sorted({int(label.split("/")[1][1:]) for label in cs["labels"]}) == list(lc.CHUNK_K)
    for f, label in enumerate(cs["labels"]):
        kind = label.split("/")[2]
        n = int(st["n_obj"][f])
        if kind.startswith("tri"):
            lead, p1, p2 = map(int, kind[3:].split("_"))
            assert n == 1 and st["lead"][f, 0] == lead and st["pair"][f, 0].tolist() == sorted((p1, p2)), label
        elif kind.startswith("together"):
            assert n == int(kind[8:]), label
        elif kind.startswith("diamond"):
            assert n == 2, label
        elif kind.startswith("fan"):
            assert n == 1 and st["lead"][f, 0] == 130, label
        else:
            assert n == 0, label
    leads = st["lead"][st["lead"] >= 0]
    assert set((leads >> 6).tolist()) == {0, 1, 2, 3}
    assert {63, 64, 127, 128, 192, 255} <= set(leads.tolist())


def test_dense_clutter_reaches_every_word():
    cs = lc.case_set("dense")
    st = lc.statement(cs)
    assert len(cs["labels"]) <= 24 and len(lc.dense_recorded(cs)) == 12
    per_k = collections.defaultdict(list)
    for f, label in enumerate(cs["labels"]):
        per_k[int(label.split("/")[1][1:])].append(int(st["n_obj"][f]))
        if label.startswith("dense/K256/"):
            assert lc.lead_words(st, f) == [0, 1, 2, 3] and st["n_obj"][f] > 12, label
    print("dense objects per K:", dict(per_k))
    assert sorted(per_k) == [63, 64, 65, 129, 256] and all(min(v) > 12 for v in per_k.values())


def test_nonfinite_points_and_out_of_range_counts():
    cs = lc.case_set("nonfinite")
    st = lc.statement(cs)
    for f, label in enumerate(cs["labels"]):
        n = int(st["n_obj"][f])
        if label.startswith("clutter_"):
            assert n == 1 and np.isfinite(st["pos"][f, 0]).all() and np.isfinite(st["error"][f, 0]), label
        elif label.startswith(("lead_", "p1_", "p2_")):
            assert n == 0, label
        elif label.startswith("err_nan_"):
            assert n == 1 and np.isfinite(st["pos"][f, 0]).all() and np.isfinite(st["heading"][f, 0]), label
            assert np.isnan(st["error"][f, 0]) == (label != "err_nan_clutter"), label
        elif label == "err_pinf_lead":
            assert n == 1 and st["error"][f, 0] == np.inf
        else:
            count = int(label.split("/")[1])
            assert n == (1 if count in (3, 8) else 0), label
    assert {int(x) for x in cs["n_pts"]} >= {-1, 0, 1, 2, 8, 9}


def test_restatement_equals_the_reference_on_every_recorded_frame():
    """n_obj, droneIndex and pos exact; error to rtol 1e-14 and heading to 1e-12 absolute (np.mean and linalg.norm are library
    calls upstream).  The inputs in the file are the builders' own, bit for bit."""
    g = load_golden("locate_edges")
    frames = 0
    for fam, cs, idx in lc.recorded():
        st = lc.statement(cs)
        assert np.array_equal(g[fam + "_frames"], idx)
        for key in ("xyz", "err"):
            assert np.array_equal(g[f"{fam}_{key}"].view(np.uint64), cs[key][idx].view(np.uint64)), (fam, key)
        assert np.array_equal(g[fam + "_n_pts"], cs["n_pts"][idx])
        assert np.array_equal(g[fam + "_ref_nobj"], st["n_obj"][idx]), fam
        O = g[fam + "_ref_drone"].shape[1]
        assert O == max(1, int(st["n_obj"][idx].max()))
        have = np.arange(O)[None, :] < g[fam + "_ref_nobj"][:, None]
        assert np.array_equal(g[fam + "_ref_drone"][have], st["droneIndex"][idx][:, :O][have]), fam
        assert np.array_equal(g[fam + "_ref_pos"][have], st["pos"][idx][:, :O][have]), fam
        np.testing.assert_allclose(st["error"][idx][:, :O][have], g[fam + "_ref_error"][have], rtol=1e-14, atol=0)
        np.testing.assert_allclose(st["heading"][idx][:, :O][have], g[fam + "_ref_heading"][have], rtol=0, atol=1e-12)
        frames += len(idx)
    assert frames > 1000


def test_tiling_puts_small_frames_behind_the_dense_one():
    """grid_bank + tile_index: workgroup 0 of the wave search walks the dense frame, then a 3-point triangle, then a count out of
    range; the tiled expectation is the bank's statement with each frame's own error."""
    from oracle import mocap_oracle as mo
    bank = lc.case_set("grid_bank")
    assert len(bank["labels"]) == 16
    idx = lc.tile_index(8193, 16)
    assert [bank["labels"][i] for i in idx[[0, 4096, 8192]]] == ["dense256", "triangle3_after_dense", "count_257"]
    assert bank["n_pts"][idx[0]] == 256 and bank["n_pts"][idx[4096]] == 3 and bank["n_pts"][idx[8192]] == 257
    xyz, err, n_pts, want = lc.tiled(bank, 4200)
    for f in (0, 17, 4096, 4099, 4199):
        n = int(lc.effective_n(n_pts[f], 256))
        objs = mo.locate_objects(xyz[f, :n], err[f, :n])
        assert len(objs) == want["n_obj"][f]
        for j, o in enumerate(objs):
            assert o["error"] == want["error"][f, j] and o["lead"] == want["lead"][f, j]
            assert np.array_equal(o["pos"], want["pos"][f, j])
    assert len({err[f, 0] for f in (0, 16, 32)}) == 3                    # the same pattern, three different errors
