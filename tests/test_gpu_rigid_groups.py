"""Rigid groups on the device (include/mocap_core.h, "rigid groups"; csrc/rigid_groups.hip) against the plain statement of the
contract (tests/rigid_groups_reference.py): cnt, group_of, gsize, ghead, gconf and n_groups exactly; dist, spread, travel and gspread
bit for bit (any NaN equal to any NaN), at the frame counts where the tree changes path and the row counts around a block of pairs;
every rule at its edge with the parameter taken from the statement's own value; the chain; the host and device forms, call after
call, a second stream, behind the gather, the sentinel, the refusals; and a tracked session end to end."""
import numpy as np
import pytest

import rigid_groups_reference as rg

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
OUT = ("cnt", "dist", "spread", "travel", "group_of", "gsize", "ghead", "gconf", "gspread", "n_groups")
SENTINEL = -7


def outputs(R, make, fill):
    """The ten outputs pre-filled with the sentinel; make(shape, dtype name, fill)."""
    o = {"cnt": make((R, R), "int32", fill), "n_groups": make((1,), "int32", fill)}
    o.update({k: make((R, R), "float64", float(fill)) for k in ("dist", "spread")})
    o.update({k: make((R,), "float64", float(fill)) for k in ("travel", "gspread")})
    o.update({k: make((R,), "int32", fill) for k in ("group_of", "gsize", "ghead", "gconf")})
    return o


def host_outputs(R):
    return outputs(R, lambda shape, dt, fill: np.full(shape, fill, dtype=dt), SENTINEL)


def dev_groups(core, traj, min_common, tol, max_dist=INF, min_travel=0.0):
    """mocap_rigid_groups_dev into outputs pre-filled with the sentinel -> host arrays."""
    import torch
    dev = torch.device("cuda", 0)
    R, F, _ = traj.shape
    d_traj = torch.from_numpy(np.ascontiguousarray(traj)).to(dev)
    o = outputs(R, lambda shape, dt, fill: torch.full(shape, fill, dtype=getattr(torch, dt), device=dev), SENTINEL)
    torch.cuda.synchronize()
    core.rigid_groups_dev(F, R, d_traj.data_ptr(), min_common, tol, max_dist, min_travel, *[o[k].data_ptr() for k in OUT])
    core.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["n_groups"] = int(got["n_groups"][0])
    return got


def assert_equal(got, ref, what):
    for k in rg.INT_OUT:
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5].tolist())
    assert got["n_groups"] == ref["n_groups"], what
    for k in rg.F64_OUT:
        assert rg.same_bits(got[k], ref[k]), (what, k)


def session(seed, F, R):
    """R rows over F frames: bodies of three rows each under motions of their own (the first rows), then loose rows; 8 % dropout.
    With four or more rows one is all NaN and one is the overflow row (coordinates of +-1e200 that change: D overflows, spread is
    NaN).  (R = 256 is 528 block pairs: three rounds of launches over the one slab.)"""
    n_bodies = max((R - 2) // 4, 1) if R >= 3 else 0
    n_loose = R - 3 * n_bodies
    traj, _ = rg.make_scene(seed, F, bodies=(3,) * n_bodies, n_loose=n_loose, n_static=0, dropout=0.08 if F > 2 else 0.0, shuffle=False)
    assert traj.shape[0] == R
    if R >= 4:
        traj[R - 1] = np.nan
        traj[R - 2] = 1e200 * np.where(np.arange(F)[:, None] % 2 == 0, 1.0, -0.5)
    return traj


# ---------------------------------------------------------------- 1. the device against the statement: frames, rows
@pytest.mark.parametrize("R", [2, 8])
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 255, 256, 257, 600, 16384, 16385])
def test_frame_counts_where_the_tree_changes_path(core, F, R):
    traj = session(F + R, F, R)
    min_common = 2 if F < 100 else 30
    ref = rg.rigid_groups(traj, min_common, 0.003)
    assert_equal(dev_groups(core, traj, min_common, 0.003), ref, (F, R))
    if F >= 255 and R == 8:
        assert ref["n_groups"] >= 1 and np.isnan(ref["spread"][R - 2, 0]) and ref["dist"][R - 2, 0] == INF and ref["cnt"][R - 1, R - 1] == 0


@pytest.mark.parametrize("R", [1, 2, 3, 8, 9, 64, 65, 256])
def test_row_counts_around_a_block_and_at_the_cap(core, R):
    traj = session(100 + R, 300, R)
    ref = rg.rigid_groups(traj, 30, 0.003, max_dist=0.5, min_travel=0.05)
    assert_equal(dev_groups(core, traj, 30, 0.003, max_dist=0.5, min_travel=0.05), ref, R)
    if R >= 8:
        assert ref["n_groups"] == max((R - 2) // 4, 1) and (ref["gsize"][:ref["n_groups"]] == 3).all() and (ref["gconf"][:ref["n_groups"]] == 0).all()


# ---------------------------------------------------------------- 2. every rule at its edge
def test_common_frames_across_the_tile_edge(core):
    """One body of eight rows; row 0 is always there, the others on runs that end on the frames 255, 256, 257 and are min_common or
    min_common - 1 long: the first are linked to row 0, the second are not (their own count is below min_common as well)."""
    F, n = 600, 30
    rng = np.random.default_rng(7)
    Rm, c = rg.rigid_motion(rng, np.arange(F) / 120.0)
    traj = np.einsum("fij,nj->nfi", Rm, rg.template(rng, 8)) + c[None]
    runs = [None, (226, 256), (227, 256), (227, 257), (228, 257), (228, 258), (229, 258), (250, 280)]
    for r, run in enumerate(runs):
        if run:
            traj[r, :run[0]] = np.nan
            traj[r, run[1]:] = np.nan
    ref = rg.rigid_groups(traj, n, 1e-9)
    assert ref["cnt"][0].tolist() == [F, 30, 29, 30, 29, 30, 29, 30]
    assert ref["group_of"].tolist() == [0, 0, -1, 0, -1, 0, -1, 0] and ref["gconf"][0] == 0
    assert ref["cnt"][1, 3] == 29 and ref["cnt"][3, 5] == 29                    # in the group through row 0 alone
    assert_equal(dev_groups(core, traj, n, 1e-9), ref, "runs")
    assert_equal(dev_groups(core, traj, n + 1, 1e-9), rg.rigid_groups(traj, n + 1, 1e-9), "one more")


def test_tol_max_dist_and_min_travel_taken_from_the_statement(core):
    traj, _ = rg.make_scene(5, 300, bodies=(3,), n_loose=1, n_static=1, dropout=0.05, shuffle=False)
    base = rg.rigid_groups(traj, 30, 1.0)
    s, d = float(base["spread"][0, 1]), float(base["dist"][0, 1])
    lo = float(min(base["travel"][:2]))
    two = traj[:2]
    cases = [(dict(tol=s), [0, 0]), (dict(tol=float(np.nextafter(s, 0.0))), [-1, -1]),
             (dict(tol=1.0, max_dist=d), [0, 0]), (dict(tol=1.0, max_dist=float(np.nextafter(d, 0.0))), [-1, -1]),
             (dict(tol=1.0, min_travel=lo), [0, 0]), (dict(tol=1.0, min_travel=float(np.nextafter(lo, INF))), [-1, -1])]
    for kw, want in cases:
        ref = rg.rigid_groups(two, 30, **kw)
        assert ref["group_of"].tolist() == want, kw
        assert_equal(dev_groups(core, two, 30, **kw), ref, kw)
    n = int(base["cnt"][0, 1])
    for min_common, want in ((n, [0, 0]), (n + 1, [-1, -1])):
        ref = rg.rigid_groups(two, min_common, 1.0)
        assert ref["group_of"].tolist() == want
        assert_equal(dev_groups(core, two, min_common, 1.0), ref, min_common)
    # the whole scene at the same edges: the static row falls to min_travel, the loose one to tol
    for kw in (dict(tol=s), dict(tol=0.003, min_travel=0.01), dict(tol=0.003, max_dist=d)):
        assert_equal(dev_groups(core, traj, 30, **kw), rg.rigid_groups(traj, 30, **kw), kw)


@pytest.mark.parametrize("R", [64, 256])
def test_the_chain(core, R):
    traj = rg.chain(R)
    ref = rg.rigid_groups(traj, **rg.CHAIN)
    assert ref["n_groups"] == 1 and ref["gsize"][0] == R and ref["gconf"][0] == R * (R - 1) // 2 - (R - 1)
    assert_equal(dev_groups(core, traj, **rg.CHAIN), ref, R)


# ---------------------------------------------------------------- 3. host form, repeated calls, streams, chaining, sentinel
def test_host_and_device_forms_streams_and_repeated_calls_give_the_same_bytes(core):
    import torch
    traj = session(5, 600, 9)
    host = core.rigid_groups(traj, 30, 0.003, max_dist=1.0, min_travel=0.01)
    one = dev_groups(core, traj, 30, 0.003, 1.0, 0.01)
    two = dev_groups(core, traj, 30, 0.003, 1.0, 0.01)
    stream = torch.cuda.Stream(device=0)
    try:
        core.set_stream(stream.cuda_stream)
        other = dev_groups(core, traj, 30, 0.003, 1.0, 0.01)
    finally:
        core.set_stream(0)
    for k in OUT[:-1]:
        assert host[k].tobytes() == one[k].tobytes() == two[k].tobytes() == other[k].tobytes(), k
        assert host[k].dtype == one[k].dtype and host[k].shape == one[k].shape
    assert host["n_groups"] == one["n_groups"] == two["n_groups"] == other["n_groups"]
    assert_equal(host, rg.rigid_groups(traj, 30, 0.003, 1.0, 0.01), "host")


def test_chained_behind_the_gather(core):
    """mocap_gather_tracks_dev and mocap_rigid_groups_dev on the context's stream with nothing in between: the rows are read where
    the gather wrote them."""
    import torch
    import track_smooth_reference as ts
    dev = torch.device("cuda", 0)
    traj, _ = rg.make_scene(9, 300, dropout=0.05)
    R, F, _ = traj.shape
    rng = np.random.default_rng(9)
    K = 16
    xyz, ids, n_pts = np.full((F, K, 3), np.nan), np.full((F, K), -1, dtype=np.int32), np.zeros(F, dtype=np.int32)
    for f in range(F):
        there = rng.permutation(np.flatnonzero(np.isfinite(traj[:, f, 0])))
        xyz[f, :there.size], ids[f, :there.size], n_pts[f] = traj[there, f], there + 3, there.size
    relabel = np.concatenate([[-1, -1, -1], np.arange(R)]).astype(np.int32)
    assert rg.same_bits(ts.gather(xyz, n_pts, ids, relabel, R), traj)
    d = [torch.from_numpy(a).to(dev) for a in (xyz, n_pts, ids, relabel)]
    rows = torch.full((R, F, 3), float(SENTINEL), dtype=torch.float64, device=dev)
    o = outputs(R, lambda shape, dt, fill: torch.full(shape, fill, dtype=getattr(torch, dt), device=dev), SENTINEL)
    torch.cuda.synchronize()
    core.gather_tracks_dev(F, K, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 0, relabel.size, d[3].data_ptr(), R, rows.data_ptr())
    core.rigid_groups_dev(F, R, rows.data_ptr(), 30, 0.003, INF, 0.0, *[o[k].data_ptr() for k in OUT])
    core.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["n_groups"] = int(got["n_groups"][0])
    ref = rg.rigid_groups(traj, 30, 0.003)
    assert ref["n_groups"] == 2
    assert_equal(got, ref, "chained")


def test_outputs_prefilled_with_a_sentinel_are_fully_overwritten(core):
    traj = session(6, 257, 9)
    got = dev_groups(core, traj, 30, 0.003)
    for k in OUT[:-1]:
        assert not (got[k] == SENTINEL).any(), k
    assert got["n_groups"] != SENTINEL
    assert np.isnan(got["travel"][8]) and got["group_of"][8] == -1 and (got["cnt"][8] == 0).all() and np.isnan(got["dist"][8]).all()
    assert (got["gsize"][got["n_groups"]:] == -1).all() and np.isnan(got["gspread"][got["n_groups"]:]).all()


# ---------------------------------------------------------------- 4. refusals
def test_every_refusal_leaves_its_outputs_untouched(core):
    from mocap_core import capi
    from mocap_core.capi import _p
    F, R = 120, 3
    traj = session(3, F, R)
    ok = dict(F=F, R=R, n=30, tol=0.003, max_dist=INF, travel=0.0)
    bad = [("F 0", dict(F=0)), ("F above the cap", dict(F=capi.RG_MAX_FRAMES + 1)), ("R 0", dict(R=0)), ("R 257", dict(R=257)),
           ("min_common 1", dict(n=1)), ("min_common 0", dict(n=0)), ("tol 0", dict(tol=0.0)), ("tol < 0", dict(tol=-1.0)),
           ("tol inf", dict(tol=INF)), ("tol NaN", dict(tol=NAN)), ("max_dist 0", dict(max_dist=0.0)), ("max_dist < 0", dict(max_dist=-1.0)),
           ("max_dist NaN", dict(max_dist=NAN)), ("travel < 0", dict(travel=-0.1)), ("travel inf", dict(travel=INF)),
           ("travel NaN", dict(travel=NAN))]
    for what, kw in bad:
        a, o = {**ok, **kw}, host_outputs(R)
        rc = core.lib.mocap_rigid_groups(core._h, a["F"], a["R"], _p(traj), a["n"], a["tol"], a["max_dist"], a["travel"], *[_p(o[k]) for k in OUT])
        assert rc == capi.MOCAP_E_ARG, (what, rc)
        assert all((o[k] == SENTINEL).all() for k in OUT), what
        assert b"mocap_rigid_groups" in core.lib.mocap_last_error(core._h), what
    o = host_outputs(R)
    ptrs = [_p(o[k]) for k in OUT]
    for i in range(len(OUT)):                                                # a null buffer, each in turn
        args = ptrs[:i] + [None] + ptrs[i + 1:]
        assert core.lib.mocap_rigid_groups(core._h, F, R, _p(traj), 30, 0.003, INF, 0.0, *args) == capi.MOCAP_E_ARG, OUT[i]
    assert core.lib.mocap_rigid_groups(core._h, F, R, None, 30, 0.003, INF, 0.0, *ptrs) == capi.MOCAP_E_ARG
    assert all((o[k] == SENTINEL).all() for k in OUT)
    with pytest.raises(capi.MocapError) as e:                                # the device form refuses before anything is enqueued
        core.rigid_groups_dev(F, R, 8, 1, 0.003, INF, 0.0, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8)
    assert e.value.code == capi.MOCAP_E_ARG
    # the edges of what is accepted
    assert_equal(core.rigid_groups(traj, 2, 1e-300, max_dist=1e-300, min_travel=0.0), rg.rigid_groups(traj, 2, 1e-300, 1e-300, 0.0), "edges")
    assert_equal(core.rigid_groups(traj, 30, 1e300, max_dist=INF, min_travel=1e300), rg.rigid_groups(traj, 30, 1e300, INF, 1e300), "edges")


# ---------------------------------------------------------------- 5. a tracked session end to end
def test_tracked_session_to_registered_bodies(core):
    """A 4-marker and a 5-marker body in flights of their own, two loose markers and a static one, 0.5 mm of noise, every marker
    hidden once for longer than the tracker's max_missed: track_markers -> session_trajectories(stitch=...) -> find_rigid_groups ->
    learn_session_bodies -> set_rigid_bodies -> locate_rigid_bodies (tests/test_rigid_groups_reference_cpu.py shows the statement
    alone gets this session right, with its margins)."""
    import torch
    from mocap_core import helpers
    t, xyz, n_pts, slot_of, owner, templates, _ = rg.flight_scene()
    M = len(owner)
    fresh_xyz, fresh_n, shown = rg.fresh_frames(43, templates)
    dev = torch.device("cuda", 0)
    core.set_world_transform(None)
    core.set_marker_tracker(**rg.FLIGHT_TRACKER)
    helpers.set_core(core)
    try:
        mk = core.track_markers(t, xyz, n_pts)
        kw = dict(hits=mk["hits"], degree=2, W=8, n_min=5, max_gap=4, **rg.FLIGHT_TABLE)
        ses = helpers.session_trajectories(t, xyz, n_pts, mk["id"], stitch=rg.FLIGHT_STITCH, **kw)
        res = helpers.session_trajectories(*[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (t, xyz, n_pts, mk["id"])],
                                           stitch=rg.FLIGHT_STITCH, **{**kw, "hits": torch.from_numpy(mk["hits"]).to(dev)})
        groups = helpers.find_rigid_groups(ses, **rg.FLIGHT_GROUPS)
        groups_res = helpers.find_rigid_groups(res, **rg.FLIGHT_GROUPS)
        capture = {"xyz": xyz, "n_pts": n_pts, "id": mk["id"]}
        learned, skipped = helpers.learn_session_bodies(capture, ses, groups, names=["first", "second"])
        resident = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in capture.items()}
        learned_res, skipped_res = helpers.learn_session_bodies(resident, res, groups_res, names=["first", "second"])
        plain = helpers.session_trajectories(t, xyz, n_pts, mk["id"], **kw)               # without stitching: ids are plain ints
        groups_plain = helpers.find_rigid_groups(plain, tol=0.003, min_common=50)
        helpers.set_rigid_bodies(learned, tol=0.005, max_rms=0.005)
        got = core.locate_rigid_bodies(fresh_xyz, fresh_n)
    finally:
        helpers.set_rigid_bodies([])
        core.set_marker_tracker(T_max=0)
    assert len(ses["ids"]) == M and all(len(c) == 2 for c in ses["ids"])                  # every id split once, and was stitched
    marker = [[m for m in range(M) if np.array_equal(np.isfinite(row[:, 0]), slot_of[m] >= 0)][0] for row in ses["traj"]]
    own = owner[marker]
    # exactly two groups made of exactly the planted rows, no conflicts, nothing else in a group
    assert len(groups) == 2 and [g["conflicts"] for g in groups] == [0, 0] and sorted(g["size"] for g in groups) == [4, 5]
    for g in groups:
        b = own[g["rows"][0]]
        assert b >= 0 and g["rows"] == np.flatnonzero(own == b).tolist() and g["max_spread"] <= 0.0015
        assert g["ids"] == [ses["ids"][r].tolist() for r in g["rows"]] and g["dist"].shape == (g["size"], g["size"])
    full = core.rigid_groups(ses["traj"], rg.FLIGHT_GROUPS["min_common"], rg.FLIGHT_GROUPS["tol"])
    assert (full["group_of"][own < 0] == -1).all() and (own < 0).sum() == 3
    assert_equal(full, rg.rigid_groups(ses["traj"], rg.FLIGHT_GROUPS["min_common"], rg.FLIGHT_GROUPS["tol"]), "flight")
    # the unstitched session: fragments of one marker never share a frame, so each body falls into groups of its fragments' overlap
    assert all(isinstance(i, int) for g in groups_plain for i in g["ids"]) and len(groups_plain) >= 2
    # NumPy and resident forms byte for byte
    assert len(groups_res) == 2 and skipped == [] and skipped_res == []
    for a, b in zip(groups, groups_res):
        assert a["rows"] == b["rows"] and a["ids"] == b["ids"] and (a["size"], a["conflicts"]) == (b["size"], b["conflicts"])
        assert a["dist"].tobytes() == b["dist"].tobytes() and np.float64(a["max_spread"]).tobytes() == np.float64(b["max_spread"]).tobytes()
    # two bodies; every learned pair distance within 0.5 mm of the planted one: the standard error of a mean over >= 100 used frames
    # of a distance with 0.71 mm of noise is <= 0.07 mm, the bound is seven of those
    assert len(learned) == len(learned_res) == 2 and [b["name"] for b in learned] == ["first", "second"]
    for body, again in zip(learned, learned_res):
        assert body["status"] == 0 and body["frames_used"] >= 100 and body["sel"] == body["rows"]
        assert np.asarray(body["markers"]).tobytes() == np.asarray(again["markers"]).tobytes()
        b = own[body["rows"][0]]
        q = templates[b][[marker[r] - (0 if b == 0 else rg.FLIGHT_BODIES[0]) for r in body["rows"]]]
        L = np.asarray(body["markers"])
        for i in range(len(q)):
            for j in range(i):
                assert abs(np.linalg.norm(L[i] - L[j]) - np.linalg.norm(q[i] - q[j])) <= 0.0005, (body["name"], i, j)
    # registered: both bodies are found wherever at least three of their markers show
    seen3 = 0
    for k, body in enumerate(learned):
        shows = shown[own[body["rows"][0]]].sum(axis=1)
        for f in range(fresh_xyz.shape[0]):
            if shows[f] >= 3:
                seen3 += 1
                assert got["found"][f, k] == 1 and got["n_used"][f, k] == shows[f], (body["name"], f)
    assert seen3 >= 70                   # (60 frames, a marker shows with probability 0.7: 39 + 50 expected)
