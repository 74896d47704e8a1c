"""Track stitching on the device (include/mocap_core.h, "track stitching"; csrc/track_stitch.hip) against the plain statement of the
contract (tests/track_stitch_reference.py): ext, next, prev, chain, row_of and n_chains exactly, cost bit for bit (any NaN equal to
any NaN), with fragment ends and fit windows around the 256-frame tile edge; the association at its full width and in its worst
case; the host and device forms, call after call, the sentinel, the refusals, and a tracked session end to end."""
import numpy as np
import pytest

import track_smooth_reference as ts
import track_stitch_reference as st

pytestmark = pytest.mark.gpu

INF = float("inf")
OUT = ("ext", "next", "prev", "cost", "chain", "row_of", "n_chains")
SENTINEL = -7
# (last frame before the cut, hidden frames): ends on 255, 256, 257, beginnings on 255, 256, 257 (b + L + 1), and a few elsewhere
FIRST_CUTS = [(255, 3), (256, 9), (257, 2), (250, 4), (250, 5), (250, 6), (254, 1), (252, 3), (120, 5), (200, 30), (150, 12), (230, 8)]
SECOND_CUTS = [(20, 3), (50, 10), (80, 2), (35, 6), (60, 1)]     # all before frame 100: ends whose fit window runs off frame 0
GATES = dict(max_dt=0.4, gate=0.4, gate_rate=2.0)


def session(seed, F, R, bad_stamps=False):
    """R rows over F frames.  F >= 255: ceil(R / 3) noisy markers with dropouts, cut into R fragments at FIRST_CUTS and SECOND_CUTS
    (whichever fit into F), the rows shuffled; every marker runs to frame F - 1, so a head window near the end runs off it.  With
    three or more rows the last is all NaN.  bad_stamps: a NaN, an equal and a decreasing stamp beside the planted ends."""
    rng = np.random.default_rng(seed)
    if F <= 2:
        t = 3.0 + np.arange(F) / 120.0
        rows = np.full((R, F, 3), np.nan)
        for r in range(R):
            rows[r, r % F] = 0.01 * rng.standard_normal(3)          # F = 2: rows alternate between the frames, and may link
        if R >= 3:
            rows[R - 1] = np.nan
        return t, rows
    M = (R + 2) // 3
    t, _, traj = ts.make_session(seed, F, M, dropout=0.04, max_run=3)
    first = [c for c in FIRST_CUTS if c[0] + 1 + c[1] < F]
    cuts = [(m, first[m % len(first)][0] + 1, first[m % len(first)][1]) for m in range(min(M, R - M) if first else 0)]
    cuts += [(m, SECOND_CUTS[m % 5][0] + 1, SECOND_CUTS[m % 5][1]) for m in range(R - M - len(cuts))]
    rows, _ = st.cut_session(traj, cuts, seed=seed)
    assert rows.shape[0] == R
    if bad_stamps:
        for f, g in ((253, None), (259, 258), (45, 43), (22, None), (F - 3, F - 5)):
            if 0 < f < F:
                t[f] = np.nan if g is None else t[g]
    if R >= 3:
        rows[R - 1] = np.nan
    return t, rows


def dev_stitch(core, t, traj, fit_frames, max_dt, gate, gate_rate):
    """mocap_stitch_tracks_dev into outputs pre-filled with the sentinel -> host arrays."""
    import torch
    dev = torch.device("cuda", 0)
    R, F, _ = traj.shape
    d_t, d_traj = torch.from_numpy(np.ascontiguousarray(t)).to(dev), torch.from_numpy(np.ascontiguousarray(traj)).to(dev)
    o = {k: torch.full((R,), SENTINEL, dtype=torch.int32, device=dev) for k in ("next", "prev", "chain", "row_of")}
    o["ext"] = torch.full((R, 3), SENTINEL, dtype=torch.int32, device=dev)
    o["cost"] = torch.full((R,), float(SENTINEL), dtype=torch.float64, device=dev)
    o["n_chains"] = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    core.stitch_tracks_dev(F, R, d_t.data_ptr(), d_traj.data_ptr(), fit_frames, max_dt, gate, gate_rate, *[o[k].data_ptr() for k in OUT])
    core.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["n_chains"] = int(got["n_chains"][0])
    return got


def assert_equal(got, ref, what):
    for k in st.INT_OUT:
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5].tolist())
    assert got["n_chains"] == ref["n_chains"], what
    assert ts.same_bits(got["cost"], ref["cost"]), (what, "cost")


# ---------------------------------------------------------------- 1. the device against the statement, around the tile edge
@pytest.mark.parametrize("fit", [1, 8, 64])
@pytest.mark.parametrize("R", [1, 2, 3, 64])
@pytest.mark.parametrize("F", [1, 2, 255, 256, 257, 600])
def test_stitch_equals_the_statement(core, F, R, fit):
    t, traj = session(F + R + fit, F, R, bad_stamps=(F + R + fit) % 2 == 1)
    ref = st.stitch(t, traj, fit, **GATES)
    assert_equal(dev_stitch(core, t, traj, fit, **GATES), ref, (F, R, fit))
    if F >= 255 and R == 64:                        # more admissible pairs than links: some rows compete for a partner
        assert (ref["next"] >= 0).sum() >= 30 and np.isfinite(ref["table"]).sum() > (ref["next"] >= 0).sum(), (F, R, fit)
    if F == 600 and R == 64:                        # ends and beginnings on either side of the tile edge, and an empty row
        assert {255, 256, 257} <= set(ref["ext"][:, 1].tolist()) and {255, 256, 257} <= set(ref["ext"][:, 0].tolist())
        assert ref["ext"][R - 1].tolist() == [-1, -1, 0] and ref["row_of"][R - 1] == -1


@pytest.mark.parametrize("fit", [1, 8, 64])
def test_bad_stamps_inside_the_fit_windows(core, fit):
    t, traj = session(40 + fit, 600, 64, bad_stamps=True)
    ref = st.stitch(t, traj, fit, INF, 0.2, 0.5)
    assert not ts.good_times(t).all() and (ref["next"] >= 0).sum() >= 10
    assert_equal(dev_stitch(core, t, traj, fit, INF, 0.2, 0.5), ref, fit)


def test_overflowing_time_differences(core):
    """h = inf, u = NaN, det = NaN: the end model falls back to the end sample."""
    t = np.array([-1.5e308, 1.5e308, 1.6e308])
    traj = np.full((2, 3, 3), np.nan)
    traj[0, :2] = [[1, 1, 1], [2, 1, 1]]
    traj[1, 2] = [2, 1, 1]
    ref = st.stitch(t, traj, 4, INF, 1.0, 0.0)
    assert ref["next"].tolist() == [1, -1]
    assert_equal(dev_stitch(core, t, traj, 4, INF, 1.0, 0.0), ref, "overflow")


# ---------------------------------------------------------------- 2. the association: full width, worst case
def test_the_full_width_of_the_association(core):
    """R = 1024, F = 64: 256 markers on a 16 x 16 grid 0.1 m apart, four fragments each, 3 cm of noise and a gate wide enough for every
    tail to see the heads of a dozen neighbours: many rows want the same partner, and the rounds go on."""
    rng = np.random.default_rng(11)
    F, R = 64, 1024
    t = 1.0 + np.cumsum((1.0 + 0.2 * rng.uniform(-1.0, 1.0, F)) / 120.0)
    home = np.array([[0.1 * (m % 16), 0.1 * (m // 16), 1.0] for m in range(256)])
    vel = 0.5 * rng.uniform(-1.0, 1.0, (256, 3))
    traj = np.full((R, F, 3), np.nan)
    for r, m in enumerate(rng.permutation(R)):
        m, k = m % 256, m // 256
        lo, hi = 16 * k + int(rng.integers(0, 4)), 16 * k + int(rng.integers(10, 15))
        traj[r, lo:hi] = home[m] + vel[m] * (t[lo:hi, None] - t[0]) + 0.03 * rng.standard_normal((hi - lo, 3))
    ref = st.stitch(t, traj, 8, INF, 0.3, 0.0)
    rounds = st.associate_rounds(ref["table"])[3]
    admissible = int(np.isfinite(ref["table"]).sum())
    print(f"admissible pairs {admissible}, links {int((ref['next'] >= 0).sum())}, chains {ref['n_chains']}, rounds {rounds}")
    assert admissible > 10 * R and rounds >= 3 and (ref["next"] >= 0).sum() > R // 2
    assert_equal(dev_stitch(core, t, traj, 8, INF, 0.3, 0.0), ref, "R 1024")


def test_the_ladder_one_commit_per_round(core):
    t, traj = st.ladder(64)
    ref = st.stitch(t, traj, **st.LADDER)
    assert st.associate_rounds(ref["table"])[3] == 63 and st.chains_of(ref) == [list(range(64))]
    assert_equal(dev_stitch(core, t, traj, **st.LADDER), ref, "ladder")


# ---------------------------------------------------------------- 3. host form, repeated calls, sentinel
def test_host_and_device_forms_and_repeated_calls_give_the_same_bytes(core):
    t, traj = session(5, 600, 64, bad_stamps=True)
    host = core.stitch_tracks(t, traj, fit_frames=8, **GATES)
    one = dev_stitch(core, t, traj, 8, **GATES)
    two = dev_stitch(core, t, traj, 8, **GATES)
    for k in OUT[:-1]:
        assert host[k].tobytes() == one[k].tobytes() == two[k].tobytes(), k
        assert host[k].dtype == one[k].dtype and host[k].shape == one[k].shape
    assert host["n_chains"] == one["n_chains"] == two["n_chains"]
    assert_equal(host, st.stitch(t, traj, 8, **GATES), "host")


def test_outputs_prefilled_with_a_sentinel_are_fully_overwritten(core):
    t, traj = session(6, 257, 3)
    got = dev_stitch(core, t, traj, 8, **GATES)
    for k in st.INT_OUT:
        assert not (got[k] == SENTINEL).any(), k
    assert not (got["cost"] == SENTINEL).any() and got["n_chains"] != SENTINEL
    assert got["ext"][2].tolist() == [-1, -1, 0]                   # the empty row: every one of its outputs is written too
    assert (got["next"][2], got["prev"][2], got["chain"][2], got["row_of"][2]) == (-1, -1, 2, -1) and np.isnan(got["cost"][2])


# ---------------------------------------------------------------- 4. refusals
def test_every_refusal_leaves_its_outputs_untouched(core):
    from mocap_core import capi
    from mocap_core.capi import _p
    F, R = 120, 2
    t, traj = session(3, F, R)

    def outputs():
        o = {k: np.full(R, SENTINEL, dtype=np.int32) for k in ("next", "prev", "chain", "row_of")}
        o.update(ext=np.full((R, 3), SENTINEL, dtype=np.int32), cost=np.full(R, float(SENTINEL)), n_chains=np.full(1, SENTINEL, dtype=np.int32))
        return o

    ok = dict(F=F, R=R, fit=4, max_dt=INF, gate=0.05, rate=0.5)
    nan = float("nan")
    bad = [("F 0", dict(F=0)), ("R 0", dict(R=0)), ("R 1025", dict(R=1025)), ("fit 0", dict(fit=0)), ("fit 65", dict(fit=65)),
           ("max_dt 0", dict(max_dt=0.0)), ("max_dt < 0", dict(max_dt=-1.0)), ("max_dt NaN", dict(max_dt=nan)), ("gate 0", dict(gate=0.0)),
           ("gate < 0", dict(gate=-0.1)), ("gate inf", dict(gate=INF)), ("gate NaN", dict(gate=nan)), ("rate < 0", dict(rate=-0.5)),
           ("rate inf", dict(rate=INF)), ("rate NaN", dict(rate=nan)), ("R F > 2^31", dict(F=(1 << 31) // 2 + 1))]
    for what, kw in bad:
        a, o = {**ok, **kw}, outputs()
        rc = core.lib.mocap_stitch_tracks(core._h, a["F"], a["R"], _p(t), _p(traj), a["fit"], a["max_dt"], a["gate"], a["rate"],
                                          *[_p(o[k]) for k in OUT])
        assert rc == capi.MOCAP_E_ARG, (what, rc)
        assert all((o[k] == SENTINEL).all() for k in OUT), what
        assert b"mocap_stitch_tracks" in core.lib.mocap_last_error(core._h), what
    # a null buffer, each in turn, and the host form's own rule: a t with no finite entry
    o = outputs()
    ptrs = [_p(o[k]) for k in OUT]
    for i in range(len(OUT)):
        args = ptrs[:i] + [None] + ptrs[i + 1:]
        assert core.lib.mocap_stitch_tracks(core._h, F, R, _p(t), _p(traj), 4, INF, 0.05, 0.5, *args) == capi.MOCAP_E_ARG, OUT[i]
    assert core.lib.mocap_stitch_tracks(core._h, F, R, None, _p(traj), 4, INF, 0.05, 0.5, *ptrs) == capi.MOCAP_E_ARG
    assert core.lib.mocap_stitch_tracks(core._h, F, R, _p(t), None, 4, INF, 0.05, 0.5, *ptrs) == capi.MOCAP_E_ARG
    nowhere = np.full(F, np.nan)
    nowhere[3] = -INF
    assert core.lib.mocap_stitch_tracks(core._h, F, R, _p(nowhere), _p(traj), 4, INF, 0.05, 0.5, *ptrs) == capi.MOCAP_E_ARG
    assert all((o[k] == SENTINEL).all() for k in OUT)
    # the device form refuses the same way, before anything is enqueued; and it takes a t with no finite entry: every row is empty
    with pytest.raises(capi.MocapError) as e:
        core.stitch_tracks_dev(F, R, 8, 8, 65, INF, 0.05, 0.5, 8, 8, 8, 8, 8, 8, 8)
    assert e.value.code == capi.MOCAP_E_ARG
    got = dev_stitch(core, nowhere, traj, 4, INF, 0.05, 0.5)
    assert got["n_chains"] == 0 and (got["row_of"] == -1).all() and (got["ext"] == [-1, -1, 0]).all() and np.isnan(got["cost"]).all()
    assert_equal(got, st.stitch(nowhere, traj, 4, INF, 0.05, 0.5), "no finite t")
    # the edges of what is accepted
    assert_equal(core.stitch_tracks(t, traj, fit_frames=64, max_dt=1e-300, gate=1e-300, gate_rate=0.0),
                 st.stitch(t, traj, 64, 1e-300, 1e-300, 0.0), "edges")


# ---------------------------------------------------------------- 5. a tracked session end to end
def test_tracked_session_is_stitched_into_one_row_per_marker(core):
    """Four markers in free flight, 0.5 mm of noise, each hidden once or twice for 10 .. 25 frames -- longer than the tracker's
    max_missed = 6, so its id splits: track_markers -> session_trajectories(stitch=...) gives four rows, each made of exactly the ids
    its marker went through (tests/test_track_stitch_reference_cpu.py shows the statement alone gets this session right)."""
    import torch
    from mocap_core import helpers
    t, xyz, n_pts, slot_of, hidden = st.flight_session()
    F, M = t.size, 4
    core.set_world_transform(None)
    core.set_marker_tracker(**st.FLIGHT_TRACKER)
    helpers.set_core(core)
    try:
        mk = core.track_markers(t, xyz, n_pts)
        kw = dict(hits=mk["hits"], degree=2, W=8, n_min=5, max_gap=4, **st.FLIGHT_TABLE)
        plain = helpers.session_trajectories(t, xyz, n_pts, mk["id"], **kw)
        none = helpers.session_trajectories(t, xyz, n_pts, mk["id"], stitch=None, **kw)
        out = helpers.session_trajectories(t, xyz, n_pts, mk["id"], stitch=st.FLIGHT_STITCH, **kw)
        dev = torch.device("cuda", 0)
        res = helpers.session_trajectories(*[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (t, xyz, n_pts, mk["id"])],
                                           stitch=st.FLIGHT_STITCH, **{**kw, "hits": torch.from_numpy(mk["hits"]).to(dev)})
    finally:
        core.set_marker_tracker(T_max=0)
    truth = st.flight_truth(mk["id"], slot_of)
    assert sum(len(c) for c in truth) == M + len(hidden)                                 # the ids really split
    # without stitching: today's function, one row per id
    assert sorted(plain) == sorted(none) and all(np.asarray(plain[k]).tobytes() == np.asarray(none[k]).tobytes() for k in plain)
    assert plain["ids"].size == M + len(hidden) and "links" not in plain
    want = helpers.track_table(mk["id"], mk["hits"], **st.FLIGHT_TABLE)
    assert np.array_equal(plain["relabel"], want[0]) and np.array_equal(plain["ids"], want[1])
    assert ts.same_bits(plain["traj"], ts.gather(xyz, n_pts, mk["id"], want[0], want[1].size, mk["hits"], 1))
    # with it
    assert len(out["ids"]) == 4 and out["pos"].shape == (M, F, 3)
    assert sorted(c.tolist() for c in out["ids"]) == sorted(truth)
    assert len(out["links"]) == len(hidden) and out["fragments"].shape == (M + len(hidden), 3)
    for a, b, cost, dt in out["links"]:
        assert any(a in c and c[c.index(a) + 1:c.index(a) + 2] == [b] for c in truth) and cost < 0.5 * 0.03 ** 2 * 4 and 9 / 120 < dt < 0.3
    for r, chain in enumerate(out["ids"]):
        m = [i for i, c in enumerate(truth) if c == chain.tolist()][0]
        assert np.array_equal(np.isfinite(out["traj"][r, :, 0]), slot_of[m] >= 0)          # the marker's every sighting, nothing else
        assert (out["relabel"][chain] == r).all()
    # the resident form: the same bytes
    for k in ("traj", "pos", "vel", "acc", "res", "n_used", "flag"):
        assert res[k].is_cuda and res[k].cpu().numpy().tobytes() == out[k].tobytes(), k
    assert [c.tolist() for c in res["ids"]] == [c.tolist() for c in out["ids"]] and res["links"] == out["links"]
    assert np.array_equal(res["fragments"], out["fragments"]) and np.array_equal(res["relabel"], out["relabel"])
