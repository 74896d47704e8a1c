"""Trajectories on the device (include/mocap_core.h, "trajectories"; csrc/track_smooth.hip) against the plain statement of the
contract (tests/track_smooth_reference.py): flag, n_used and traj exactly, pos, vel, acc and res bit for bit (any NaN equal to any
NaN), at the frame counts around the 256-frame tile and its halo; the host and device forms, call after call, the sentinel, the
refusals, and a tracked session end to end."""
import numpy as np
import pytest

import track_smooth_reference as ts

pytestmark = pytest.mark.gpu

INF = float("inf")
TILE = 256
OUT = ("pos", "vel", "acc", "res", "n_used", "flag")
SENTINEL = -7.0


def session(seed, F, R, max_gap, bad_halo_W=0):
    """A noisy irregular session with random dropouts, and planted around every tile edge E = 256, 512, ... < F: in row 0 and row 1 a
    gap of exactly max_gap frames and one of max_gap + 1 that contain frame E - 1 (and E, from two frames on), alternating between
    the rows from edge to edge; a dropout-free stretch around them so that the gaps are what they are meant to be.  With three or
    more rows the last is all NaN.  bad_halo_W = W: an equal time stamp in the lower halo of every edge's tile and a NaN one in the
    upper halo of the tile before it."""
    t, truth, traj = ts.make_session(seed, F, R, dropout=0.06, max_run=max(max_gap + 2, 3))
    rng = np.random.default_rng(seed + 1000)
    for E in range(TILE, F, TILE):
        for r in range(min(R, 2)):
            lo, hi = max(E - 40, 0), min(E + 40, F)
            gone = np.isnan(traj[r, lo:hi, 0])
            traj[r, lo:hi][gone] = truth[r, lo:hi][gone] + 5e-4 * rng.standard_normal((int(gone.sum()), 3))
            g = max_gap + (r + E // TILE) % 2
            if g:
                start = E - (g + 1) // 2
                traj[r, start:min(start + g, F)] = np.nan
        if bad_halo_W:
            if E + bad_halo_W - 1 < F:
                t[E + bad_halo_W - 1] = np.nan          # the last frame of the upper halo of the tile below the edge
            if E - bad_halo_W - 1 >= 0:
                t[E - bad_halo_W] = t[E - bad_halo_W - 1]   # the first frame of the lower halo of the tile above it
    if R >= 3:
        traj[R - 1] = np.nan
    return t, traj


def dev_smooth(core, t, traj, d, W, span, n_min, max_gap):
    """mocap_smooth_tracks_dev into outputs pre-filled with the sentinel -> host arrays."""
    import torch
    dev = torch.device("cuda", 0)
    R, F, _ = traj.shape
    d_t, d_traj = torch.from_numpy(np.ascontiguousarray(t)).to(dev), torch.from_numpy(np.ascontiguousarray(traj)).to(dev)
    o = {k: torch.full((R, F, 3), SENTINEL, dtype=torch.float64, device=dev) for k in ("pos", "vel", "acc")}
    o["res"] = torch.full((R, F), SENTINEL, dtype=torch.float64, device=dev)
    o["n_used"], o["flag"] = (torch.full((R, F), int(SENTINEL), dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    core.smooth_tracks_dev(F, R, d_t.data_ptr(), d_traj.data_ptr(), d, W, span, n_min, max_gap, *[o[k].data_ptr() for k in OUT])
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def assert_equal(got, ref, what):
    for k in ("flag", "n_used"):
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5])
    for k in ts.FIELDS:
        assert ts.same_bits(got[k], ref[k]), (what, k)


def params(F, W, i):
    d = min(1 + i % 3, 2 * W)                       # n_min <= 2 W + 1 leaves W = 1 the degrees 1 and 2
    return d, min(d + 1 + i % 2, 2 * W + 1), W if i % 2 else max(W // 2, 1)


# ---------------------------------------------------------------- 1. the device against the statement, around the tile and its halo
@pytest.mark.parametrize("W", [1, 8, 32])
@pytest.mark.parametrize("F", [1, 2, 255, 256, 257, "256+W", 3 * 256 + 5])
def test_smooth_equals_the_statement_bit_for_bit(core, F, W):
    F = 256 + W if F == "256+W" else F
    i = F + W
    R = (3, 64)[i % 2] if F > TILE else (1, 3, 64)[i % 3]
    d, n_min, max_gap = params(F, W, i)
    span = INF if i % 3 else 1.3 * W / 120.0
    t, traj = session(i, F, R, max_gap)
    ref = ts.smooth(t, traj, d, W, span, n_min, max_gap)
    got = dev_smooth(core, t, traj, d, W, span, n_min, max_gap)
    assert_equal(got, ref, (F, W, R, d))
    if F > 2 * TILE:                                # the planted gaps straddle the first edge: max_gap + 1 frames in row 0, max_gap in row 1
        assert ref["flag"][0, TILE - 1] == 0 and ref["flag"][1, TILE - 1] in (ts.FILLED, ts.FEW), ref["flag"][:2, TILE - 1]


@pytest.mark.parametrize("W", [1, 8, 32])
@pytest.mark.parametrize("F", [257, "256+W", 3 * 256 + 5])
def test_bad_time_stamps_in_the_halo(core, F, W):
    F = 256 + W if F == "256+W" else F
    d, n_min, max_gap = params(F, W, F + W + 1)
    t, traj = session(F + 7 * W, F, 3, max_gap, bad_halo_W=W)
    ref = ts.smooth(t, traj, d, W, INF, n_min, max_gap)
    assert (ref["flag"] == ts.BAD_TIME).any()
    assert_equal(dev_smooth(core, t, traj, d, W, INF, n_min, max_gap), ref, (F, W))


@pytest.mark.parametrize("R", [1, 3, 64])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_every_degree_and_row_count(core, d, R):
    F, W = 3 * 256 + 5, 8
    t, traj = session(10 * d + R, F, R, 5)
    ref = ts.smooth(t, traj, d, W, 0.09, d + 2, 5)
    got = dev_smooth(core, t, traj, d, W, 0.09, d + 2, 5)
    assert_equal(got, ref, (d, R))
    assert {ts.SMOOTHED, ts.FILLED, 0} <= set(np.unique(ref["flag"]).tolist())
    assert np.isnan(got["acc"]).all() == (d == 1)
    if R >= 3:
        assert (got["flag"][R - 1] == 0).all() and (got["n_used"][R - 1] == 0).all() and np.isnan(got["pos"][R - 1]).all()


def test_singular_and_overflowing_windows(core):
    """Time stamps whose differences overflow: h = inf, u = NaN, the first pivot past S_0 fails."""
    t = np.array([-1.5e308, -1.0e308, 1.0e308, 1.5e308, 1.6e308])
    traj = np.ones((1, 5, 3))
    ref = ts.smooth(t, traj, 1, 2, INF, 2, 0)
    assert (ref["flag"] == ts.SINGULAR).any()
    assert_equal(dev_smooth(core, t, traj, 1, 2, INF, 2, 0), ref, "overflow")


# ---------------------------------------------------------------- 2. host form, repeated calls, sentinel
def test_host_and_device_forms_and_repeated_calls_give_the_same_bytes(core):
    F, R, W, d = 3 * 256 + 5, 3, 8, 2
    t, traj = session(5, F, R, 4, bad_halo_W=W)
    host = core.smooth_tracks(t, traj, degree=d, W=W, span=0.08, n_min=4, max_gap=4)
    one = dev_smooth(core, t, traj, d, W, 0.08, 4, 4)
    two = dev_smooth(core, t, traj, d, W, 0.08, 4, 4)
    for k in OUT:
        assert host[k].tobytes() == one[k].tobytes() == two[k].tobytes(), k
        assert host[k].dtype == one[k].dtype and host[k].shape == one[k].shape
    assert_equal(host, ts.smooth(t, traj, d, W, 0.08, 4, 4), "host")


def test_outputs_prefilled_with_a_sentinel_are_fully_overwritten(core):
    t, traj = session(6, 257, 3, 2)
    got = dev_smooth(core, t, traj, 1, 2, INF, 2, 2)
    for k in OUT:
        assert not (got[k] == SENTINEL).any(), k
    import torch
    dev = torch.device("cuda", 0)
    xyz, n_pts, ids, hits, relabel = cloud(9, 257, 5, 4)
    d = [torch.from_numpy(a).to(dev) for a in (xyz, n_pts, ids, hits, relabel)]
    d_traj = torch.full((4, 257, 3), SENTINEL, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    core.gather_tracks_dev(257, 5, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 2, relabel.size, d[4].data_ptr(),
                           4, d_traj.data_ptr())
    core.synchronize()
    got = d_traj.cpu().numpy()
    assert not (got == SENTINEL).any() and ts.same_bits(got, ts.gather(xyz, n_pts, ids, relabel, 4, hits, 2))


# ---------------------------------------------------------------- 3. gather
def cloud(seed, F, K, R):
    """Frame-major points with shuffled slots: ids 0 .. R + 2, two of them sharing row 0, one without a row, some ids beyond the
    table, non-finite points, counts outside 0 .. K, low hits."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-2.0, 2.0, (F, K, 3))
    ids = rng.integers(-1, R + 5, (F, K)).astype(np.int32)
    hits = rng.integers(0, 6, (F, K)).astype(np.int32)
    n_pts = rng.integers(0, K + 1, F).astype(np.int32)
    n_pts[rng.uniform(size=F) < 0.05] = K + 1
    n_pts[rng.uniform(size=F) < 0.05] = -1
    n_pts[F // 2] = K
    xyz[rng.uniform(size=(F, K)) < 0.05] = [1.0, np.nan, 1.0]
    xyz[rng.uniform(size=(F, K)) < 0.03] = [np.inf, 0.0, 0.0]
    relabel = np.concatenate([np.arange(R), [0, -1, R]]).astype(np.int32)      # id R shares row 0; R + 1 has none; R + 2 -> row R: out of range
    return xyz, n_pts, ids, hits, relabel


@pytest.mark.parametrize("F,K,R", [(1, 1, 1), (2, 3, 3), (255, 16, 3), (256, 64, 64), (257, 5, 1), (3 * 256 + 5, 16, 64)])
def test_gather_equals_the_statement(core, F, K, R):
    xyz, n_pts, ids, hits, relabel = cloud(F + K, F, K, R)
    for h, m in ((None, 0), (hits, 3)):
        want = ts.gather(xyz, n_pts, ids, relabel, R, h, m)
        got = core.gather_tracks(xyz, n_pts, ids, relabel, R, hits=h, min_hits=m)
        assert got.shape == (R, F, 3) and ts.same_bits(got, want), (F, K, R, m)
    assert np.isfinite(want).any() or F < 3


# ---------------------------------------------------------------- 4. refusals
def test_every_refusal_leaves_its_outputs_untouched(core):
    from mocap_core import capi
    from mocap_core.capi import _p
    F, R = 20, 2
    t, traj = session(3, F, R, 2)
    ok = dict(F=F, R=R, d=2, W=4, span=INF, n_min=3, max_gap=2)
    bad = [("F 0", dict(F=0)), ("R 0", dict(R=0)), ("R 1025", dict(R=1025)), ("d 0", dict(d=0)), ("d 4", dict(d=4)), ("W 0", dict(W=0)),
           ("W 33", dict(W=33)), ("span 0", dict(span=0.0)), ("span < 0", dict(span=-1.0)), ("span NaN", dict(span=float("nan"))),
           ("n_min d", dict(n_min=2)), ("n_min 2W+2", dict(n_min=10)), ("max_gap -1", dict(max_gap=-1)), ("max_gap W+1", dict(max_gap=5)),
           ("R F > 2^31", dict(F=(1 << 31) // 2 + 1))]
    for what, kw in bad:
        a = {**ok, **kw}
        o = {k: np.full((R, F, 3) if k in ("pos", "vel", "acc") else (R, F), SENTINEL, dtype=np.int32 if k in ("n_used", "flag") else np.float64)
             for k in OUT}
        rc = core.lib.mocap_smooth_tracks(core._h, a["F"], a["R"], _p(t), _p(traj), a["d"], a["W"], a["span"], a["n_min"], a["max_gap"],
                                          *[_p(o[k]) for k in OUT])
        assert rc == capi.MOCAP_E_ARG, (what, rc)
        assert all((o[k] == SENTINEL).all() for k in OUT), what
        assert b"mocap_smooth_tracks" in core.lib.mocap_last_error(core._h), what
    # a null buffer, and the host form's own rule: a t with no finite entry
    o = {k: np.full((R, F, 3) if k in ("pos", "vel", "acc") else (R, F), SENTINEL, dtype=np.int32 if k in ("n_used", "flag") else np.float64)
         for k in OUT}
    ptrs = [_p(o[k]) for k in OUT]
    assert core.lib.mocap_smooth_tracks(core._h, F, R, _p(t), _p(traj), 2, 4, INF, 3, 2, *ptrs[:3], None, *ptrs[4:]) == capi.MOCAP_E_ARG
    nowhere = np.full(F, np.nan)
    nowhere[3] = -INF
    assert core.lib.mocap_smooth_tracks(core._h, F, R, _p(nowhere), _p(traj), 2, 4, INF, 3, 2, *ptrs) == capi.MOCAP_E_ARG
    assert all((o[k] == SENTINEL).all() for k in OUT)
    # the device form refuses the same way, before anything is enqueued; and it takes a t with no finite entry: all BAD_TIME
    import torch
    with pytest.raises(capi.MocapError) as e:
        core.smooth_tracks_dev(F, R, 8, 8, 2, 33, INF, 3, 2, 8, 8, 8, 8, 8, 8)
    assert e.value.code == capi.MOCAP_E_ARG
    got = dev_smooth(core, nowhere, traj, 2, 4, INF, 3, 2)
    assert (got["flag"] == ts.BAD_TIME).all() and (got["n_used"] == 0).all() and np.isnan(got["pos"]).all() and np.isnan(got["res"]).all()
    # the edges of what is accepted
    assert_equal(core.smooth_tracks(t, traj, degree=3, W=32, span=1e-300, n_min=65, max_gap=32), ts.smooth(t, traj, 3, 32, 1e-300, 65, 32), "edges")

    xyz, n_pts, ids, hits, relabel = cloud(4, F, 6, R)
    gok = dict(F=F, K=6, n_ids=relabel.size, R=R)
    for what, kw in [("F 0", dict(F=0)), ("K 0", dict(K=0)), ("K 65", dict(K=65)), ("R 0", dict(R=0)), ("R 1025", dict(R=1025)),
                     ("n_ids 0", dict(n_ids=0)), ("R F > 2^31", dict(F=(1 << 30) + 1))]:
        a = {**gok, **kw}
        out = np.full((R, F, 3), SENTINEL)
        rc = core.lib.mocap_gather_tracks(core._h, a["F"], a["K"], _p(xyz), _p(n_pts), _p(ids), _p(hits), 0, a["n_ids"], _p(relabel),
                                          a["R"], _p(out))
        assert rc == capi.MOCAP_E_ARG and (out == SENTINEL).all(), (what, rc)
        assert b"mocap_gather_tracks" in core.lib.mocap_last_error(core._h), what
    out = np.full((R, F, 3), SENTINEL)
    assert core.lib.mocap_gather_tracks(core._h, F, 6, _p(xyz), _p(n_pts), _p(ids), None, 0, relabel.size, None, R, _p(out)) == capi.MOCAP_E_ARG
    assert (out == SENTINEL).all()
    with pytest.raises(capi.MocapError):
        core.gather_tracks_dev(F, 65, 8, 8, 8, 0, 0, 4, 8, R, 8)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. a tracked session end to end
def test_tracked_session_to_trajectories(core):
    """Four markers in free flight (constant acceleration: a degree-2 window has no model error), 0.5 mm of planted noise, shuffled
    slots, dropouts of up to 4 frames: track_markers -> session_trajectories.  With n_min = 9 samples of a 17-frame window and a
    sample on either side of every filled frame, a fitted coordinate is a combination of the window's noises whose weights have a
    sum of squares (the leverage) below 1: its error is Gaussian with a deviation below the planted sigma, and 5 sigma holds for
    every one of a few thousand values."""
    import torch
    from mocap_core import helpers
    sigma, F, M, K = 0.0005, 400, 4, 8
    rng = np.random.default_rng(77)
    t = 1.0 + np.cumsum((1.0 + 0.2 * rng.uniform(-1.0, 1.0, F)) / 120.0)
    tau = (t - t[0])[None, :, None]
    p0 = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.2], [0.0, 1.0, 0.8], [1.0, 1.0, 1.5]])[:, None, :]
    v0 = np.array([0.4, -0.3, 0.5]) + 0.1 * rng.uniform(-1.0, 1.0, (M, 1, 3))
    a0 = np.array([0.3, 0.5, -1.0]) + 0.1 * rng.uniform(-1.0, 1.0, (M, 1, 3))
    truth = p0 + v0 * tau + 0.5 * a0 * tau * tau                                  # [M][F][3]
    seen = np.ones((M, F), dtype=bool)
    for m in range(M):
        for f in rng.choice(np.arange(20, F - 20, 12), 12, replace=False):
            seen[m, f:f + int(rng.integers(1, 5))] = False
    xyz = np.full((F, K, 3), np.nan)
    n_pts = np.zeros(F, dtype=np.int32)
    slot_of = np.full((M, F), -1)
    for f in range(F):
        order = rng.permutation(np.nonzero(seen[:, f])[0])
        n_pts[f] = order.size
        for j, m in enumerate(order):
            xyz[f, j] = truth[m, f] + sigma * rng.standard_normal(3)
            slot_of[m, f] = j
    core.set_world_transform(None)
    core.set_marker_tracker(gate=0.05, max_missed=6, vel_alpha=0.5, T_max=16)
    helpers.set_core(core)
    try:
        mk = core.track_markers(t, xyz, n_pts)
        kw = dict(hits=mk["hits"], min_hits=1, min_len=50, degree=2, W=8, n_min=9, max_gap=4)
        out = helpers.session_trajectories(t, xyz, n_pts, mk["id"], **kw)
        dev = torch.device("cuda", 0)
        res = helpers.session_trajectories(*[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (t, xyz, n_pts, mk["id"])],
                                           **{**kw, "hits": torch.from_numpy(mk["hits"]).to(dev)})
    finally:
        core.set_marker_tracker(T_max=0)
    assert out["ids"].tolist() == [0, 1, 2, 3] and out["pos"].shape == (M, F, 3)
    for k in ("traj",) + OUT:
        assert res[k].is_cuda and res[k].cpu().numpy().tobytes() == out[k].tobytes(), k
    filled = 0
    for r in range(M):
        m = int(np.argmin(np.linalg.norm(truth[:, 0] - out["traj"][r, 0], axis=1)))      # every marker is seen in frame 0
        assert np.array_equal(np.isfinite(out["traj"][r, :, 0]), seen[m])                # one id per marker through every dropout
        fit = np.isin(out["flag"][r], (ts.SMOOTHED, ts.FILLED))
        assert (out["flag"][r][~seen[m]] == ts.FILLED).all() and fit.all()
        filled += int((~seen[m]).sum())
        err = np.abs(out["pos"][r] - truth[m])
        print(f"row {r}: marker {m}, {int((~seen[m]).sum())} filled, worst error filled {err[~seen[m]].max():.2e} m, "
              f"smoothed {err[seen[m]].max():.2e} m (sigma {sigma:.1e})")
        assert err[~seen[m]].max() <= 5.0 * sigma
        assert err[seen[m]].max() <= 5.0 * sigma
    assert filled >= 60
