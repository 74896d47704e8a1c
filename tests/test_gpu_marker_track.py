"""GPU: the marker tracker (include/mocap_core.h "marker tracker", csrc/marker_track.hip) against its plain NumPy statement
(tests/marker_track_reference.py).  No tolerance anywhere: every decision is a comparison of doubles that come out of one pinned
expression, so ids, hits, counts and status are compared exactly and the state's positions, velocities and times bit for bit."""
import numpy as np
import pytest

import marker_track_reference as mt

pytestmark = pytest.mark.gpu

OUT_KEYS = ("id", "hits", "n_tracks", "mk_status")
STATE_KEYS = ("id", "pos", "vel", "t_seen", "missed", "hits")
PLANTED = {"m20_k32": (20, 32, 3, 1), "m40_k64": (40, 64, 3, 11), "m5_k8": (5, 8, 1, 12)}   # markers, K_max, clutter, seed


@pytest.fixture(scope="module")
def scenes():
    """Each planted scene once, with the reference's outputs and final state under the issue's parameters."""
    out = {}
    for name, (markers, K_max, clutter, seed) in PLANTED.items():
        t, xyz, n_pts, truth = mt.planted_scene(markers, K_max, clutter, seed)
        ref = mt.Tracker(**mt.DEFAULTS)
        out[name] = dict(t=t, xyz=xyz, n_pts=n_pts, truth=truth, want=ref.run(t, xyz, n_pts), state=ref.tracks())
    return out


@pytest.fixture()
def mcore(core):
    core.set_world_transform(None)
    yield core
    core.set_marker_tracker(T_max=0)


def same_outputs(got, want, where=""):
    for k in OUT_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (where, k)


def same_state(got, want, where=""):
    for k in STATE_KEYS:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (where, k)


def run_both(core, t, xyz, n_pts, **kw):
    """The session through the device (one call) and the reference, both from a cleared state; returns (got, reference tracker)."""
    kw = {**mt.DEFAULTS, **kw}
    core.set_marker_tracker(**kw)
    ref = mt.Tracker(**kw)
    got, want = core.track_markers(t, xyz, n_pts), ref.run(t, xyz, n_pts)
    same_outputs(got, want)
    same_state(core.marker_tracks(), ref.tracks())
    return got, ref


def session(frames, K_max, t0=100.0, rate=60.0):
    """frames: one list of points per frame -> t, xyz (unused slots 1e6), n_pts."""
    F = len(frames)
    xyz = np.full((F, K_max, 3), 1e6)
    for f, pts in enumerate(frames):
        if len(pts):
            xyz[f, :len(pts)] = pts
    return t0 + np.arange(F) / rate, xyz, np.array([len(p) for p in frames], dtype=np.int32)


# ---------------------------------------------------------------- 1. planted scenes
@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_scenes_equal_the_reference(mcore, scenes, name):
    s = scenes[name]
    # preconditions, on the reference alone: no planted marker ever changes id, no frame is FULL
    assert mt.id_switches(s["want"]["id"], s["truth"]) == 0
    assert not (s["want"]["mk_status"] & mt.ST_FULL).any()
    assert s["want"]["n_tracks"].max() > PLANTED[name][0]            # ghosts of the clutter coast next to the markers
    mcore.set_marker_tracker(**mt.DEFAULTS)
    got = mcore.track_markers(s["t"], s["xyz"], s["n_pts"])
    same_outputs(got, s["want"], name)
    same_state(mcore.marker_tracks(), s["state"], name)
    assert mt.id_switches(got["id"], s["truth"]) == 0


def test_many_rounds_equal_the_reference(mcore):
    """Scenes in which nearly every track has several admissible points (up to six rounds per frame, exact duplicates among the
    points): the rounds must commit what the sorted list commits."""
    for points, K_max, T_max, seed in ((64, 64, 64, 3), (30, 32, 20, 4), (12, 16, 64, 5)):
        t, xyz, n_pts = mt.crowded_scene(points, K_max, seed)
        run_both(mcore, t, xyz, n_pts, max_missed=2, T_max=T_max)


# ---------------------------------------------------------------- 2. lane shapes
def test_lane_shapes(mcore):
    rng = np.random.default_rng(2)
    grid = np.array([[a, b, c] for a in range(4) for b in range(4) for c in range(4)], dtype=np.float64) * 0.2
    moved = grid + rng.normal(0, 0.002, grid.shape)
    order = rng.permutation(64)
    with_nan = moved.copy()
    with_nan[5, 1] = np.nan
    t, xyz, n_pts = session([grid, moved[order], [], moved[:1], moved, moved, with_nan], 64)
    n_pts[4], n_pts[5] = -1, 65                                     # both count as 0
    got, ref = run_both(mcore, t, xyz, n_pts)
    assert got["id"][0].tolist() == list(range(64)) and got["n_tracks"][0] == 64
    assert got["id"][1].tolist() == order.tolist() and (got["hits"][1] == 2).all()          # every lane live, every lane matched
    for f in (2, 4, 5):
        assert (got["id"][f] == -1).all() and not got["hits"][f].any() and got["n_tracks"][f] == 64
    assert got["id"][3].tolist() == [0] + [-1] * 63 and got["hits"][3, 0] == 3
    want6 = np.arange(64)
    want6[5] = -1                                                   # the NaN point: no id, no birth, the others unaffected
    assert got["id"][6].tolist() == want6.tolist() and got["hits"][6, 5] == 0 and got["mk_status"][6] == 0
    assert got["n_tracks"][6] == 64 and ref.next_id == 64


# ---------------------------------------------------------------- 3. FULL
def test_full(mcore, scenes):
    far = [[float(k), 0.0, 0.0] for k in range(5)]
    t, xyz, n_pts = session([far, [[0.0, 9.0, 0.0]]], 8)
    got, ref = run_both(mcore, t, xyz, n_pts, T_max=4, max_missed=0)
    assert got["id"][0].tolist() == [0, 1, 2, 3, -1, -1, -1, -1] and got["mk_status"][0] == mt.ST_FULL and got["n_tracks"][0] == 4
    # the point that found no slot took no id: the next birth (all four tracks retire in frame 1) is number 4
    assert got["id"][1, 0] == 4 and got["mk_status"][1] == 0 and got["n_tracks"][1] == 1
    s = scenes["m5_k8"]
    got, ref = run_both(mcore, s["t"], s["xyz"], s["n_pts"], T_max=8)
    assert (got["mk_status"] & mt.ST_FULL).sum() > 10 and got["n_tracks"].max() == 8


# ---------------------------------------------------------------- 4. occlusion
def test_occlusion_keeps_the_id_up_to_max_missed(mcore):
    A, B, C = [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]
    M = 3
    frames = [[A, B, C]] + [[A, C]] * M + [[A, B, C]] + [[A, C]] * (M + 1) + [[A, B, C]]
    t, xyz, n_pts = session(frames, 4)
    got, ref = run_both(mcore, t, xyz, n_pts, max_missed=M)
    assert got["id"][M + 1].tolist() == [0, 1, 2, -1] and got["hits"][M + 1].tolist() == [M + 2, 2, M + 2, 0]   # hidden M frames: same id
    assert got["n_tracks"][2 * M + 2] == 2                                     # hidden M + 1 frames: retired in the last of them
    assert got["id"][-1].tolist() == [0, 3, 2, -1] and got["hits"][-1, 1] == 1  # ... and born again
    assert mcore.marker_tracks()["id"].tolist() == [0, 3, 2]                   # in the slot the old track left (lowest free)


# ---------------------------------------------------------------- 5. crossing
@pytest.mark.parametrize("alpha,last", [(0.0, [1, 0]), (0.5, [0, 1]), (1.0, [0, 1])])
def test_crossing(mcore, alpha, last):
    t, xyz, n_pts = mt.crossing_scene()
    got, ref = run_both(mcore, t, xyz, n_pts, vel_alpha=alpha)
    assert got["id"][0].tolist() == [0, 1] and got["id"][-1].tolist() == last and (got["n_tracks"] == 2).all()


# ---------------------------------------------------------------- 6. ties
def test_ties(mcore):
    P, Q = [0.25, 0.5, 1.0], [0.26, 0.5, 1.0]
    # two exactly equal points near one track: the smaller index gets it, the other is born
    got, _ = run_both(mcore, *session([[P], [Q, Q]], 4))
    assert got["id"][1].tolist() == [0, 1, -1, -1] and got["hits"][1].tolist() == [2, 1, 0, 0]
    # two tracks with bit-equal predictions (born on equal points, v = 0) and one point: the lower slot gets it
    got, _ = run_both(mcore, *session([[P, P], [Q]], 4))
    assert got["id"][0].tolist() == [0, 1, -1, -1] and got["id"][1].tolist() == [0, -1, -1, -1] and got["n_tracks"][1] == 2
    # a point at distance exactly `gate` (d2 == g2 in double: 0.5 * 0.5 == 0.25) is not matched, one ulp nearer is
    assert mt.pair_d2(np.zeros((1, 3)), np.array([[0.5, 0.0, 0.0]]))[0, 0] == 0.5 * 0.5
    got, _ = run_both(mcore, *session([[[0.0, 0.0, 0.0]], [[0.5, 0.0, 0.0]]], 4), gate=0.5)
    assert got["id"][1, 0] == 1 and got["n_tracks"][1] == 2
    got, _ = run_both(mcore, *session([[[0.0, 0.0, 0.0]], [[np.nextafter(0.5, 0.0), 0.0, 0.0]]], 4), gate=0.5)
    assert got["id"][1, 0] == 0 and got["n_tracks"][1] == 1


# ---------------------------------------------------------------- 7. time
def _track_dev(core, torch, t, xyz, n_pts):
    dev = torch.device("cuda", 0)
    F, K_max, _ = xyz.shape
    d_t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(dev)
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float64)).to(dev)
    d_n = torch.from_numpy(np.ascontiguousarray(n_pts, dtype=np.int32)).to(dev)
    z = lambda shape: torch.full(shape, 77, dtype=torch.int32, device=dev)   # noqa: E731  (every entry must be overwritten)
    o = {"id": z((F, K_max)), "hits": z((F, K_max)), "n_tracks": z((F,)), "mk_status": z((F,))}
    torch.cuda.synchronize()
    core.track_markers_dev(F, d_t.data_ptr(), K_max, d_xyz.data_ptr(), d_n.data_ptr(), *[o[k].data_ptr() for k in OUT_KEYS])
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def test_time(mcore):
    import torch
    from mocap_core import capi
    xs = [0.0, 0.02, 0.04, 0.05]
    _, xyz, n_pts = session([[[x, 0.0, 1.0]] for x in xs], 2)
    t = np.array([10.0, 10.5, 10.5, 10.25])                          # the same time twice, then backwards
    got, ref = run_both(mcore, t, xyz, n_pts)
    assert (got["id"][:, 0] == 0).all() and got["hits"][:, 0].tolist() == [1, 2, 3, 4]
    st = mcore.marker_tracks()
    assert st["vel"][0].tolist() == [0.0 + 0.5 * ((0.02 - 0.0) / 0.5 - 0.0), 0.0, 0.0]      # frame 1's; frames 2, 3 left it alone
    assert st["pos"][0].tolist() == [0.05, 0.0, 1.0] and st["t_seen"][0] == 10.25
    # a NaN time stamp through the _dev form: BAD_TIME, outputs -1 / 0, the state untouched
    for bad in (np.nan, np.inf, -np.inf):
        before = mcore.marker_tracks()
        out = _track_dev(mcore, torch, np.array([bad]), xyz[:1], n_pts[:1])
        assert out["id"].tolist() == [[-1, -1]] and not out["hits"].any() and out["n_tracks"].tolist() == [0]
        assert out["mk_status"].tolist() == [mt.ST_BAD_TIME]
        same_state(mcore.marker_tracks(), before, bad)
    # ... in the middle of a call: the frames around it go on as if it were not there
    t3 = np.array([10.75, np.nan, 11.0])
    x3 = session([[[0.06, 0.0, 1.0]], [[0.06, 0.0, 1.0]], [[0.07, 0.0, 1.0]]], 2)[1]
    out, want = _track_dev(mcore, torch, t3, x3, np.ones(3, dtype=np.int32)), ref.run(t3, x3, np.ones(3, dtype=np.int32))
    same_outputs(out, want)
    assert want["mk_status"].tolist() == [0, mt.ST_BAD_TIME, 0] and want["hits"][:, 0].tolist() == [5, 0, 6]
    same_state(mcore.marker_tracks(), ref.tracks())
    # the host form refuses it before anything runs
    before = mcore.marker_tracks()
    with pytest.raises(capi.MocapError) as e:
        mcore.track_markers(t3, x3, np.ones(3, dtype=np.int32))
    assert e.value.code == capi.MOCAP_E_ARG
    same_state(mcore.marker_tracks(), before)


# ---------------------------------------------------------------- 8. chunking
def test_every_cut_into_calls_is_bit_identical(mcore, scenes):
    import torch
    s = scenes["m20_k32"]
    t, xyz, n_pts = s["t"], s["xyz"], s["n_pts"]
    F = len(t)

    def run(cuts, dev=False):
        mcore.reset_marker_tracker()
        parts, f = [], 0
        for L in cuts:
            L = min(L, F - f)
            if dev:
                parts.append(_track_dev(mcore, torch, t[f:f + L], xyz[f:f + L], n_pts[f:f + L]))
            else:
                parts.append(mcore.track_markers(t[f:f + L], xyz[f:f + L], n_pts[f:f + L]))
            f += L
        assert f == F
        return {k: np.concatenate([p[k] for p in parts]) for k in OUT_KEYS}, mcore.marker_tracks()

    mcore.set_marker_tracker(**mt.DEFAULTS)
    for cuts in ([F], [F], [1] * F, [1, 7, 64, F]):                  # one call (twice), one frame per call, ragged chunks
        got, state = run(cuts)
        same_outputs(got, s["want"], cuts[:4])
        same_state(state, s["state"], cuts[:4])
    got, state = run([1, 7, 64, F], dev=True)                        # the _dev form is the same kernel
    same_outputs(got, s["want"], "dev")
    same_state(state, s["state"], "dev")


# ---------------------------------------------------------------- 9. live path
def _stream():
    """4 frames of the 8 x 16 synthetic stream, the markers drifting 5 mm per frame."""
    from mocap_core import synth
    rig = synth.ring_rig(8)
    drift = lambda sampled: sampled[:1] + np.arange(4)[:, None, None] * np.array([0.005, 0.0, 0.0])   # noqa: E731
    blobs, counts, _ = synth.make_blob_stream(rig, 4, 16, seed=31, noise_px=0.02, dropout=0.0, min_sep=0.15, world=drift)
    return rig, blobs, counts, 50.0 + np.arange(4) / 60.0


def test_track_frame_ids_is_track_frame_plus_the_tracker(mcore):
    import torch
    rig, blobs, counts, t = _stream()
    mcore.set_cameras(rig["K"], rig["R"], rig["t"])
    mcore.set_marker_tracker(**mt.DEFAULTS)
    plain = mcore.track_frame(blobs, counts, K_max=32, O_max=4)
    both = mcore.track_frame_ids(blobs, counts, t, K_max=32, O_max=4)
    for k, v in plain.items():
        assert both[k].tobytes() == v.tobytes(), k
    assert not both["status"].any() and both["n_pts"].min() >= 12
    state = mcore.marker_tracks()
    # the ids are the batch tracker's, and the reference's, on the same points (slots beyond n_pts hold NaN in the host arrays)
    xyz = np.nan_to_num(both["xyz"], nan=1e6)
    mcore.reset_marker_tracker()
    same_outputs(both, mcore.track_markers(t, xyz, both["n_pts"]), "track_markers")
    same_state(mcore.marker_tracks(), state)
    ref = mt.Tracker(**mt.DEFAULTS)
    same_outputs(both, ref.run(t, xyz, both["n_pts"]), "reference")
    same_state(state, ref.tracks())
    n = int(both["n_pts"][3])
    assert (both["hits"][3, :n] == 4).sum() >= 12 and (both["id"][3, :n] >= 0).all()      # the markers kept their ids over the 4 frames
    # one frame per call (the live loop), and the _dev form: the same ids
    mcore.reset_marker_tracker()
    for f in range(4):
        one = mcore.track_frame_ids(blobs[f:f + 1], counts[f:f + 1], t[f:f + 1], K_max=32, O_max=4)
        for k in OUT_KEYS + ("xyz", "n_pts", "pos", "n_obj"):
            assert one[k][0].tobytes() == both[k][f].tobytes(), (f, k)
    same_state(mcore.marker_tracks(), state)
    mcore.reset_marker_tracker()
    dev = torch.device("cuda", 0)
    F, C, M, K, O = 4, 8, 16, 32, 4
    d_in = [torch.from_numpy(a).to(dev) for a in (blobs, counts, t)]
    shapes = {"xyz": ((F, K, 3), torch.float64), "err": ((F, K), torch.float64), "corr": ((F, K, C), torch.int16),
              "n_pts": ((F,), torch.int32), "status": ((F,), torch.int32), "pos": ((F, O, 3), torch.float64),
              "heading": ((F, O), torch.float64), "error": ((F, O), torch.float64), "droneIndex": ((F, O), torch.int32),
              "n_obj": ((F,), torch.int32), "id": ((F, K), torch.int32), "hits": ((F, K), torch.int32),
              "n_tracks": ((F,), torch.int32), "mk_status": ((F,), torch.int32)}
    d = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
    torch.cuda.synchronize()
    mcore.track_frame_ids_dev(F, M, d_in[0].data_ptr(), d_in[1].data_ptr(), 5.0, K, 1 << 20,
                              *[d[k].data_ptr() for k in ("xyz", "err", "corr", "n_pts", "status")], O,
                              *[d[k].data_ptr() for k in ("pos", "heading", "error", "droneIndex", "n_obj")], d_in[2].data_ptr(),
                              *[d[k].data_ptr() for k in OUT_KEYS])
    mcore.synchronize()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    same_outputs(got, both, "track_frame_ids_dev")
    valid = np.arange(K)[None, :] < both["n_pts"][:, None]
    assert np.array_equal(got["n_pts"], both["n_pts"]) and np.array_equal(got["xyz"][valid], both["xyz"][valid])
    same_state(mcore.marker_tracks(), state)


def test_helpers_seam(mcore):
    from mocap_core import helpers, synth
    rig, blobs, counts, t = _stream()
    helpers.set_core(mcore)
    helpers.set_camera_params([{"intrinsic_matrix": rig["K"][i].tolist()} for i in range(8)])
    poses = synth.rig_to_pose_dicts(rig)
    try:
        helpers.set_marker_tracker()                                   # the issue's defaults: 0.05, 5, 0.5, 64
        assert mcore.marker_tracker == (0.05, 5, 0.5, 64)
        fused = []
        for f in range(4):
            ip = synth.frame_to_reference_lists(blobs[f], counts[f], as_int=True)
            errors, pts, objects, ids = helpers.track_frame_ids(ip, poses, now=t[f])
            assert len(ids) == len(pts) == len(errors) and all(isinstance(i, int) for i in ids)
            fused.append((pts, ids))
        assert sorted(fused[0][1]) == list(range(len(fused[0][1])))    # the first frame: births in point order
        assert len(set(fused[3][1]) & set(fused[0][1])) >= 12          # the markers kept their ids
        helpers.set_marker_tracker()                                   # again: cleared
        for f in range(4):
            assert helpers.track_markers(fused[f][0], now=t[f]) == fused[f][1], f
        assert helpers.track_markers([], now=t[3] + 0.1) == []
        # a core handed over later gets the remembered settings on first use
        mcore.set_marker_tracker(T_max=0)
        assert helpers.track_markers(fused[0][0], now=t[3] + 0.2) == list(range(len(fused[0][0])))
        assert mcore.marker_tracker == (0.05, 5, 0.5, 64)
    finally:
        helpers._state["markers"] = None


# ---------------------------------------------------------------- 10. errors and the off state
def test_errors_and_the_off_state(mcore, scenes):
    from mocap_core import capi
    rig, blobs, counts, t4 = _stream()
    mcore.set_cameras(rig["K"], rig["R"], rig["t"])
    s = scenes["m5_k8"]
    t, xyz, n_pts = s["t"], s["xyz"], s["n_pts"]

    def refused(fn, *a, **kw):
        with pytest.raises(capi.MocapError) as e:
            fn(*a, **kw)
        assert e.value.code == capi.MOCAP_E_ARG, fn.__name__

    def every_entry_is_refused():
        refused(mcore.reset_marker_tracker)
        refused(mcore.track_markers, t, xyz, n_pts)
        refused(mcore.track_markers_dev, 1, 0, 8, 0, 0, 0, 0, 0, 0)
        refused(mcore.marker_tracks)
        refused(mcore.track_frame_ids, blobs, counts, t4, K_max=32)
        refused(mcore.track_frame_ids_dev, 1, 16, 0, 0, 5.0, 32, 1 << 20, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)

    mcore.set_marker_tracker(T_max=0)                               # off = as before mocap_set_marker_tracker
    every_entry_is_refused()
    # bad parameters leave the previous settings, and the state, in force
    mcore.set_marker_tracker(**mt.DEFAULTS)
    ref = mt.Tracker(**mt.DEFAULTS)
    same_outputs(mcore.track_markers(t[:40], xyz[:40], n_pts[:40]), ref.run(t[:40], xyz[:40], n_pts[:40]))
    for kw in (dict(gate=0.0), dict(gate=-1.0), dict(gate=float("inf")), dict(gate=float("nan")), dict(max_missed=-1),
               dict(vel_alpha=-0.01), dict(vel_alpha=1.01), dict(vel_alpha=float("nan")), dict(T_max=65), dict(T_max=-1)):
        assert mt.validate(**{**mt.DEFAULTS, **kw}) is not None, kw
        refused(mcore.set_marker_tracker, **{**mt.DEFAULTS, **kw})
        assert mcore.marker_tracker == (0.05, 5, 0.5, 64)
    same_outputs(mcore.track_markers(t[40:], xyz[40:], n_pts[40:]), ref.run(t[40:], xyz[40:], n_pts[40:]))
    same_state(mcore.marker_tracks(), ref.tracks())
    # more than 64 point slots
    refused(mcore.track_markers, [0.0], np.zeros((1, 65, 3)), [0])
    refused(mcore.track_frame_ids, blobs, counts, t4, K_max=65)
    # the limits themselves are accepted
    mcore.set_marker_tracker(gate=1e-9, max_missed=0, vel_alpha=0.0, T_max=1)
    mcore.set_marker_tracker(gate=1e9, max_missed=2 ** 31 - 1, vel_alpha=1.0, T_max=64)
    # with the tracker off the other live calls return what they returned before
    mcore.set_marker_tracker(T_max=0)

    def live_calls():
        mcore.set_object_filter(2)
        try:
            return (mcore.track_frame(blobs, counts, K_max=32, O_max=4), mcore.track_frame_bodies(blobs, counts, K_max=32, O_max=4, B_max=2),
                    mcore.track_frame_filtered(blobs, counts, t4, K_max=32, O_max=4))
        finally:
            mcore.set_object_filter(0)

    before = live_calls()
    mcore.set_marker_tracker(**mt.DEFAULTS)
    mcore.track_frame_ids(blobs, counts, t4, K_max=32, O_max=4)
    mcore.set_marker_tracker(T_max=0)
    every_entry_is_refused()
    for a, b in zip(before, live_calls()):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
