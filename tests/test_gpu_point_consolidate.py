"""GPU: point consolidation (include/mocap_core.h "point consolidation", csrc/point_consolidate.hip) against its plain Python
statement (tests/point_consolidate_reference.py).  No tolerance anywhere: the rule compares integers, and rows are moved, never
computed -- counts, source slots and every byte of xyz, err and corr are compared exactly."""
import numpy as np
import pytest

import marker_track_reference as mt
import point_consolidate_reference as pc
from conftest import load_golden

pytestmark = pytest.mark.gpu

ROWS = ("xyz", "err", "corr")
# (C, K_max, frames): one wave per frame up to 64 slots, 256 lanes above; (64, 256) has frames whose rows do not fit the kernel's
# row buffer at once (two groups)
SHAPES = [(2, 1, 6), (8, 16, 12), (8, 64, 12), (8, 65, 10), (8, 128, 10), (64, 256, 6)]


@pytest.fixture()
def pcore(core):
    core.set_world_transform(None)
    yield core
    core.set_point_consolidation(0)
    core.set_world_transform(None)
    core.set_marker_tracker(T_max=0)
    core.set_rigid_bodies([])


def _rig(core, C):
    from mocap_core import synth
    rig = synth.ring_rig(C)
    core.set_cameras(rig["K"], rig["R"], rig["t"])


def _frames(C, K_max, F, seed):
    """Random frames with a planted chain; the first ones have n = K_max, 0 and 1, then: nothing to drop, all but one dropped."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, K_max + 1, F)
    n[:3] = (K_max, 0, min(1, K_max))
    blob_range = 256 if C == 64 else max(2, min(256, K_max // 2))
    xyz, err, corr, n = pc.random_rows(rng, F, C, K_max, blob_range, n_pts=n, p_none=max(0.0, 1.0 - 3.0 / C), chain=12)
    if F > 4 and K_max > 1:
        m = K_max
        n[3] = n[4] = m
        corr[3:5, :m] = -1
        corr[3, np.arange(m), np.arange(m) // 256] = np.arange(m) % 256    # every point a blob of its own: nothing is dropped
        corr[4, :m, C - 1] = 255                                     # every point the same blob: one is left
        corr[4, :m, 0] = np.arange(m) % 256
        err[3:5, :m] = rng.random((2, m))
        xyz[3:5, :m] = rng.normal(0, 1, (2, m, 3))
    return xyz, err, corr, n


def _dev(core, xyz, err, corr, n_pts, status=None, want_src=True, want_n_in=True):
    """mocap_consolidate_points_dev on device copies; src and n_in start at -1 / -5 so that what is not written shows."""
    import torch
    dev = torch.device("cuda", 0)
    F, K_max = err.shape
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in (("xyz", xyz), ("err", err), ("corr", corr), ("n_pts", n_pts))}
    d_st = None if status is None else torch.from_numpy(np.ascontiguousarray(status, dtype=np.int32)).to(dev)
    d["src"] = torch.full((F, K_max), -1, dtype=torch.int32, device=dev)
    d["n_in"] = torch.full((F,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    core.consolidate_points_dev(F, K_max, d["xyz"].data_ptr(), d["err"].data_ptr(), d["corr"].data_ptr(), d["n_pts"].data_ptr(),
                                0 if d_st is None else d_st.data_ptr(), d["src"].data_ptr() if want_src else 0,
                                d["n_in"].data_ptr() if want_n_in else 0)
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(got, want, where="", keys=ROWS + ("n_pts", "src", "n_in")):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (where, k)


# ---------------------------------------------------------------- 1. the staged forms against the reference
@pytest.mark.parametrize("C,K_max,F", SHAPES)
def test_staged_forms_equal_the_reference(pcore, C, K_max, F):
    _rig(pcore, C)
    xyz, err, corr, n = _frames(C, K_max, F, seed=100 * C + K_max)
    want = pc.consolidate(xyz, err, corr, n)
    # the cases are what they claim to be
    assert want["n_in"].tolist() == n.tolist() and want["n_pts"][0] <= K_max and want["n_pts"][1] == 0
    if F > 4 and K_max > 1:
        assert want["n_pts"][3] == n[3] and want["n_pts"][4] == 1
        assert max(pc.longest_chain(err[f, :n[f]], corr[f, :n[f]]) for f in range(F)) >= 4
    if K_max > 1:
        assert (want["n_pts"] < n).any()
    # (reference: slots from the new count on are the input's)
    for f in range(F):
        m = want["n_pts"][f]
        assert all(np.array_equal(want[k][f, m:], v[f, m:]) for k, v in (("xyz", xyz), ("err", err), ("corr", corr)))
    _same(_dev(pcore, xyz, err, corr, n), want, "dev")
    host = pcore.consolidate_points(xyz, err, corr, n)
    _same(host, want, "host")


def test_unprocessed_frames_are_left_as_they_are(pcore):
    C, K_max, F = 8, 16, 10
    _rig(pcore, C)
    xyz, err, corr, n = pc.random_rows(np.random.default_rng(7), F, C, K_max, 4, n_pts=[12] * F)
    status = np.array([0, 1, 2, 4, 8, 16 | 2, 32 | 1, 0, 0, 0], dtype=np.int32)     # 8 = ROUNDED: informational, processed
    n[7], n[8] = K_max + 1, -1
    corr[9, 11, C - 1] = 256                                                        # one entry outside -1 .. 255
    want = pc.consolidate(xyz, err, corr, n, status)
    assert want["n_in"].tolist() == [12, -1, -1, -1, 12, -1, -1, -1, -1, -1]
    for f in (1, 2, 3, 5, 6, 7, 8, 9):
        assert all(np.array_equal(want[k][f], v[f]) for k, v in (("xyz", xyz), ("err", err), ("corr", corr), ("n_pts", n)))
    assert want["n_pts"][0] < 12 and want["n_pts"][4] < 12
    _same(_dev(pcore, xyz, err, corr, n, status), want, "dev")
    _same(pcore.consolidate_points(xyz, err, corr, n, status), want, "host")
    # an entry below -1, in a slot that counts
    corr[0, 0, 0] = -2
    want = pc.consolidate(xyz, err, corr, n, status)
    assert want["n_in"][0] == -1
    _same(_dev(pcore, xyz, err, corr, n, status), want, "dev, -2")


def test_null_optional_arguments(pcore):
    C, K_max, F = 8, 16, 8
    _rig(pcore, C)
    xyz, err, corr, n = _frames(C, K_max, F, seed=3)
    want = pc.consolidate(xyz, err, corr, n)
    got = _dev(pcore, xyz, err, corr, n, status=None, want_src=False, want_n_in=False)
    _same(got, want, "no src, no n_in", keys=ROWS + ("n_pts",))
    assert (got["src"] == -1).all() and (got["n_in"] == -5).all()
    got = _dev(pcore, xyz, err, corr, n, status=np.zeros(F, dtype=np.int32), want_src=True, want_n_in=False)
    _same(got, want, "no n_in", keys=ROWS + ("n_pts", "src"))
    # the host form with every optional pointer null, straight through the C ABI
    from mocap_core.capi import _p
    a = [np.array(v) for v in (xyz, err, corr, n)]
    pcore._check(pcore.lib.mocap_consolidate_points(pcore._h, F, K_max, *[_p(v) for v in a], None, None, None))
    for k, v in zip(ROWS + ("n_pts",), a):
        assert v.tobytes() == want[k].tobytes(), k
    # no frames: nothing is read
    pcore.consolidate_points_dev(0, 16, 0, 0, 0, 0)


@pytest.mark.parametrize("F", [1, 513])
def test_batch_sizes(pcore, F):
    C, K_max = 8, 16
    _rig(pcore, C)
    xyz, err, corr, n = pc.random_rows(np.random.default_rng(F), F, C, K_max, 6, p_none=0.6)
    want = pc.consolidate(xyz, err, corr, n)
    _same(_dev(pcore, xyz, err, corr, n), want, F)
    _same(pcore.consolidate_points(xyz, err, corr, n), want, F)


def test_twenty_launches_are_byte_identical(pcore):
    C, K_max, F = 8, 128, 24
    _rig(pcore, C)
    xyz, err, corr, n = _frames(C, K_max, F, seed=20)
    first = _dev(pcore, xyz, err, corr, n)
    _same(first, pc.consolidate(xyz, err, corr, n))
    for i in range(19):
        _same(_dev(pcore, xyz, err, corr, n), first, i)


# ---------------------------------------------------------------- 2. refusals
def test_refusals(pcore):
    from mocap_core import capi
    xyz, err, corr, n = pc.random_rows(np.random.default_rng(1), 2, 8, 16, 4)

    def refused(code, fn, *a, **kw):
        with pytest.raises(capi.MocapError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (fn.__name__, e.value)
        return str(e.value)

    fresh = capi.MocapCore(0)                                       # no cameras
    try:
        refused(-3, fresh.consolidate_points, xyz, err, corr, n)
        refused(-3, fresh.consolidate_points_dev, 1, 16, 0, 0, 0, 0)
    finally:
        fresh.close()
    _rig(pcore, 8)
    for mode in (2, -1, 7):
        refused(capi.MOCAP_E_ARG, pcore.set_point_consolidation, mode)
        assert pcore.point_consolidation == capi.CONSOLIDATE_OFF
    refused(capi.MOCAP_E_ARG, pcore.consolidate_points_dev, 1, 0, 0, 0, 0, 0)
    assert "1025" in refused(capi.MOCAP_E_LIMIT, pcore.consolidate_points_dev, 1, 1025, 0, 0, 0, 0)
    assert "257" in refused(capi.MOCAP_E_LIMIT, pcore.consolidate_points_dev, 1, 257, 0, 0, 0, 0)
    refused(capi.MOCAP_E_ARG, pcore.consolidate_points, np.zeros((1, 0, 3)), np.zeros((1, 0)), np.zeros((1, 0, 8), dtype=np.int16), [0])
    refused(capi.MOCAP_E_LIMIT, pcore.consolidate_points, np.zeros((1, 1025, 3)), np.zeros((1, 1025)),
            np.full((1, 1025, 8), -1, dtype=np.int16), [0])
    refused(capi.MOCAP_E_ARG, pcore.consolidate_points_dev, 1, 16, 0, 0, 0, 0)          # null buffers
    # a _dev live call without d_corr: fine with the mode off (as before), refused with a text of its own with it on
    import torch
    dev = torch.device("cuda", 0)
    rig, blobs, counts, _, _ = pc.drift_stream(2)
    d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    K = 32
    d = [torch.zeros(s, dtype=t, device=dev) for s, t in (((2, K, 3), torch.float64), ((2, K), torch.float64), ((2, K, 8), torch.int16),
                                                          ((2,), torch.int32), ((2,), torch.int32))]
    torch.cuda.synchronize()
    args = lambda corr_ptr: (2, 16, d_b.data_ptr(), d_c.data_ptr(), 5.0, K, 1 << 20, d[0].data_ptr(), d[1].data_ptr(), corr_ptr,   # noqa: E731
                             d[3].data_ptr(), d[4].data_ptr())
    pcore.set_point_consolidation(capi.CONSOLIDATE_BLOBS)
    text = refused(capi.MOCAP_E_ARG, pcore.track_frame_dev, *args(0))
    assert "consolidation" in text and "d_corr" in text
    pcore.track_frame_dev(*args(d[2].data_ptr()))
    pcore.synchronize()
    assert (d[3].cpu().numpy() > 0).all()
    # with the mode on the live loop takes at most 256 point slots
    refused(capi.MOCAP_E_LIMIT, pcore.track_frame, blobs, counts, K_max=1025, O_max=0)


# ---------------------------------------------------------------- 3. the live loop
@pytest.fixture()
def chain(pcore):
    g = load_golden("track_apptsx_chain")
    pcore.set_cameras(g["K"], g["R"], g["t"])
    pcore.set_world_transform(g["to_world"])
    return g


def _consolidated_staged(core, blobs, counts, K):
    """match_triangulate_auto + the reference consolidation: what the live loop's points must be with the mode on."""
    sep = core.match_triangulate_auto(blobs, counts, K_max=K)
    assert not sep["status"].any()
    want = pc.consolidate(sep["xyz"], sep["err"], sep["corr"], sep["n_out"], sep["status"])
    assert (want["n_pts"] < sep["n_out"]).any()                     # the input has twins
    return sep, want


def _same_points(got, want, K):
    assert np.array_equal(got["n_pts"], want["n_pts"])
    valid = np.arange(K)[None, :] < want["n_pts"][:, None]
    for k in ROWS:
        assert got[k][valid].tobytes() == want[k][valid].tobytes(), k
    return valid


def test_track_frame_is_the_staged_calls_with_the_consolidation_between(pcore, chain):
    from mocap_core import capi
    from oracle import mocap_oracle as mo
    g, K, O = chain, 48, 8
    sep, want = _consolidated_staged(pcore, g["blobs"], g["counts"], K)
    off = pcore.track_frame(g["blobs"], g["counts"], K_max=K, O_max=O)
    pcore.set_point_consolidation(capi.CONSOLIDATE_BLOBS)
    on = pcore.track_frame(g["blobs"], g["counts"], K_max=K, O_max=O)
    valid = _same_points(on, want, K)
    assert np.isnan(on["xyz"][~valid]).all() and not on["status"].any()       # only the kept slots travel to the caller
    # the object search saw the consolidated points: the staged call on them, bit for bit; counts and drone indices as the Python
    # statement of locate_objects finds them
    loc = pcore.locate_objects(want["xyz"], want["err"], want["n_pts"], O_max=O)
    assert np.array_equal(on["n_obj"], loc["n_obj"]) and loc["n_obj"].sum() > 20
    have = np.arange(O)[None, :] < loc["n_obj"][:, None]
    for k in ("pos", "heading", "error", "droneIndex"):
        assert on[k][have].tobytes() == loc[k][have].tobytes(), k
    for f in range(len(on["n_pts"])):
        m = int(want["n_pts"][f])
        objs = mo.locate_objects(want["xyz"][f, :m], want["err"][f, :m])
        assert len(objs) == on["n_obj"][f] and [o["droneIndex"] for o in objs][:O] == on["droneIndex"][f, :len(objs)].tolist(), f
    # one frame per call (the live use) gives the batch's frames
    for f in (0, 7, 12):
        one = pcore.track_frame(g["blobs"][f:f + 1], g["counts"][f:f + 1], K_max=K, O_max=O)
        for k in ROWS + ("n_pts", "pos", "n_obj"):
            assert one[k][0].tobytes() == on[k][f].tobytes(), (f, k)
    # corr not asked for: the stage runs on the device's own rows all the same
    F, C, M, _ = g["blobs"].shape
    o = pcore._track_outputs(F, K, O)
    o["corr"] = None
    pcore._check(pcore.lib.mocap_track_frame(pcore._h, F, M, capi._p(g["blobs"]), capi._p(g["counts"]), 5.0, K, 1 << 20,
                                             *pcore._track_ptrs(o, O)))
    assert np.array_equal(o["n_pts"], want["n_pts"]) and o["xyz"][valid].tobytes() == want["xyz"][valid].tobytes()
    # back to 0: what a context returns that never heard of the mode
    pcore.set_point_consolidation(capi.CONSOLIDATE_OFF)
    again = pcore.track_frame(g["blobs"], g["counts"], K_max=K, O_max=O)
    for k in off:
        assert again[k].tobytes() == off[k].tobytes(), k
    assert np.array_equal(off["n_pts"], sep["n_out"])
    fresh = capi.MocapCore(0)
    try:
        fresh.set_cameras(g["K"], g["R"], g["t"])
        fresh.set_world_transform(g["to_world"])
        never = fresh.track_frame(g["blobs"], g["counts"], K_max=K, O_max=O)
    finally:
        fresh.close()
    for k in off:
        assert never[k].tobytes() == off[k].tobytes(), k


def test_track_frame_ids_and_bodies_see_the_consolidated_points(pcore, chain):
    from mocap_core import capi
    g, K, O = chain, 48, 4
    F = g["blobs"].shape[0]
    t = 20.0 + np.arange(F) / 60.0
    sep, want = _consolidated_staged(pcore, g["blobs"], g["counts"], K)
    pcore.set_marker_tracker(**mt.DEFAULTS)
    ids_off = pcore.track_frame_ids(g["blobs"], g["counts"], t, K_max=K, O_max=O)
    pcore.set_point_consolidation(capi.CONSOLIDATE_BLOBS)
    pcore.reset_marker_tracker()
    ids_on = pcore.track_frame_ids(g["blobs"], g["counts"], t, K_max=K, O_max=O)
    _same_points(ids_on, want, K)
    ref = mt.Tracker(**mt.DEFAULTS)
    ref_out = ref.run(t, np.nan_to_num(want["xyz"], nan=1e6), want["n_pts"])
    for k in ("id", "hits", "n_tracks", "mk_status"):
        assert np.array_equal(ids_on[k], ref_out[k]), k
    state, rstate = pcore.marker_tracks(), ref.tracks()
    for k in ("id", "pos", "vel", "t_seen", "missed", "hits"):
        assert state[k].tobytes() == rstate[k].tobytes(), k
    assert ids_on["id"].max() < ids_off["id"].max()                 # fewer points, fewer births
    # rigid bodies: a triangle the size of the drones' LED pattern; the stage reads the consolidated points
    body = np.array([[0.0, 0.0, 0.0], [0.15, 0.0, 0.0], [0.075, 0.058, 0.0]])
    pcore.set_rigid_bodies([body], tol=0.03, max_rms=0.03)
    bod = pcore.track_frame_bodies(g["blobs"], g["counts"], K_max=K, O_max=O, B_max=2)
    _same_points(bod, want, K)
    staged = pcore.locate_rigid_bodies(np.nan_to_num(want["xyz"], nan=1e6), want["n_pts"], B_max=2)
    assert staged["found"].sum() > 10
    for k in staged:
        assert bod[k].tobytes() == staged[k].tobytes(), k
    # the _dev forms equal the host forms
    import torch
    dev = torch.device("cuda", 0)
    C, M = g["blobs"].shape[1:3]
    d_in = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (g["blobs"], g["counts"], t)]
    shapes = {"xyz": ((F, K, 3), torch.float64), "err": ((F, K), torch.float64), "corr": ((F, K, C), torch.int16),
              "n_pts": ((F,), torch.int32), "status": ((F,), torch.int32), "pos": ((F, O, 3), torch.float64),
              "heading": ((F, O), torch.float64), "error": ((F, O), torch.float64), "droneIndex": ((F, O), torch.int32),
              "n_obj": ((F,), torch.int32), "id": ((F, K), torch.int32), "hits": ((F, K), torch.int32),
              "n_tracks": ((F,), torch.int32), "mk_status": ((F,), torch.int32)}
    d = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
    torch.cuda.synchronize()
    pcore.reset_marker_tracker()
    pcore.track_frame_ids_dev(F, M, d_in[0].data_ptr(), d_in[1].data_ptr(), 5.0, K, 1 << 20,
                              *[d[k].data_ptr() for k in ("xyz", "err", "corr", "n_pts", "status")], O,
                              *[d[k].data_ptr() for k in ("pos", "heading", "error", "droneIndex", "n_obj")], d_in[2].data_ptr(),
                              *[d[k].data_ptr() for k in ("id", "hits", "n_tracks", "mk_status")])
    pcore.synchronize()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    _same_points(got, want, K)
    for k in ("id", "hits", "n_tracks", "mk_status", "n_obj"):
        assert np.array_equal(got[k], ids_on[k]), k
    have = np.arange(O)[None, :] < np.minimum(ids_on["n_obj"], O)[:, None]
    for k in ("pos", "heading", "error", "droneIndex"):
        assert got[k][have].tobytes() == ids_on[k][have].tobytes(), k
    rb_shapes = {"found": ((F, 2), torch.int32), "n_used": ((F, 2), torch.int32), "assign": ((F, 2, 8), torch.int8),
                 "R": ((F, 2, 9), torch.float64), "t": ((F, 2, 3), torch.float64), "rms": ((F, 2), torch.float64),
                 "score": ((F, 2), torch.float64), "rb_status": ((F, 2), torch.int32)}
    r = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in rb_shapes.items()}
    torch.cuda.synchronize()
    pcore.track_frame_bodies_dev(F, M, d_in[0].data_ptr(), d_in[1].data_ptr(), 5.0, K, 1 << 20,
                                 *[d[k].data_ptr() for k in ("xyz", "err", "corr", "n_pts", "status")], O,
                                 *[d[k].data_ptr() for k in ("pos", "heading", "error", "droneIndex", "n_obj")], 2,
                                 *[r[k].data_ptr() for k in rb_shapes])
    pcore.synchronize()
    _same_points({k: v.cpu().numpy() for k, v in d.items()}, want, K)
    for k, v in zip(staged, r.values()):
        assert v.cpu().numpy().tobytes() == staged[k].tobytes(), k
    # off again: track_frame_ids returns what it returned before the mode was ever set
    pcore.set_point_consolidation(capi.CONSOLIDATE_OFF)
    pcore.reset_marker_tracker()
    again = pcore.track_frame_ids(g["blobs"], g["counts"], t, K_max=K, O_max=O)
    for k in ids_off:
        assert again[k].tobytes() == ids_off[k].tobytes(), k


def test_helpers_seam(pcore):
    from mocap_core import capi, helpers, synth
    rig, blobs, counts, _, _ = pc.drift_stream(2)
    helpers.set_core(pcore)
    helpers.set_camera_params([{"intrinsic_matrix": rig["K"][i].tolist()} for i in range(8)])
    poses = synth.rig_to_pose_dicts(rig)
    lists = lambda f: synth.frame_to_reference_lists(blobs[f], counts[f], as_int=True)   # noqa: E731
    try:
        _, plain, _ = helpers.track_frame(lists(0), poses, is_locating_objects=False)
        helpers.set_point_consolidation(True)
        assert pcore.point_consolidation == capi.CONSOLIDATE_BLOBS
        _, fewer, _ = helpers.track_frame(lists(0), poses, is_locating_objects=False)
        assert 0 < len(fewer) < len(plain)
        # a core handed over later gets the remembered mode on first use
        pcore.set_point_consolidation(capi.CONSOLIDATE_OFF)
        _, again, _ = helpers.track_frame(lists(0), poses, is_locating_objects=False)
        assert pcore.point_consolidation == capi.CONSOLIDATE_BLOBS and np.array_equal(again, fewer)
        helpers.set_point_consolidation(False)
        _, back, _ = helpers.track_frame(lists(0), poses, is_locating_objects=False)
        assert np.array_equal(back, plain)
    finally:
        helpers._state["consolidate"] = capi.CONSOLIDATE_OFF


# ---------------------------------------------------------------- 4. the purpose, end to end
def test_the_drift_stream_keeps_its_identities(pcore):
    """150 frames of the 8 x 16 stream as bench.py makes it, sixteen markers drifting, through mocap_track_frame_ids with the
    tracker's defaults, the mode off and on.  The bounds are the issue's, measured on the CPU oracle (13.17 markers with exactly one
    point against 9.33; 59 ids against 449; 13 old tracks against 2)."""
    from mocap_core import capi
    rig, blobs, counts, t, markers = pc.drift_stream(150)
    pcore.set_cameras(rig["K"], rig["R"], rig["t"])
    lines = {}
    for mode in (capi.CONSOLIDATE_OFF, capi.CONSOLIDATE_BLOBS):
        pcore.set_point_consolidation(mode)
        pcore.set_marker_tracker(**mt.DEFAULTS)
        res = pcore.track_frame_ids(blobs, counts, t, K_max=48, O_max=0)
        assert not res["status"].any()
        one = two = far = 0
        shared = []
        for f in range(150):
            m = int(res["n_pts"][f])
            at, fr = pc.points_per_marker(res["xyz"][f, :m], markers[f])
            one, two, far = one + int((at == 1).sum()), two + int((at >= 2).sum()), far + fr
            if pc.shares_a_blob(res["corr"][f, :m]):
                shared.append(f)
        last = res["hits"][-1][:res["n_pts"][-1]]
        lines[mode] = dict(points=res["n_pts"].mean(), one=one / 150, two=two / 150, far=far / 150, ids=int(res["id"].max()) + 1,
                           old=int((last > 75).sum()), shared=len(shared))
        print(("on:  " if mode else "off: ") + ", ".join(f"{k} {v:.2f}" if isinstance(v, float) else f"{k} {v}" for k, v in lines[mode].items()))
    off, on = lines[capi.CONSOLIDATE_OFF], lines[capi.CONSOLIDATE_BLOBS]
    assert off["two"] > 1.0 and off["shared"] > 75                  # the input has the problem
    assert on["two"] == 0                                           # no frame has a marker with two points at it
    assert on["shared"] == 0                                        # no two points of a frame share a blob
    assert on["one"] >= 12
    assert on["ids"] * 4 <= off["ids"]
    assert on["old"] >= 10
