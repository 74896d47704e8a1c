"""GPU: point refinement (include/mocap_core.h "point refinement", csrc/point_refine.hip) against its plain Python statement
(tests/point_refine_reference.py), the start taken from mocap_triangulate on the same observations.  No tolerance anywhere: the
header pins every operation, so xyz, err and info are compared bit for bit."""
import numpy as np
import pytest

import point_refine_reference as pr
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture()
def rcore(core):
    core.set_world_transform(None)
    core.set_point_refinement(0)
    yield core
    core.set_point_refinement(0)
    core.set_point_consolidation(0)
    core.set_world_transform(None)
    core.set_rigid_bodies([])


def _rig(C, kind):
    from mocap_core import synth
    if kind == "uniform":
        return synth.ring_rig(C)
    rig = synth.calibrated_ring_rig(C, seed=0)
    if kind == "skewed":                                   # a general 3 x 3 K: skew, and a last row that is not (0, 0, 1)
        for c in range(C):
            rig["K"][c, 0, 1] = 1.5 + 0.25 * c
            rig["K"][c, 2] = (1e-5 * (c + 1), -2e-5, 1.0 + 1e-3 * c)
    return rig


def _same(got, want, where=""):
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (where, k)
        assert got[k].tobytes() == want[k].tobytes(), (where, k, np.argwhere(got[k] != want[k])[:4].tolist())


# ---------------------------------------------------------------- 1. the observation form against the statement
@pytest.mark.parametrize("kind", ["uniform", "per_camera", "skewed"])
@pytest.mark.parametrize("iters", [1, 4, 16])
@pytest.mark.parametrize("C", [2, 3, 8, 64])
def test_observation_form_equals_the_statement(rcore, C, iters, kind):
    rig = _rig(C, kind)
    rcore.set_cameras(rig["K"], rig["R"], rig["t"])
    rng = np.random.default_rng(1000 * C + 10 * iters + len(kind))
    obs, _ = pr.random_groups(rig, 200, rng, noise=0.3, integer=(iters == 4))
    obs[5] = np.nan                                        # no view
    obs[6, 1:] = np.nan                                    # one view
    obs[7, int(np.nonzero(~np.isnan(obs[7, :, 0]))[0][0]), 1] = np.inf
    starts, _ = rcore.triangulate(obs)
    P = pr.camera_table(rig["K"], rig["R"], rig["t"])
    want = dict(zip(("xyz", "err", "info"), pr.triangulate_refined(P, obs, starts, iters)))
    assert want["info"][5] == want["info"][6] == pr.RF_FEW_VIEWS and want["info"][7] == pr.RF_BAD_OBS
    steps = want["info"] >> pr.RF_STEPS_SHIFT
    refined = (want["info"] & pr.RF_REFINED) != 0
    assert refined.sum() >= 190 and (steps[refined] >= 1).mean() > 0.5 and steps.max() <= iters
    got = dict(zip(("xyz", "err", "info"), rcore.triangulate_refined(obs, iters=iters)))
    _same(got, want, "host form")
    if iters == 4:                                         # the _dev form, err and info left out
        import torch
        dev = torch.device("cuda", 0)
        d_obs = torch.from_numpy(obs).to(dev)
        d_xyz = torch.zeros((200, 3), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        rcore.triangulate_refined_dev(200, d_obs.data_ptr(), iters, d_xyz.data_ptr())
        rcore.synchronize()
        assert d_xyz.cpu().numpy().tobytes() == want["xyz"].tobytes()


# ---------------------------------------------------------------- 2. the staged frame-path form
def _stream(C, K_max, F):
    """(rig, blobs, counts, gate) of a shape; (3, 4, .) is the calibrated golden rig."""
    from mocap_core import synth
    if C == 3:
        g = load_golden("frames_c3_calibK")
        return {"K": g["K"], "R": g["R"], "t": g["t"]}, g["blobs"][:F], g["counts"][:F], 5.0
    if C == 64:
        rig = synth.stress_rig(64)
        blobs, counts, _ = synth.make_stress_stream(rig, F, n_markers=48, seed=4)
        return rig, blobs, counts, synth.STRESS_GATE_PX
    rig = synth.ring_rig(C)
    markers = {1: 1, 16: 6}.get(K_max, 16)                 # (six markers and their twins fit sixteen slots in most frames)
    blobs, counts, _ = synth.make_blob_stream(rig, F, markers, seed=11, m_max=1 if K_max == 1 else 16,
                                              dropout=0.4 if K_max == 1 else 0.05)   # (one marker: two of the four frames lose it)
    return rig, blobs, counts, 5.0


def _starts_for(core, blobs, counts, corr, n_pts, status, K_max):
    """mocap_triangulate on every group the stage will refine -> start_of(views) for the statement."""
    rows, keys = [], []
    C = blobs.shape[1]
    for f in range(blobs.shape[0]):
        n = int(n_pts[f])
        if (int(status[f]) & pr.STATUS_SKIP) or n < 0 or n > K_max:
            continue
        for k in range(n):
            views, flags = pr.corr_views(blobs[f], counts[f], corr[f, k])
            if not flags and tuple(views) not in keys:
                keys.append(tuple(views))
                rows.append(pr.views_to_obs(views, C))
    table = {}
    if rows:
        xyz, _ = core.triangulate(np.array(rows))
        table = {k: x for k, x in zip(keys, xyz)}
    return lambda views: table[tuple(views)]


def _plant(blobs, counts, out, K_max):
    """The untouched cases, planted into copies of a frame-path result.  -> (blobs, counts, xyz, err, corr, n_pts, status, what)"""
    blobs, counts = blobs.copy(), counts.copy()
    xyz, err, corr, n, st = (out[k].copy() for k in ("xyz", "err", "corr", "n_out", "status"))
    F, what = len(n), {}
    # sentinels beyond n_out (and everywhere in frames the frame path flagged)
    for f in range(F):
        m = int(n[f]) if 0 <= n[f] <= K_max and not st[f] else 0
        xyz[f, m:] = -777.25
        err[f, m:] = -3.5
    order = [int(f) for f in np.argsort(-n) if not st[f] and 0 < n[f] <= K_max]
    if len(order) >= 6:
        what["overflow"], what["minus"], what["over"] = order[1], order[2], order[3]
        st[order[1]] |= 2
        n[order[2]] = -1
        n[order[3]] = K_max + 1
    f = order[0] if order else 0
    if order and n[f] >= 5:
        C = corr.shape[2]
        seen = lambda k: np.nonzero(corr[f, k] >= 0)[0]              # noqa: E731
        corr[f, 0, seen(0)[1:]] = -1                                 # one view
        corr[f, 1] = -1                                              # no view
        c2 = int(seen(2)[0])
        corr[f, 2, c2] = counts[f, c2]                               # an index >= counts
        c3 = int(seen(3)[-1])
        blobs[f, c3, corr[f, 3, c3], 0] = np.nan                     # a NaN blob
        what["rows"] = f
        assert C >= 2
    return blobs, counts, xyz, err, corr, n, st, what


def _refine_dev(core, blobs, counts, xyz, err, corr, n, st, iters, want_info=True, want_status=True):
    import torch
    dev = torch.device("cuda", 0)
    F, K_max = err.shape
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
         for k, v in (("blobs", blobs), ("counts", counts), ("xyz", xyz), ("err", err), ("corr", corr), ("n_pts", n), ("status", st))}
    d["info"] = torch.full((F, K_max), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    core.refine_points_dev(F, blobs.shape[2], d["blobs"].data_ptr(), d["counts"].data_ptr(), K_max, iters, d["xyz"].data_ptr(),
                           d["err"].data_ptr(), d["corr"].data_ptr(), d["n_pts"].data_ptr(), d["status"].data_ptr() if want_status else 0,
                           d["info"].data_ptr() if want_info else 0)
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


SHAPES = [(2, 1, 4), (3, 4, 6), (8, 16, 12), (8, 64, 6), (64, 256, 2)]
_staged = {}


def _staged_case(core, C, K_max, F):
    """One frame-path result per shape with the untouched cases planted, and the statement's answer: computed once."""
    rig, blobs, counts, gate = _stream(C, K_max, F)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    if (C, K_max, F) not in _staged:
        out = core.match_triangulate(blobs, counts, gate_px=gate, K_max=K_max)
        b, c, xyz, err, corr, n, st, what = _plant(blobs, counts, out, K_max)
        P = pr.camera_table(rig["K"], rig["R"], rig["t"])
        want = pr.refine_frames(P, b, c, xyz, err, corr, n, st, _starts_for(core, b, c, corr, n, st, K_max), 4)
        _staged[(C, K_max, F)] = dict(inputs=(b, c, xyz, err, corr, n, st), what=what, want=want)
    return _staged[(C, K_max, F)]


@pytest.mark.parametrize("C,K_max,F", SHAPES)
def test_staged_form_equals_the_statement_per_group(rcore, C, K_max, F):
    case = _staged_case(rcore, C, K_max, F)
    b, c, xyz, err, corr, n, st = case["inputs"]
    want = case["want"]
    refined = (want["info"] & pr.RF_REFINED) != 0
    assert refined.sum() >= 2 and ((want["info"] >> pr.RF_STEPS_SHIFT)[refined] >= 1).any() and (~refined).any()
    got = _refine_dev(rcore, b, c, xyz, err, corr, n, st, 4)
    _same(got, want, "dev")
    for k, v in (("corr", corr), ("n_pts", n), ("status", st), ("blobs", b), ("counts", c)):
        assert got[k].tobytes() == v.tobytes(), k
    # what is not refined keeps its bytes, the sentinels beyond n_out included
    assert got["xyz"][~refined].tobytes() == xyz[~refined].tobytes() and got["err"][~refined].tobytes() == err[~refined].tobytes()
    assert (got["xyz"][~refined] == -777.25).any()
    host = rcore.refine_points(b, c, xyz, err, corr, n, st, iters=4)
    _same(host, want, "host")
    # info may be NULL
    bare = _refine_dev(rcore, b, c, xyz, err, corr, n, st, 4, want_info=False)
    assert (bare["info"] == -9).all() and bare["xyz"].tobytes() == want["xyz"].tobytes() and bare["err"].tobytes() == want["err"].tobytes()


def test_untouched_cases_keep_their_bytes_and_say_why(rcore):
    C, K_max, F = 8, 16, 12
    case = _staged_case(rcore, C, K_max, F)
    b, c, xyz, err, corr, n, st = case["inputs"]
    what, want = case["what"], case["want"]
    assert set(what) == {"overflow", "minus", "over", "rows"}
    got = _refine_dev(rcore, b, c, xyz, err, corr, n, st, 4)
    for f in (what["overflow"], what["minus"], what["over"]):       # skipped frames: byte for byte, info 0
        assert not got["info"][f].any()
        assert got["xyz"][f].tobytes() == xyz[f].tobytes() and got["err"][f].tobytes() == err[f].tobytes()
    f = what["rows"]
    assert got["info"][f, :4].tolist() == [pr.RF_FEW_VIEWS, pr.RF_FEW_VIEWS, pr.RF_BAD_INDEX, pr.RF_BAD_OBS]
    assert got["xyz"][f, :4].tobytes() == xyz[f, :4].tobytes() and got["err"][f, :4].tobytes() == err[f, :4].tobytes()
    assert (got["info"][f, 4:] & pr.RF_REFINED).any() and not got["info"][f, int(n[f]):].any()
    _same(got, want)
    # two views along one ray (the same camera pose twice, the same pixel): the group keeps its start, with 0 accepted steps
    from mocap_core import synth
    rig = synth.ring_rig(2)
    K, R, t = rig["K"], np.array([rig["R"][0]] * 2), np.array([rig["t"][0]] * 2)
    rcore.set_cameras(K, R, t)
    blobs = np.zeros((1, 2, 1, 2), dtype=np.float32)
    blobs[0, :, 0] = (171.0, 140.0)
    counts = np.ones((1, 2), dtype=np.int32)
    corr1 = np.zeros((1, 1, 2), dtype=np.int16)
    start, e0 = rcore.triangulate(pr.views_to_obs([(0, 171.0, 140.0), (1, 171.0, 140.0)], 2)[None])
    one = _refine_dev(rcore, blobs, counts, start[None].copy(), e0[None].copy(), corr1, np.ones(1, dtype=np.int32), np.zeros(1, dtype=np.int32), 4)
    assert one["xyz"].tobytes() == start.tobytes() and one["info"][0, 0] >> pr.RF_STEPS_SHIFT == 0
    P = pr.camera_table(K, R, t)
    ref = pr.refine_frames(P, blobs, counts, start[None], e0[None], corr1, [1], None, lambda v: start[0], 4)
    _same(one, ref)


# ---------------------------------------------------------------- 3. the live loop
@pytest.fixture()
def chain(rcore):
    g = load_golden("track_apptsx_chain")
    rcore.set_cameras(g["K"], g["R"], g["t"])
    rcore.set_world_transform(g["to_world"])
    return g


POINTS = ("xyz", "err", "corr", "n_pts", "status")


def _valid(res, K):
    return np.arange(K)[None, :] < res["n_pts"][:, None]


def _same_points(got, want, K, where=""):
    assert np.array_equal(got["n_pts"], want["n_pts"]) and np.array_equal(got["status"], want["status"]), where
    v = _valid(want, K)
    for k in ("xyz", "err", "corr"):
        assert got[k][v].tobytes() == want[k][v].tobytes(), (where, k)


def _staged_refine(core, blobs, counts, off, iters=4):
    """The staged refine applied to a mode-off result: what the live loop's points must be with the mode on."""
    r = core.refine_points(blobs, counts, off["xyz"], off["err"], off["corr"], off["n_pts"], off["status"], iters=iters)
    assert ((r["info"] >> pr.RF_STEPS_SHIFT) >= 1).sum() > 20
    return dict(off, xyz=r["xyz"], err=r["err"])


def test_track_frame_is_the_staged_calls_with_the_refinement_between(rcore, chain):
    from mocap_core import capi
    g, K, O = chain, 48, 8
    off = rcore.track_frame(g["blobs"], g["counts"], K_max=K, O_max=O)
    assert not off["status"].any()
    want = _staged_refine(rcore, g["blobs"], g["counts"], off)
    v = _valid(off, K)
    assert (want["xyz"][v] != off["xyz"][v]).any() and (want["err"][v] != off["err"][v]).any()
    rcore.set_point_refinement(4)
    assert rcore.point_refinement == 4
    on = rcore.track_frame(g["blobs"], g["counts"], K_max=K, O_max=O)
    _same_points(on, want, K, "host")
    # the object search saw the refined points and errors: the staged call on them, bit for bit
    loc = rcore.locate_objects(want["xyz"], want["err"], want["n_pts"], O_max=O)
    assert np.array_equal(on["n_obj"], loc["n_obj"]) and loc["n_obj"].sum() > 20
    have = np.arange(O)[None, :] < loc["n_obj"][:, None]
    for k in ("pos", "heading", "error", "droneIndex"):
        assert on[k][have].tobytes() == loc[k][have].tobytes(), k
    # a batch of F frames equals F one-frame calls
    for f in (0, 7, 12):
        one = rcore.track_frame(g["blobs"][f:f + 1], g["counts"][f:f + 1], K_max=K, O_max=O)
        for k in POINTS + ("pos", "n_obj"):
            assert one[k][0].tobytes() == on[k][f].tobytes(), (f, k)
    # the world epilogue: the camera-frame refined point through the restated store, in its order and unfused
    rcore.set_point_refinement(0)
    rcore.set_world_transform(None)
    cam = _staged_refine(rcore, g["blobs"], g["counts"], rcore.track_frame(g["blobs"], g["counts"], K_max=K, O_max=0))
    moved = np.array([pr.store_point(g["to_world"], [float(a) for a in x]) for x in cam["xyz"][v]])
    assert moved.tobytes() == on["xyz"][v].tobytes() and cam["err"][v].tobytes() == on["err"][v].tobytes()
    rcore.set_world_transform(g["to_world"])
    # the device form
    import torch
    dev = torch.device("cuda", 0)
    F, C, M, _ = g["blobs"].shape
    d_in = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (g["blobs"], g["counts"])]
    shapes = {"xyz": ((F, K, 3), torch.float64), "err": ((F, K), torch.float64), "corr": ((F, K, C), torch.int16),
              "n_pts": ((F,), torch.int32), "status": ((F,), torch.int32)}
    d = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
    torch.cuda.synchronize()
    rcore.set_point_refinement(4)
    rcore.track_frame_dev(F, M, d_in[0].data_ptr(), d_in[1].data_ptr(), 5.0, K, 1 << 20, *[d[k].data_ptr() for k in POINTS])
    rcore.synchronize()
    _same_points({k: t.cpu().numpy() for k, t in d.items()}, want, K, "dev")
    # with consolidation also on: staged refine, then staged consolidate
    rcore.set_point_consolidation(capi.CONSOLIDATE_BLOBS)
    both = rcore.track_frame(g["blobs"], g["counts"], K_max=K, O_max=O)
    cons = rcore.consolidate_points(want["xyz"], want["err"], want["corr"], want["n_pts"], want["status"])
    assert (cons["n_pts"] < want["n_pts"]).any()
    _same_points(both, dict(cons, status=want["status"]), K, "refine + consolidate")
    rcore.set_point_consolidation(capi.CONSOLIDATE_OFF)
    # off again: the bytes from before the mode was ever on
    rcore.set_point_refinement(0)
    again = rcore.track_frame(g["blobs"], g["counts"], K_max=K, O_max=O)
    for k in off:
        assert again[k].tobytes() == off[k].tobytes(), k


def test_track_frame_bodies_sees_the_refined_points(rcore, chain):
    g, K, O = chain, 48, 4
    off = rcore.track_frame(g["blobs"], g["counts"], K_max=K, O_max=O)
    want = _staged_refine(rcore, g["blobs"], g["counts"], off)
    body = np.array([[0.0, 0.0, 0.0], [0.15, 0.0, 0.0], [0.075, 0.058, 0.0]])
    rcore.set_rigid_bodies([body], tol=0.03, max_rms=0.03)
    rcore.set_point_refinement(4)
    bod = rcore.track_frame_bodies(g["blobs"], g["counts"], K_max=K, O_max=O, B_max=2)
    _same_points(bod, want, K)
    staged = rcore.locate_rigid_bodies(np.nan_to_num(want["xyz"], nan=1e6), want["n_pts"], B_max=2)
    assert staged["found"].sum() > 0
    for k in staged:
        assert bod[k].tobytes() == staged[k].tobytes(), k


def test_track_frame_images_refines_the_points_of_its_own_blobs(rcore):
    from mocap_core import synth
    rig = synth.ring_rig(2)
    images, _ = synth.render_camera_frames(rig, 2, 6, seed=7)
    rcore.set_cameras(rig["K"], rig["R"], rig["t"])
    rcore.set_image_params(240, 320, rig["K"], [synth.REFERENCE_DISTORTION] * 2)
    off = rcore.track_frame_images(images, M_max=16, K_max=32, O_max=0)
    assert off["n_pts"].sum() >= 4 and not off["status"].any()
    r = rcore.refine_points(off["blobs"], off["counts"], off["xyz"], off["err"], off["corr"], off["n_pts"], off["status"], iters=4)
    assert (r["info"] & pr.RF_REFINED).sum() >= 4
    rcore.set_point_refinement(4)
    on = rcore.track_frame_images(images, M_max=16, K_max=32, O_max=0)
    _same_points(on, dict(off, xyz=r["xyz"], err=r["err"]), 32)
    for k in ("blobs", "counts", "blob_status"):
        assert on[k].tobytes() == off[k].tobytes(), k


# ---------------------------------------------------------------- 4. refusals
def test_refusals(rcore):
    from mocap_core import capi

    def refused(code, fn, *a, **kw):
        with pytest.raises(capi.MocapError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (fn.__name__, e.value)
        return str(e.value)

    g = load_golden("frames_c2_m1")
    blobs, counts = g["blobs"][:2], g["counts"][:2]
    xyz, err, corr, n = np.zeros((2, 2, 3)), np.zeros((2, 2)), np.full((2, 2, 2), -1, dtype=np.int16), np.zeros(2, dtype=np.int32)
    fresh = capi.MocapCore(0)                                       # no cameras
    try:
        assert "mocap_set_cameras" in refused(-3, fresh.refine_points_dev, 1, 1, 0, 0, 2, 4, 0, 0, 0, 0)
        refused(-3, fresh.refine_points, blobs, counts, xyz, err, corr, n)
        refused(-3, fresh.triangulate_refined_dev, 1, 0, 4, 0)
    finally:
        fresh.close()
    rcore.set_cameras(g["K"], g["R"], g["t"])
    for iters in (-1, 17):
        text = refused(capi.MOCAP_E_ARG, rcore.set_point_refinement, iters)
        assert "iters=%d" % iters in text and rcore.point_refinement == 0
        refused(capi.MOCAP_E_ARG, rcore.refine_points, blobs, counts, xyz, err, corr, n, iters=iters)
        refused(capi.MOCAP_E_ARG, rcore.triangulate_refined, np.zeros((1, 2, 2)), iters=iters)
    refused(capi.MOCAP_E_ARG, rcore.refine_points, blobs, counts, xyz, err, corr, n, iters=0)
    assert "null buffer" in refused(capi.MOCAP_E_ARG, rcore.refine_points_dev, 1, 1, 0, 0, 2, 4, 0, 0, 0, 0)
    refused(capi.MOCAP_E_ARG, rcore.refine_points_dev, 1, 1, 0, 0, 0, 4, 0, 0, 0, 0)             # K_max = 0
    rcore.refine_points_dev(0, 1, 0, 0, 2, 4, 0, 0, 0, 0)                                        # no frames: nothing is read
    # the mode is still off after the refused values: track_frame returns the frame path's points
    a = rcore.track_frame(blobs, counts, K_max=2, O_max=0)
    sep = rcore.match_triangulate(blobs, counts, K_max=2)
    v = np.arange(2)[None, :] < sep["n_out"][:, None]
    assert v.any() and a["xyz"][v].tobytes() == sep["xyz"][v].tobytes()
    # a _dev live call without d_corr is refused with a text of its own with the mode on
    import torch
    dev = torch.device("cuda", 0)
    d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    d = [torch.zeros(s, dtype=t, device=dev) for s, t in (((2, 2, 3), torch.float64), ((2, 2), torch.float64), ((2, 2, 2), torch.int16),
                                                          ((2,), torch.int32), ((2,), torch.int32))]
    torch.cuda.synchronize()
    args = lambda corr_ptr: (2, 1, d_b.data_ptr(), d_c.data_ptr(), 5.0, 2, 1 << 20, d[0].data_ptr(), d[1].data_ptr(), corr_ptr,   # noqa: E731
                             d[3].data_ptr(), d[4].data_ptr())
    rcore.set_point_refinement(4)
    text = refused(capi.MOCAP_E_ARG, rcore.track_frame_dev, *args(0))
    assert "refinement" in text and "d_corr" in text and "mocap_track_frame_dev" in text
    rcore.track_frame_dev(*args(d[2].data_ptr()))
    rcore.synchronize()


# ---------------------------------------------------------------- 5. the helpers seam
def test_helpers_seam(rcore):
    from mocap_core import helpers, synth
    rig = synth.calibrated_ring_rig(8, seed=0)
    blobs, counts, _ = synth.make_blob_stream(rig, 1, 6, seed=3)
    helpers.set_core(rcore)
    helpers.set_camera_params([{"intrinsic_matrix": rig["K"][i].tolist()} for i in range(8)])
    poses = synth.rig_to_pose_dicts(rig)
    lists = lambda: synth.frame_to_reference_lists(blobs[0], counts[0], as_int=True)   # noqa: E731
    try:
        e0, p0, _ = helpers.find_point_correspondance_and_object_points(lists(), poses, None)
        helpers.set_point_refinement(4)
        assert rcore.point_refinement == 4
        e1, p1, _ = helpers.find_point_correspondance_and_object_points(lists(), poses, None)
        sep = rcore.match_triangulate_auto(blobs, counts)
        r = rcore.refine_points(blobs, counts, sep["xyz"], sep["err"], sep["corr"], sep["n_out"], sep["status"], iters=4)
        k = int(sep["n_out"][0])
        assert k >= 4 and p1.tobytes() == r["xyz"][0, :k].tobytes() and e1.tobytes() == r["err"][0, :k].tobytes()
        assert p1.shape == p0.shape and (p1 != p0).any() and (e1 != e0).any()
        _, live, _ = helpers.track_frame(lists(), poses, is_locating_objects=False)
        assert np.asarray(live).tobytes() == p1.tobytes()
        # explicit correspondences
        obs, _ = pr.random_groups(rig, 5, np.random.default_rng(2))
        rows = [[None if np.isnan(u) else [u, v] for u, v in o] for o in obs]
        rows = [[p if p is not None else [None, None] for p in row] for row in rows]
        assert np.asarray(helpers.triangulate_points_refined(rows, poses), dtype=np.float64).tobytes() == rcore.triangulate_refined(obs, 4)[0].tobytes()
        # a core handed over later gets the remembered count on first use
        rcore.set_point_refinement(0)
        e2, p2, _ = helpers.find_point_correspondance_and_object_points(lists(), poses, None)
        assert rcore.point_refinement == 4 and p2.tobytes() == p1.tobytes()
        helpers.set_point_refinement(0)
        e3, p3, _ = helpers.find_point_correspondance_and_object_points(lists(), poses, None)
        assert p3.tobytes() == p0.tobytes() and e3.tobytes() == e0.tobytes()
    finally:
        helpers._state["refine"] = 0
