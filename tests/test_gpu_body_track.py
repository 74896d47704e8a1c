"""The body tracker on the GPU (csrc/body_track.hip, include/mocap_core.h "body tracker") against the plain statement of its
contract in tests/body_track_reference.py: sources, assignments, hits and missed exactly; poses against a 50-digit evaluation on
the GPU's own assignment; coasting and the state to 1e-9; chunk invariance bit for bit; the live path, the helpers, the refusals.
The scenes are those of body_track_reference.scene(), whose margins tests/test_body_track_reference_cpu.py asserts."""
import numpy as np
import pytest

import body_track_reference as br
from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL, MAX_RMS = br.TOL, br.MAX_RMS
# reference key -> the key of MocapCore.track_bodies
KEYS = {"tracked": "tracked", "source": "source", "n_used": "bt_n_used", "assign": "bt_assign", "R": "bt_R", "t": "bt_t",
        "rms": "bt_rms", "hits": "bt_hits", "missed": "bt_missed", "status": "bt_status"}
EXACT = ("tracked", "source", "n_used", "assign", "hits", "missed", "status")
BT_KEYS = tuple(KEYS.values())
STATE_KEYS = ("live", "R", "p", "v", "t_seen", "missed", "hits")


@pytest.fixture()
def bcore(core):
    from mocap_core import capi
    core.set_world_transform(None)
    yield core
    core.set_body_tracker(on=False)
    core.set_rigid_bodies([])
    core.set_point_consolidation(capi.CONSOLIDATE_OFF)


def setup(core, s, settings=None):
    core.set_rigid_bodies(s["bodies"], tol=TOL, max_rms=MAX_RMS)
    gate, max_missed, alpha = settings or s["settings"]
    core.set_body_tracker(gate=gate, max_missed=max_missed, vel_alpha=alpha)


def same_bytes(a, b, keys, what):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def check_against_reference(got, ref, bodies, xyz, state=None, ref_state=None, what=""):
    """Integers exactly; GUIDED / SEARCH poses by the rule of test_pose_against_fifty_digits on the GPU's own assignment; COAST
    poses and the state's p, v to 1e-9 absolute (the pose floor over the smallest dt is below 1e-11: slack, not a measurement)."""
    for k in EXACT:
        assert np.array_equal(got[KEYS[k]], ref[k]), (what, k, np.argwhere(got[KEYS[k]] != ref[k])[:4].tolist())
    F, B = ref["source"].shape
    worst, n_cases = 0.0, 0
    for f in range(F):
        for b in range(B):
            src = int(ref["source"][f, b])
            R, t, rms = got["bt_R"][f, b], got["bt_t"][f, b], got["bt_rms"][f, b]
            if src in (br.SRC_GUIDED, br.SRC_SEARCH):
                q, a = np.asarray(bodies[b]), got["bt_assign"][f, b]
                used = [m for m in range(len(q)) if a[m] >= 0]
                Q, P = q[used], xyz[f][[a[m] for m in used]]
                exact = br.pose_mp(Q, P)
                d_ref = br.pose_errors(*br.kabsch(Q, P), exact)
                d_gpu = br.pose_errors(R, t, rms, exact)
                floor = 64 * np.spacing(max(1.0, float(np.abs(t).max())))
                for k, name in enumerate(("R", "t", "rms")):
                    worst = max(worst, d_gpu[k] / max(16 * d_ref[k], floor))
                    assert d_gpu[k] <= max(16 * d_ref[k], floor), (what, f, b, name, d_gpu[k], d_ref[k], floor)
                assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and np.linalg.det(R) > 0, (what, f, b)
                n_cases += 1
            elif src == br.SRC_COAST:
                assert np.abs(R - ref["R"][f, b]).max() <= 1e-9 and np.abs(t - ref["t"][f, b]).max() <= 1e-9 and rms == 0.0, (what, f, b)
            else:
                assert not R.any() and not t.any() and rms == 0.0, (what, f, b)
    print(f"{what}: {n_cases} fitted poses, worst error / bound = {worst:.3f}")
    if state is not None:
        for k in ("live", "missed", "hits", "t_seen"):
            assert np.array_equal(state[k], ref_state[k]), (what, k)
        for k in ("p", "v"):
            assert np.abs(state[k] - ref_state[k]).max() <= 1e-9, (what, k, np.abs(state[k] - ref_state[k]).max())
    return n_cases


def _dev_outputs(torch, F, B_max, fill=77):
    dev = torch.device("cuda", 0)
    shapes = {"tracked": ((F, B_max), torch.int32), "source": ((F, B_max), torch.int32), "bt_n_used": ((F, B_max), torch.int32),
              "bt_assign": ((F, B_max, 8), torch.int8), "bt_R": ((F, B_max, 3, 3), torch.float64), "bt_t": ((F, B_max, 3), torch.float64),
              "bt_rms": ((F, B_max), torch.float64), "bt_hits": ((F, B_max), torch.int32), "bt_missed": ((F, B_max), torch.int32),
              "bt_status": ((F,), torch.int32)}
    return {k: torch.full(shape, fill, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}   # (every entry must be overwritten)


def track_dev(core, torch, t, xyz, n_pts, B_max):
    dev = torch.device("cuda", 0)
    F, K_max, _ = xyz.shape
    d_t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(dev)
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float64)).to(dev)
    d_n = torch.from_numpy(np.ascontiguousarray(n_pts, dtype=np.int32)).to(dev)
    o = _dev_outputs(torch, F, B_max)
    torch.cuda.synchronize()
    core.track_bodies_dev(F, d_t.data_ptr(), K_max, d_xyz.data_ptr(), d_n.data_ptr(), B_max, *[o[k].data_ptr() for k in BT_KEYS])
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


# ---------------------------------------------------------------- 1. planted scenes; 5. lane shapes (64 of 64, 8 markers, 8 bodies)
@pytest.mark.parametrize("name", ["planted1", "planted3", "full64", "eight"])
def test_planted_scenes_equal_the_reference(bcore, name):
    import torch
    s = br.scene(name)
    setup(bcore, s)
    got = bcore.track_bodies(s["t"], s["xyz"], s["n_pts"])
    n = check_against_reference(got, s["ref"], s["bodies"], s["xyz"], bcore.get_body_tracks(), s["ref_state"], name)
    assert n == int(np.isin(s["ref"]["source"], (br.SRC_GUIDED, br.SRC_SEARCH)).sum()) and n >= 40
    # a SEARCH pose is the search's own, byte for byte: the same arithmetic on the same assignment
    loc = bcore.locate_rigid_bodies(s["xyz"], s["n_pts"])
    took = got["source"] == br.SRC_SEARCH
    assert took.any() and (loc["found"][took] == 1).all()
    for bt_key, rb_key in (("bt_assign", "assign"), ("bt_R", "R"), ("bt_t", "t"), ("bt_rms", "rms")):
        assert got[bt_key][took].tobytes() == loc[rb_key][took].tobytes(), bt_key
    # the device form, and more body slots than bodies: the same bytes, the slots beyond zero
    bcore.reset_body_tracker()
    B = len(s["bodies"])
    wide = track_dev(bcore, torch, s["t"], s["xyz"], s["n_pts"], B + 2)
    for k in BT_KEYS[:-1]:
        assert wide[k][:, :B].tobytes() == got[k].tobytes() and not wide[k][:, B:].any(), k
    assert wide["bt_status"].tobytes() == got["bt_status"].tobytes()


# ---------------------------------------------------------------- 2. the symmetric body
def test_the_symmetric_body_keeps_its_labelling(bcore):
    s = br.scene("symmetric")
    setup(bcore, s)
    got = bcore.track_bodies(s["t"], s["xyz"], s["n_pts"])
    check_against_reference(got, s["ref"], s["bodies"], s["xyz"], bcore.get_body_tracks(), s["ref_state"], "symmetric")
    truth = s["truth"]["assign"]
    labels = {br.labelling(got["bt_assign"][f, 0], truth[f, 0], 5) for f in range(120)}
    assert got["tracked"].all() and len(labels) == 1 and -1 not in next(iter(labels)), labels
    # the per-frame search on the same frames does not: its labelling changes between found frames
    loc = bcore.locate_rigid_bodies(s["xyz"], s["n_pts"])
    lab = [br.labelling(loc["assign"][f, 0], truth[f, 0], 5) if loc["found"][f, 0] else None for f in range(120)]
    assert sum(lab[f] is not None and lab[f - 1] is not None and lab[f] != lab[f - 1] for f in range(1, 120)) >= 20
    # R turns 3 degrees per frame, never a quarter turn
    for f in range(1, 120):
        step = got["bt_R"][f, 0] @ got["bt_R"][f - 1, 0].T
        assert np.degrees(np.arccos(np.clip((np.trace(step) - 1) / 2, -1, 1))) < 6.0, f


# ---------------------------------------------------------------- 3. occlusion
def test_occlusion_coasts_retires_and_reacquires(bcore):
    s = br.scene("occlusion")
    setup(bcore, s)
    got = bcore.track_bodies(s["t"], s["xyz"], s["n_pts"])
    check_against_reference(got, s["ref"], s["bodies"], s["xyz"], bcore.get_body_tracks(), s["ref_state"], "occlusion")
    src = got["source"][:, 0].tolist()
    assert src[20:25] == [br.SRC_COAST] * 5 and src[25:29] == [br.SRC_NONE] * 4 and src[29] == br.SRC_SEARCH
    assert got["bt_missed"][20:25, 0].tolist() == [1, 2, 3, 4, 5] and got["bt_hits"][29, 0] == 1
    # COAST follows p + v dt from the state before the occlusion, the orientation held
    bcore.reset_body_tracker()
    bcore.track_bodies(s["t"][:20], s["xyz"][:20], s["n_pts"][:20])
    st = bcore.get_body_tracks()
    for f in range(20, 25):
        dt = s["t"][f] - st["t_seen"][0]
        assert got["bt_t"][f, 0].tobytes() == (st["p"][0] + st["v"][0] * dt).tobytes(), f
        assert got["bt_R"][f, 0].tobytes() == st["R"][0].tobytes(), f


# ---------------------------------------------------------------- 4. two identical bodies
def test_two_identical_bodies_keep_their_points(bcore):
    s = br.scene("identical")
    setup(bcore, s)
    got = bcore.track_bodies(s["t"], s["xyz"], s["n_pts"])
    check_against_reference(got, s["ref"], s["bodies"], s["xyz"], bcore.get_body_tracks(), s["ref_state"], "identical")
    truth = s["truth"]["assign"]
    for f in range(90):
        a0, a1 = got["bt_assign"][f, 0, :5], got["bt_assign"][f, 1, :5]
        assert not set(a0[a0 >= 0].tolist()) & set(a1[a1 >= 0].tolist()), f                    # disjoint claims
        for b in range(2):
            assert br.labelling(got["bt_assign"][f, b], truth[f, b], 5) == (0, 1, 2, 3, 4), (f, b)


# ---------------------------------------------------------------- 5. lane shapes: no points, n out of range, NaN points
def test_empty_out_of_range_and_nan_frames(bcore):
    s = br.scene("planted1")
    xyz, n_pts = s["xyz"].copy(), s["n_pts"].copy()
    n_pts[10], n_pts[11], n_pts[12] = 0, 99, -3                      # (the "no valid slot" rule: both count as 0)
    own = s["truth"]["assign"][20, 0]
    xyz[20, own[own >= 0][:3], 1] = np.nan                           # three of the body's points are not finite
    xyz[21, :, 0] = np.inf                                           # a frame without a finite point
    trk = br.Tracker(s["bodies"], TOL, MAX_RMS, *s["settings"])
    ref = trk.run(s["t"], xyz, n_pts)
    assert trk.margins_ok(), trk.margin
    assert ref["source"][10:13, 0].tolist() == [br.SRC_COAST] * 3 and ref["source"][21, 0] == br.SRC_COAST
    setup(bcore, s)
    got = bcore.track_bodies(s["t"], xyz, n_pts)
    check_against_reference(got, ref, s["bodies"], xyz, bcore.get_body_tracks(), trk.state(), "edge frames")


# ---------------------------------------------------------------- 6. chunk invariance, determinism
def test_every_cut_of_a_session_gives_the_same_bytes(bcore):
    import torch
    s = br.scene("planted3")
    F = len(s["t"])
    setup(bcore, s)
    whole = bcore.track_bodies(s["t"], s["xyz"], s["n_pts"])
    state = bcore.get_body_tracks()
    bcore.reset_body_tracker()
    same_bytes(bcore.track_bodies(s["t"], s["xyz"], s["n_pts"]), whole, BT_KEYS, "second run")
    same_bytes(bcore.get_body_tracks(), state, STATE_KEYS, "second run")
    for cuts, dev in (([1, F - 1], False), ([F // 2, F - F // 2], True), ([1] * F, False)):
        bcore.reset_body_tracker()
        parts, f = [], 0
        for L in cuts:
            sl = slice(f, f + L)
            parts.append(track_dev(bcore, torch, s["t"][sl], s["xyz"][sl], s["n_pts"][sl], 3) if dev
                         else bcore.track_bodies(s["t"][sl], s["xyz"][sl], s["n_pts"][sl]))
            f += L
        same_bytes({k: np.concatenate([p[k] for p in parts]) for k in BT_KEYS}, whole, BT_KEYS, cuts[:2])
        same_bytes(bcore.get_body_tracks(), state, STATE_KEYS, cuts[:2])


# ---------------------------------------------------------------- 7. time
def test_time_stamps(bcore):
    import torch
    from mocap_core import capi
    s = br.scene("planted1")
    t = s["t"][:8].copy()
    t[4], t[5] = t[3], t[3] - 0.5                                    # dt = 0 and dt < 0: v is kept, the prediction is p
    xyz, n_pts = s["xyz"][:8], s["n_pts"][:8]
    trk = br.Tracker(s["bodies"], TOL, MAX_RMS, *s["settings"])
    ref = trk.run(t, xyz, n_pts)
    assert trk.margins_ok() and (ref["source"][4:6, 0] == br.SRC_GUIDED).all()
    setup(bcore, s)
    bcore.track_bodies(t[:4], xyz[:4], n_pts[:4])
    v3 = bcore.get_body_tracks()["v"].copy()
    assert np.abs(v3[0]).max() > 0.05
    mid = bcore.track_bodies(t[4:6], xyz[4:6], n_pts[4:6])
    st = bcore.get_body_tracks()
    assert st["v"].tobytes() == v3.tobytes() and st["t_seen"][0] == t[5] and st["hits"][0] == ref["hits"][5, 0]
    for k in EXACT:
        assert np.array_equal(mid[KEYS[k]], ref[k][4:6]), k
    tail = bcore.track_bodies(t[6:], xyz[6:], n_pts[6:])
    for k in EXACT:
        assert np.array_equal(tail[KEYS[k]], ref[k][6:]), k
    # a time stamp that is not finite: the _dev form flags the frame and leaves the state alone, the host form refuses
    before = bcore.get_body_tracks()
    for bad in (np.nan, np.inf):
        tb = np.array([t[7] + 0.1, bad, t[7] + 0.2])
        out = track_dev(bcore, torch, tb[1:2], xyz[:1], n_pts[:1], 1)
        assert out["bt_status"].tolist() == [br.ST_BAD_TIME]
        for k in BT_KEYS[:-1]:
            assert not out[k].any(), k
        same_bytes(bcore.get_body_tracks(), before, STATE_KEYS, bad)
        with pytest.raises(capi.MocapError) as e:
            bcore.track_bodies(tb, xyz[:3], n_pts[:3])
        assert e.value.code == capi.MOCAP_E_ARG and "mocap_track_bodies: time stamp 1 is not finite" in str(e.value)
        same_bytes(bcore.get_body_tracks(), before, STATE_KEYS, bad)


# ---------------------------------------------------------------- 8. the live path
TRIANGLE = np.array([[0.0, 0.0, 0.0], [0.15, 0.0, 0.0], [0.075, 0.058, 0.0]])    # the size of the drones' LED pattern


@pytest.fixture()
def chain(bcore):
    g = load_golden("track_apptsx_chain")
    bcore.set_cameras(g["K"], g["R"], g["t"])
    bcore.set_world_transform(g["to_world"])
    yield g
    bcore.set_world_transform(None)


def test_track_frame_bodies_tracked_is_track_frame_bodies_plus_the_tracker(bcore, chain):
    import torch
    from mocap_core import capi
    g, K, O, B = chain, 48, 4, 2
    F, C, M, _ = g["blobs"].shape
    t = 20.0 + np.arange(F) / 60.0
    bcore.set_rigid_bodies([TRIANGLE], tol=0.03, max_rms=0.03)
    bcore.set_body_tracker(gate=0.08, max_missed=3, vel_alpha=0.5)
    plain = bcore.track_frame_bodies(g["blobs"], g["counts"], K_max=K, O_max=O, B_max=B)

    def tracked_on_its_own_points(both, what):
        """The tracker outputs of a live call are track_bodies' on the call's points, and leave the same state."""
        state = bcore.get_body_tracks()
        bcore.reset_body_tracker()
        staged = bcore.track_bodies(t, np.nan_to_num(both["xyz"], nan=1e6), both["n_pts"], B_max=B)
        same_bytes(both, staged, BT_KEYS, what)
        same_bytes(bcore.get_body_tracks(), state, STATE_KEYS, what)
        return state

    both = bcore.track_frame_bodies_tracked(g["blobs"], g["counts"], t, K_max=K, O_max=O, B_max=B)
    same_bytes(both, plain, plain.keys(), "shared outputs")
    # (the golden frames are independent scenes: the drone-sized triangle is found by the search or coasts, frame by frame)
    assert both["tracked"][:, 0].sum() > 10 and not both["tracked"][:, 1].any()
    assert (both["source"] == br.SRC_SEARCH).any() and (both["source"] == br.SRC_COAST).any()
    # SEARCH: the search's assignment, and its pose recomputed by the same arithmetic -- the search's own R, t, rms byte for byte
    took = both["source"] == br.SRC_SEARCH
    assert took.sum() > 10 and (both["found"][took] == 1).all()
    for bt_key, rb_key in (("bt_assign", "assign"), ("bt_R", "R"), ("bt_t", "t"), ("bt_rms", "rms"), ("bt_n_used", "n_used")):
        assert both[bt_key][took].tobytes() == both[rb_key][took].tobytes(), bt_key
    state = tracked_on_its_own_points(both, "host form")
    # one frame per call (the live loop)
    bcore.reset_body_tracker()
    for f in range(F):
        one = bcore.track_frame_bodies_tracked(g["blobs"][f:f + 1], g["counts"][f:f + 1], t[f:f + 1], K_max=K, O_max=O, B_max=B)
        for k in BT_KEYS + ("xyz", "n_pts", "found", "assign"):
            assert one[k][0].tobytes() == both[k][f].tobytes(), (f, k)
    same_bytes(bcore.get_body_tracks(), state, STATE_KEYS, "one frame per call")
    # the _dev form
    dev = torch.device("cuda", 0)
    d_in = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (g["blobs"], g["counts"], t)]
    shapes = {"xyz": ((F, K, 3), torch.float64), "err": ((F, K), torch.float64), "corr": ((F, K, C), torch.int16),
              "n_pts": ((F,), torch.int32), "status": ((F,), torch.int32), "pos": ((F, O, 3), torch.float64),
              "heading": ((F, O), torch.float64), "error": ((F, O), torch.float64), "droneIndex": ((F, O), torch.int32),
              "n_obj": ((F,), torch.int32), "found": ((F, B), torch.int32), "n_used": ((F, B), torch.int32),
              "assign": ((F, B, 8), torch.int8), "R": ((F, B, 9), torch.float64), "t": ((F, B, 3), torch.float64),
              "rms": ((F, B), torch.float64), "score": ((F, B), torch.float64), "rb_status": ((F, B), torch.int32)}
    d = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
    o = _dev_outputs(torch, F, B)
    torch.cuda.synchronize()
    bcore.reset_body_tracker()
    bcore.track_frame_bodies_tracked_dev(
        F, M, d_in[0].data_ptr(), d_in[1].data_ptr(), 5.0, K, 1 << 20, *[d[k].data_ptr() for k in ("xyz", "err", "corr", "n_pts", "status")],
        O, *[d[k].data_ptr() for k in ("pos", "heading", "error", "droneIndex", "n_obj")], B,
        *[d[k].data_ptr() for k in ("found", "n_used", "assign", "R", "t", "rms", "score", "rb_status")], d_in[2].data_ptr(),
        *[o[k].data_ptr() for k in BT_KEYS])
    bcore.synchronize()
    got = {k: v.cpu().numpy() for k, v in {**d, **o}.items()}
    same_bytes(got, both, BT_KEYS + ("n_pts", "found", "n_used", "assign", "R", "t", "rms", "score", "rb_status"), "_dev form")
    valid = np.arange(K)[None, :] < both["n_pts"][:, None]
    assert got["xyz"][valid].tobytes() == both["xyz"][valid].tobytes()
    same_bytes(bcore.get_body_tracks(), state, STATE_KEYS, "_dev form")
    # with the consolidation on the tracker sees the consolidated points
    bcore.set_point_consolidation(capi.CONSOLIDATE_BLOBS)
    plain_on = bcore.track_frame_bodies(g["blobs"], g["counts"], K_max=K, O_max=O, B_max=B)
    assert (plain_on["n_pts"] < plain["n_pts"]).any()
    bcore.reset_body_tracker()
    on = bcore.track_frame_bodies_tracked(g["blobs"], g["counts"], t, K_max=K, O_max=O, B_max=B)
    same_bytes(on, plain_on, plain_on.keys(), "shared outputs, consolidated")
    assert on["tracked"][:, 0].sum() > 10
    tracked_on_its_own_points(on, "consolidated")
    # no bodies registered: zero-filled, the shared outputs as track_frame_bodies gives them
    bcore.set_point_consolidation(capi.CONSOLIDATE_OFF)
    bcore.set_rigid_bodies([])
    none = bcore.track_frame_bodies_tracked(g["blobs"], g["counts"], t, K_max=K, O_max=O, B_max=B)
    for k in BT_KEYS:
        assert not none[k].any(), k
    for k in ("xyz", "n_pts", "pos", "n_obj"):
        assert none[k].tobytes() == plain[k].tobytes(), k


# ---------------------------------------------------------------- 9. the helpers seam
def test_helpers_seam(bcore):
    from mocap_core import helpers, synth
    rig = synth.ring_rig(4)
    rng = np.random.default_rng(19)
    q = br.make_body(rng, 4)
    R0 = br._rot([0.2, 1.0, 0.4], 0.7)

    def plant(sampled):
        out = sampled.copy()
        for f in range(out.shape[0]):
            out[f, :4] = (br._rot([0, 0, 1], 0.03 * f) @ R0 @ q.T).T + np.array([0.1 + 0.005 * f, -0.2, 0.3])
        return out

    blobs, counts, _ = synth.make_blob_stream(rig, 4, 6, seed=23, noise_px=0.02, dropout=0.0, truncate=False, world=plant)
    t = 70.0 + np.arange(4) / 60.0
    helpers.set_core(bcore)
    helpers.set_camera_params([{"intrinsic_matrix": rig["K"][i].tolist()} for i in range(4)])
    poses = synth.rig_to_pose_dicts(rig)
    try:
        helpers.set_rigid_bodies([{"name": "wand", "markers": q.tolist()}])
        helpers.set_body_tracker()                                     # the issue's defaults: 0.03, 10, 0.5
        assert bcore.body_tracker == (0.03, 10, 0.5)
        fused = []
        for f in range(4):
            ip = synth.frame_to_reference_lists(blobs[f], counts[f], as_int=False)
            errors, pts, objects, bodies = helpers.track_frame_bodies_tracked(ip, poses, now=t[f])
            assert len(pts) == len(errors) == 6 and len(bodies) == 1
            b = bodies[0]
            assert b["name"] == "wand" and b["source"] == ("search" if f == 0 else "guided") and b["hits"] == f + 1 and b["missed"] == 0
            fit = (b["R"] @ q.T).T + b["t"]
            assert sorted(b["markers"]) == sorted(set(b["markers"])) and np.abs(fit - pts[b["markers"]]).max() < 0.005
            fused.append((pts, b))
        payload = helpers.object_points_payload(errors, pts, objects, bodies=bodies)
        assert payload["bodies"][0]["source"] == "guided" and isinstance(payload["bodies"][0]["R"], list)
        helpers.set_body_tracker()                                     # again: cleared
        for f in range(4):
            (b,) = helpers.track_bodies(fused[f][0], now=t[f])
            assert b["source"] == fused[f][1]["source"] and b["markers"] == fused[f][1]["markers"]
            assert b["R"].tobytes() == fused[f][1]["R"].tobytes() and b["t"].tobytes() == fused[f][1]["t"].tobytes()
        (b,) = helpers.track_bodies([], now=t[3] + 1 / 60)            # no points: the body coasts
        assert b["source"] == "coast" and b["missed"] == 1 and b["markers"] == [-1] * 4
        # a core handed over later gets the remembered settings on first use
        bcore.set_body_tracker(on=False)
        (b,) = helpers.track_bodies(fused[0][0], now=t[3] + 0.5)
        assert b["source"] == "search" and b["hits"] == 1 and bcore.body_tracker == (0.03, 10, 0.5)
    finally:
        helpers._state["bodies"] = None
        helpers._state["body_tracker"] = None


# ---------------------------------------------------------------- 10. errors and the off state
def test_errors_and_the_off_state(bcore, chain):
    from mocap_core import capi
    g = chain
    s = br.scene("planted3")
    t, xyz, n_pts = s["t"][:6], s["xyz"][:6], s["n_pts"][:6]
    t4 = 20.0 + np.arange(g["blobs"].shape[0]) / 60.0

    def refused(text, fn, *a, **kw):
        with pytest.raises(capi.MocapError) as e:
            fn(*a, **kw)
        assert e.value.code == capi.MOCAP_E_ARG and text in str(e.value), (fn.__name__, str(e.value))

    dev_args = (1, 0, 32, 0, 0, 3) + (0,) * 10
    live_dev_args = (1, 16, 0, 0, 5.0, 32, 1 << 20) + (0,) * 5 + (0,) + (0,) * 5 + (3,) + (0,) * 8 + (0,) + (0,) * 10
    bcore.set_rigid_bodies(s["bodies"], tol=TOL, max_rms=MAX_RMS)
    bcore.set_body_tracker(on=False)                                 # off = as before mocap_set_body_tracker
    off = "mocap_set_body_tracker has not been called"
    refused("mocap_reset_body_tracker: " + off, bcore.reset_body_tracker)
    refused("mocap_track_bodies: " + off, bcore.track_bodies, t, xyz, n_pts)
    refused("mocap_track_bodies_dev: " + off, bcore.track_bodies_dev, *dev_args)
    refused("mocap_get_body_tracks: " + off, bcore.get_body_tracks)
    refused("mocap_track_frame_bodies_tracked: " + off, bcore.track_frame_bodies_tracked, g["blobs"], g["counts"], t4, K_max=32)
    refused("mocap_track_frame_bodies_tracked_dev: " + off, bcore.track_frame_bodies_tracked_dev, *live_dev_args)
    # with the tracker off the rigid-body entry points do what they did
    before = bcore.locate_rigid_bodies(xyz, n_pts)
    # bad settings leave the previous ones, and the state, in force
    setup(bcore, s)
    first = bcore.track_bodies(t[:3], xyz[:3], n_pts[:3])
    st = bcore.get_body_tracks()
    for kw in (dict(gate=0.0), dict(gate=float("inf")), dict(gate=float("nan")), dict(max_missed=-1), dict(vel_alpha=-0.1),
               dict(vel_alpha=1.5), dict(vel_alpha=float("nan"))):
        args = dict(gate=0.03, max_missed=10, vel_alpha=0.5)
        args.update(kw)
        refused("mocap_set_body_tracker: gate must be finite and > 0, max_missed >= 0, vel_alpha in [0, 1]", bcore.set_body_tracker, **args)
        assert bcore.body_tracker == (0.03, 10, 0.5)
    with pytest.raises(capi.MocapError):
        bcore._check(bcore.lib.mocap_set_body_tracker(bcore._h, 2, 0.03, 10, 0.5))
    same_bytes(bcore.get_body_tracks(), st, STATE_KEYS, "after refused settings")
    rest = bcore.track_bodies(t[3:], xyz[3:], n_pts[3:])
    for k in EXACT:
        assert np.array_equal(np.concatenate([first[KEYS[k]], rest[KEYS[k]]]), s["ref"][k][:6]), k
    after = bcore.locate_rigid_bodies(xyz, n_pts)
    same_bytes(after, before, before.keys(), "the search with the tracker on")
    # sizes and null buffers
    refused("mocap_track_bodies: K_max=65 exceeds the 64 points per frame the body tracker takes", bcore.track_bodies, [0.0],
            np.zeros((1, 65, 3)), [0])
    refused("mocap_track_bodies: B_max=2 is less than the 3 registered bodies", bcore.track_bodies, t, xyz, n_pts, B_max=2)
    refused("mocap_track_bodies_dev: null tracker buffer", bcore.track_bodies_dev, *dev_args)
    refused("mocap_track_bodies_dev: B_max=1 is less than the 3 registered bodies", bcore.track_bodies_dev, 1, 0, 32, 0, 0, 1, *(0,) * 10)
    refused("mocap_track_bodies_dev: bad size argument", bcore.track_bodies_dev, -1, 0, 32, 0, 0, 3, *(0,) * 10)
    refused("mocap_track_frame_bodies_tracked: K_max=65 exceeds", bcore.track_frame_bodies_tracked, g["blobs"], g["counts"], t4, K_max=65)
    refused("mocap_track_frame_bodies_tracked: B_max=1 is less than the 3 registered bodies", bcore.track_frame_bodies_tracked,
            g["blobs"], g["counts"], t4, K_max=32, B_max=1)
    bad_t = t4.copy()
    bad_t[2] = np.nan
    refused("mocap_track_frame_bodies_tracked: time stamp 2 is not finite", bcore.track_frame_bodies_tracked, g["blobs"], g["counts"],
            bad_t, K_max=32)
    refused("mocap_track_frame_bodies_tracked_dev: null tracker buffer", bcore.track_frame_bodies_tracked_dev, *live_dev_args)
    lib, h = bcore.lib, bcore._h
    assert lib.mocap_get_body_tracks(h, *(None,) * 7) == capi.MOCAP_E_ARG
    assert lib.mocap_last_error(h).decode() == "mocap_get_body_tracks: null buffer"
    same_bytes(bcore.get_body_tracks(), bcore.get_body_tracks(), STATE_KEYS, "read-out")
    # registering bodies again clears the slots and keeps the settings; so does reset, and set again
    assert bcore.get_body_tracks()["live"][:3].all()
    bcore.set_rigid_bodies(s["bodies"], tol=TOL, max_rms=MAX_RMS)
    zero = bcore.get_body_tracks()
    for k in STATE_KEYS:
        assert not zero[k].any(), k
    again = bcore.track_bodies(t[:3], xyz[:3], n_pts[:3])
    same_bytes(again, first, BT_KEYS, "after registering again")
    bcore.reset_body_tracker()
    assert not bcore.get_body_tracks()["live"].any()
    bcore.track_bodies(t[:3], xyz[:3], n_pts[:3])
    bcore.set_rigid_bodies([])                                       # B = 0 clears too
    assert not bcore.get_body_tracks()["live"].any()
    none = bcore.track_bodies(t, xyz, n_pts, B_max=2)                # no bodies registered: zero-filled
    for k in BT_KEYS:
        assert none[k].shape[0] == 6 and not none[k].any(), k
