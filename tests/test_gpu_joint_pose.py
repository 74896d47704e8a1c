"""Joint poses on the device (include/mocap_core.h, "joint poses"; csrc/joint_pose.hip) against the plain statement of the contract
(tests/joint_pose_reference.py): flag, hops and via exactly; quat, R, t_pose and rms_j bit for bit (any NaN equal to any NaN), at the
frame counts around a tile and the body counts up to the cap; chains, a star and a component nobody anchors; max_rms taken from a
try's own rms; NaN and huge values; the sign walk from a JOINTED first frame and across tile seams; the refusals with canaries; the
host and device forms, call after call, a second stream, behind mocap_pose_rows_dev; and the helper on the five-body scene."""
import numpy as np
import pytest

import body_session_reference as bsr
import joint_pose_reference as jp
import joints_reference as jr
import test_joint_pose_reference_cpu as cpu

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
OUT = ("flag", "hops", "via", "quat", "R", "t_pose", "rms_j")
SENTINEL = -7


def outputs(B, F, make, fill):
    o = {k: make((B, F), "int32", fill) for k in ("flag", "hops", "via")}
    o.update(quat=make((B, F, 4), "float64", float(fill)), R=make((B, F, 9), "float64", float(fill)),
             t_pose=make((B, F, 3), "float64", float(fill)), rms_j=make((B, F), "float64", float(fill)))
    return o


def host_fill(shape, dt, fill):
    return np.full(shape, fill, dtype=dt)


def dev_fill(shape, dt, fill):
    import torch
    return torch.full(shape, fill, dtype=getattr(torch, dt), device=torch.device("cuda", 0))


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))         # (a copy: the shared scene's arrays are read-only)


def dev_pose(core, traj, bodies, p, joints, axis_len=0.1, max_rms=INF, rounds=4):
    """mocap_pose_joints_dev into outputs pre-filled with the sentinel -> host arrays."""
    import torch
    R, F, _ = traj.shape
    B = len(bodies)
    d = [to_dev(traj), to_dev(p["flag"].astype(np.int32)), to_dev(p["quat"]), to_dev(p["R"]), to_dev(p["t_pose"])]
    o = outputs(B, F, dev_fill, SENTINEL)
    torch.cuda.synchronize()
    core.pose_joints_dev(F, R, d[0].data_ptr(), bodies, *[x.data_ptr() for x in d[1:]], joints, axis_len, max_rms, rounds,
                         *[o[k].data_ptr() for k in OUT])
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def statement(traj, bodies, p, joints, axis_len=0.1, max_rms=INF, rounds=4, trace=None):
    return jp.pose_joints(traj, bodies, p["flag"], p["quat"], p["R"], p["t_pose"], joints, axis_len, max_rms, rounds, trace=trace)


def assert_equal(got, ref, what):
    for k in jp.INT_OUT:
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5].tolist())
    for k in jp.F64_OUT:
        g, r = got[k].reshape(ref[k].shape), ref[k]
        assert jp.same_bits(g, r), (what, k, np.argwhere(~((g == r) | (np.isnan(g) & np.isnan(r))))[:5].tolist())


def chain(B):
    """Body b hangs on b - 1; every fourth body flies free."""
    return [-1 if b % 4 == 0 else b - 1 for b in range(B)]


# ---------------------------------------------------------------- 1. the device against the statement: frames, bodies
@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 255, 256, 257, 16385])
def test_frame_counts_around_a_tile(core, F, B):
    traj, bodies, joints, _ = jp.tree_session(F + B, F, [-1, 0, 1, 1, 3][:B])
    p = bsr.pose_rows(traj, bodies, INF)
    ref = statement(traj, bodies, p, joints)
    assert_equal(dev_pose(core, traj, bodies, p, joints), ref, (F, B))
    if F >= 63:
        assert (ref["flag"] == jp.JOINTED).any() and ((p["flag"] == jp.FEW) & (ref["flag"] == jp.FEW)).any()
    if F >= 255 and B == 5:
        assert (ref["hops"] == 2).any() and {jp.BALL, jp.HINGE} == {joints[j]["kind"] for j in np.unique(ref["via"][ref["via"] >= 0])}


@pytest.mark.parametrize("B", [2, 3, 5, 9, 64])
def test_body_counts_up_to_the_cap(core, B):
    traj, bodies, joints, _ = jp.tree_session(100 + B, 257, chain(B))
    p = bsr.pose_rows(traj, bodies, 0.01)
    ref = statement(traj, bodies, p, joints, max_rms=0.01)
    assert_equal(dev_pose(core, traj, bodies, p, joints, max_rms=0.01), ref, B)
    assert (ref["flag"] == jp.JOINTED).any()


# ---------------------------------------------------------------- 2. the skeleton's shapes
def _only_body_0_posed(seed, F, parent, n_seen):
    traj, bodies, joints, _ = jp.tree_session(seed, F, parent, n_markers=[4] * len(parent), shares={})
    for rows, _ in bodies[1:]:
        traj[rows[n_seen:]] = np.nan
    return traj, bodies, joints


@pytest.mark.parametrize("rounds", [1, 2, 3, 4, 16])
def test_a_chain_of_five_from_one_posed_body(core, rounds):
    traj, bodies, joints = _only_body_0_posed(31, 300, [-1, 0, 1, 2, 3], 2)
    p = bsr.pose_rows(traj, bodies, INF)
    assert (p["flag"][0] == jp.POSED).all() and (p["flag"][1:] == jp.FEW).all()
    ref = statement(traj, bodies, p, joints, rounds=rounds)
    assert_equal(dev_pose(core, traj, bodies, p, joints, rounds=rounds), ref, rounds)
    reach = min(rounds, 4)
    assert all((ref["hops"][b] == (b if b <= reach else -1)).all() for b in range(5))
    assert (ref["via"][1:reach + 1] == np.arange(reach)[:, None]).all()


def test_a_star_of_64_and_the_hub_through_its_lowest_open_joint(core):
    traj, bodies, joints, _ = jp.tree_session(32, 257, [-1] + [0] * 63, shares={0: 0.05, 1: 0.1, 2: 0.15})
    p = bsr.pose_rows(traj, bodies, INF)
    tr = {}
    ref = statement(traj, bodies, p, joints, trace=tr)
    assert_equal(dev_pose(core, traj, bodies, p, joints), ref, "star")
    hub = ref["flag"][0] == jp.JOINTED
    assert hub.any() and tr["contested"] > 0 and len(np.unique(ref["via"][0][hub])) > 1 and (ref["hops"] == 2).any()


def test_a_component_with_no_posed_body_stays_as_it_was(core):
    traj, bodies, joints, _ = jp.tree_session(33, 300, [-1, 0, -1, 2], n_markers=[4] * 4)
    for rows, _ in bodies[2:]:
        traj[rows[2:]] = np.nan
    p = bsr.pose_rows(traj, bodies, INF)
    ref = statement(traj, bodies, p, joints, rounds=16)
    assert_equal(dev_pose(core, traj, bodies, p, joints, rounds=16), ref, "two components")
    assert (ref["hops"][2:] == -1).all() and np.array_equal(ref["flag"][2:], p["flag"][2:]) and (ref["flag"][1] == jp.JOINTED).any()


# ---------------------------------------------------------------- 3. decisions at their edge, and values that are not numbers
def test_max_rms_at_a_trys_own_rms_and_one_double_below(core):
    traj, bodies, joints, _ = jp.tree_session(34, 400, [-1, 0, 1], sigma=0.0005)
    p = bsr.pose_rows(traj, bodies, INF)
    base = statement(traj, bodies, p, joints)
    b, f = np.argwhere((base["flag"] == jp.JOINTED) & (base["hops"] == 1) & (base["rms_j"] > 0))[0]
    r0 = float(base["rms_j"][b, f])
    for max_rms, kept in ((r0, True), (float(np.nextafter(r0, 0.0)), False)):
        ref = statement(traj, bodies, p, joints, max_rms=max_rms)
        assert (ref["flag"][b, f] == jp.JOINTED and ref["via"][b, f] == base["via"][b, f]) == kept
        assert_equal(dev_pose(core, traj, bodies, p, joints, max_rms=max_rms), ref, max_rms)


def test_nan_and_huge_values_in_an_anchors_pose_and_in_a_marker(core):
    traj, bodies, joints, _ = jp.tree_session(35, 600, [-1, 0, 1, 1, 3])
    f = np.arange(600)
    row = bodies[1][0][0]
    traj[row, f % 11 == 2, 1] = np.nan                       # a marker with one NaN is absent
    traj[row, f % 11 == 4, 0] = 1e200                        # finite: present, and the fit is what the arithmetic gives
    traj[row, f % 11 == 6, 2] = -1e200
    p = {k: v.copy() for k, v in bsr.pose_rows(traj, bodies, INF).items()}
    p["R"][0, f % 7 == 3, 1, 1] = np.nan
    p["t_pose"][0, f % 7 == 5, 2] = 1e200
    p["t_pose"][3, f % 7 == 6, 0] = -1e200
    p["quat"][0, f % 13 == 1, 2] = np.nan
    tr = {}
    ref = statement(traj, bodies, p, joints, trace=tr)
    assert_equal(dev_pose(core, traj, bodies, p, joints), ref, "not numbers")
    assert sum(v for k, v in tr.items() if isinstance(k, tuple) and k[-1] == "not finite") > 0
    ref = statement(traj, bodies, p, joints, max_rms=1e150)
    assert_equal(dev_pose(core, traj, bodies, p, joints, max_rms=1e150), ref, "not numbers, max_rms")


def test_sign_walk_from_a_jointed_first_frame_and_across_tile_seams(core):
    F = 770
    traj, bodies, joints, _ = jp.tree_session(36, F, [-1, 0, 1], n_markers=[4, 4, 4], shares={})
    rng = np.random.default_rng(36)
    hide = rng.uniform(size=(3, F)) < 0.25
    hide[1, [0, 1, 255, 256, 257, 511, 512, 513, 768, 769]] = True
    hide[0, [0, 1, 255, 256, 257, 511, 512, 513, 768, 769]] = False
    for b, (rows, _) in enumerate(bodies):
        for m in rows[2:]:
            traj[m, hide[b]] = np.nan                        # a hidden body shows two markers
    p = bsr.pose_rows(traj, bodies, INF)
    ref = statement(traj, bodies, p, joints)
    assert ref["flag"][1, 0] == jp.JOINTED and all(ref["flag"][1, f] == jp.JOINTED for f in (255, 256, 257, 511, 512, 513))
    got = dev_pose(core, traj, bodies, p, joints)
    assert_equal(got, ref, "sign walk")
    for b in range(3):                                        # one hemisphere along the carrying frames, the first leading positive
        q = got["quat"][b][(got["flag"][b] == jp.POSED) | (got["flag"][b] == jp.JOINTED)]
        assert (np.einsum("fi,fi->f", q[1:], q[:-1]) >= 0).all() and q[0][np.flatnonzero(q[0])[0]] > 0


# ---------------------------------------------------------------- 4. forms
def test_host_and_device_forms_streams_and_repeated_calls_give_the_same_bytes(core):
    import torch
    traj, bodies, joints, _ = jp.tree_session(37, 600, chain(9), sigma=0.0005)
    p = bsr.pose_rows(traj, bodies, 0.005)
    host = core.pose_joints(traj, bodies, p["flag"], p["quat"], p["R"], p["t_pose"], joints, 0.1, 0.005, 4)
    one = dev_pose(core, traj, bodies, p, joints, max_rms=0.005)
    two = dev_pose(core, traj, bodies, p, joints, max_rms=0.005)
    stream = torch.cuda.Stream(device=0)
    try:
        core.set_stream(stream.cuda_stream)
        other = dev_pose(core, traj, bodies, p, joints, max_rms=0.005)
    finally:
        core.set_stream(0)
    for k in OUT:
        assert host[k].tobytes() == one[k].tobytes() == two[k].tobytes() == other[k].tobytes(), k
        assert host[k].dtype == one[k].dtype and host[k].size == one[k].size
        assert not (one[k] == SENTINEL).any(), k
    assert_equal(host, statement(traj, bodies, p, joints, max_rms=0.005), "host")


def test_chained_behind_pose_rows_with_no_synchronise(core):
    """mocap_pose_rows_dev -> mocap_find_joints_dev -> mocap_pose_joints_dev on the context's stream with nothing in between (the
    joints are the statement's: they are host data)."""
    import torch
    _, traj, bodies, _, _, poses, _, _ = cpu.scene(0.0, 0.0, cpu.MAX_RMS)           # (no mislabelled samples: the joints found are the planted ones)
    R, F, _ = traj.shape
    B = len(bodies)
    found = jr.find_joints(poses["flag"], poses["R"], poses["t_pose"], 30, 1e-4, 0.01)
    joints = jr.scene_joints(found)
    assert [(j["a"], j["b"], j["kind"]) for j in joints] == [(0, 1, jr.BALL), (1, 2, jr.HINGE), (1, 3, jr.BALL)]   # (3 is rigid on 0)
    ref = statement(traj, bodies, poses, joints, max_rms=cpu.MAX_RMS)
    d_traj = to_dev(traj)
    p = {"quat": dev_fill((B, F, 4), "float64", -7.0), "R": dev_fill((B, F, 9), "float64", -7.0), "t_pose": dev_fill((B, F, 3), "float64", -7.0),
         "rms": dev_fill((B, F), "float64", -7.0)}
    p.update({k: dev_fill((B, F), "int32", SENTINEL) for k in ("n_used", "present", "flag")})
    fj = {k: dev_fill((B, B), "int32", SENTINEL) for k in ("cnt", "kind", "accepted")}
    fj.update({k: dev_fill((B, B, 3), "float64", -7.0) for k in ("lam", "centre", "axis")})
    fj.update(sep=dev_fill((B, B), "float64", -7.0), parent=dev_fill((B,), "int32", SENTINEL), n_joints=dev_fill((1,), "int32", SENTINEL))
    o = outputs(B, F, dev_fill, SENTINEL)
    torch.cuda.synchronize()
    core.pose_rows_dev(F, R, d_traj.data_ptr(), bodies, cpu.MAX_RMS, *[p[k].data_ptr() for k in core.POSE_OUT])
    core.find_joints_dev(F, B, p["flag"].data_ptr(), p["R"].data_ptr(), p["t_pose"].data_ptr(), 30, 1e-4, 0.01,
                         *[fj[k].data_ptr() for k in core.JOINTS_OUT])
    core.pose_joints_dev(F, R, d_traj.data_ptr(), bodies, p["flag"].data_ptr(), p["quat"].data_ptr(), p["R"].data_ptr(),
                         p["t_pose"].data_ptr(), joints, cpu.AXIS_LEN, cpu.MAX_RMS, cpu.ROUNDS, *[o[k].data_ptr() for k in OUT])
    core.synchronize()
    assert_equal({k: v.cpu().numpy() for k, v in o.items()}, ref, "chained")
    assert fj["parent"].cpu().numpy().tolist() == found["parent"].tolist()
    assert (ref["flag"] == jp.JOINTED).sum() > 300


# ---------------------------------------------------------------- 5. refusals
def test_every_refusal_leaves_its_outputs_untouched(core):
    from mocap_core import capi
    from mocap_core.capi import _p
    F = 120
    traj, bodies, joints, _ = jp.tree_session(38, F, [-1, 0, 1, 1, 3])
    traj = np.ascontiguousarray(traj)
    R, B = traj.shape[0], 5
    p = bsr.pose_rows(traj, bodies, INF)
    flag, quat, Rm, t = (np.ascontiguousarray(p[k]) for k in ("flag", "quat", "R", "t_pose"))

    def call(joints=joints, bodies=bodies, F=F, R=R, axis_len=0.1, max_rms=INF, rounds=4, null=None, J=None):
        Bn, n, rows, q = core._session_bodies(bodies)
        Jn, *arrays = core._joint_pose_arrays(joints)
        o = outputs(max(Bn, 1), max(F, 1), host_fill, SENTINEL)
        ptrs = [_p(traj), _p(n), _p(rows), _p(q), _p(flag), _p(quat), _p(Rm), _p(t)] + [_p(a) for a in arrays] + [_p(o[k]) for k in OUT]
        if null is not None:
            ptrs[null] = None
        rc = core.lib.mocap_pose_joints(core._h, F, R, ptrs[0], Bn, *ptrs[1:8], Jn if J is None else J, *ptrs[8:15], axis_len, max_rms, rounds,
                                        *ptrs[15:])
        assert all((o[k] == SENTINEL).all() for k in OUT)
        return rc

    def with_joint(i, **kw):
        return [dict(j, **kw) if n == i else j for n, j in enumerate(joints)]

    hinge = next(i for i, j in enumerate(joints) if j["kind"] == jp.HINGE)
    bad = [("a cycle", dict(joints=with_joint(3, a=2, b=3))), ("a duplicate pair", dict(joints=with_joint(3, a=1, b=0))),
           ("a FIXED kind", dict(joints=with_joint(0, kind=jr.FIXED))), ("an UNSEEN kind", dict(joints=with_joint(0, kind=jr.UNSEEN))),
           ("a bad axis norm", dict(joints=with_joint(hinge, axis_a=[0.0, 0.0, 1.001]))), ("a NaN axis", dict(joints=with_joint(hinge, axis_b=[NAN, 0.0, 1.0]))),
           ("axis_len 0", dict(axis_len=0.0)), ("axis_len NaN", dict(axis_len=NAN)), ("axis_len inf", dict(axis_len=INF)),
           ("axis_len < 0", dict(axis_len=-0.1)), ("max_rounds 0", dict(rounds=0)), ("max_rounds 17", dict(rounds=17)),
           ("J = B", dict(joints=joints + [dict(joints[0], a=0, b=4)])), ("J = 0", dict(J=0)), ("max_rms 0", dict(max_rms=0.0)),
           ("max_rms NaN", dict(max_rms=NAN)), ("a NaN centre", dict(joints=with_joint(1, c_b=[0.0, NAN, 0.0]))),
           ("a body outside", dict(joints=with_joint(0, b=5))), ("a = b", dict(joints=with_joint(0, a=1, b=1))),
           ("one body", dict(bodies=bodies[:1], joints=joints[:1])), ("a row used twice", dict(bodies=bodies[:4] + [bodies[3]])),
           ("n_frames 0", dict(F=0)), ("R 0", dict(R=0)), ("R too small", dict(R=R - 2))]
    for what, kw in bad:
        assert call(**kw) == capi.MOCAP_E_ARG, what
        assert b"mocap_pose_joints" in core.lib.mocap_last_error(core._h), what
    for i in range(22):                                                          # a null buffer, each in turn
        assert call(null=i) == capi.MOCAP_E_ARG, i
    with pytest.raises(capi.MocapError) as e:                                    # the device form refuses before anything is enqueued
        core.pose_joints_dev(F, R, 8, bodies, 8, 8, 8, 8, joints, 0.1, INF, 17, 8, 8, 8, 8, 8, 8, 8)
    assert e.value.code == capi.MOCAP_E_ARG
    # the edges of what is accepted
    edge = dict(axis_len=1e-300, max_rms=5e-324, rounds=16)
    got = core.pose_joints(traj, bodies, flag, quat, Rm, t, joints, edge["axis_len"], edge["max_rms"], edge["rounds"])
    assert_equal(got, statement(traj, bodies, p, joints, edge["axis_len"], edge["max_rms"], edge["rounds"]), "edges")


# ---------------------------------------------------------------- 6. the helper on the five-body scene
def test_helper_numpy_resident_and_statement_on_the_scene(core):
    from mocap_core import capi, helpers
    t, traj, bodies, joints, _, poses, ref, _ = cpu.scene()
    blist = [{"rows": rows, "markers": q} for rows, q in bodies]
    par = dict(axis_len=cpu.AXIS_LEN, max_rms=cpu.MAX_RMS, max_rounds=cpu.ROUNDS, degree=2, W=8, n_min=5, max_gap=4)
    helpers.set_core(core)
    a = helpers.session_joint_poses(t, {"traj": traj}, blist, poses, joints, **par)
    res_poses = {k: to_dev(v) for k, v in poses.items()}
    b = helpers.session_joint_poses(to_dev(t), {"traj": to_dev(traj)}, blist, res_poses, {"joints": joints}, **par)
    b = {k: v.cpu().numpy() for k, v in b.items()}
    assert_equal(a, ref, "helper")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype, k
    posed = jp.fill_flag(ref["flag"])
    assert np.array_equal(a["flag_posed"], posed)
    # the smoothers take the new tables unchanged; the fill is mocap_fill_rows' over the mapped flag
    tr = core.smooth_tracks(t, ref["t_pose"], 2, 8, INF, 5, 4)
    rot = core.smooth_rotations(t, ref["quat"], 2, 8, INF, 5, 4)
    assert a["pos"].tobytes() == tr["pos"].tobytes() and a["quat_s"].tobytes() == rot["quat_s"].tobytes() and np.array_equal(a["flag_s"], rot["flag"])
    fill = bsr.fill_rows(traj, bodies, posed, ref["R"], ref["t_pose"], rot["flag"], rot["quat_s"], tr["pos"])
    assert np.array_equal(a["src"], fill["src"]) and jp.same_bits(a["filled"], fill["filled"])
    want = np.zeros(a["src"].shape, dtype=bool)
    for y, (rows, _) in enumerate(bodies):
        want[rows] = (fill["src"][rows] == capi.BP_SRC_RIGID) & (ref["flag"][y] == jp.JOINTED)[None, :]
    assert np.array_equal(a["from_joint"], want) and want.sum() > 1000
    before = core.fill_rows(traj, bodies, poses["flag"], poses["R"], poses["t_pose"])
    assert (a["src"] == capi.BP_SRC_NONE).sum() < (before["src"] == capi.BP_SRC_NONE).sum() - 1000
    # with the mapped flag the joint's series sees the jointed frames
    series = helpers.session_joint_motion(t, {**a, "flag": a["flag_posed"]}, joints[:2])
    assert series["present"].sum() > helpers.session_joint_motion(t, poses, joints[:2])["present"].sum()
