"""Skeleton fit on the device (include/mocap_core.h, "skeleton fit"; csrc/skeleton_fit.hip) against the plain statement of the contract
(tests/skeleton_fit_reference.py): steps and n_act exactly; quat, R, t_pose, rms_s, cost0 and cost bit for bit (any NaN equal to any
NaN), at the frame counts around a tile and the body counts up to the cap, across a round's seam of the workspace; a chain and a star
of 64 and a component nobody anchors; frames without an active body, a cut chain, a body with no marker on a ball joint; iters and
w_joint at their ends; NaN and huge values; the sign walk across tile seams; the refusals with canaries; the host and device forms,
call after call, a second stream, behind the three stages before it; and the helper on the five-body scene."""
import numpy as np
import pytest

import body_session_reference as bsr
import joint_pose_reference as jp
import joints_reference as jr
import skeleton_fit_reference as sk
import test_joint_pose_reference_cpu as jcpu
import test_skeleton_fit_reference_cpu as cpu

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
OUT = ("quat", "R", "t_pose", "rms_s", "cost0", "cost", "steps", "n_act")
SENTINEL = -7
# the workspace of a round as csrc/skeleton_fit.hpp lays it out: 96 planes of doubles and one int32 per (body, frame), a double and
# an int32 per frame, whole tiles of 256 frames under 256 MiB
WS_CAP, TILE = 256 << 20, 256


def round_frames(B):
    return WS_CAP // (B * (96 * 8 + 4) + 12) // TILE * TILE


def outputs(B, F, make, fill):
    o = dict(quat=make((B, F, 4), "float64", float(fill)), R=make((B, F, 9), "float64", float(fill)), t_pose=make((B, F, 3), "float64", float(fill)),
             rms_s=make((B, F), "float64", float(fill)), cost0=make((F,), "float64", float(fill)), cost=make((F,), "float64", float(fill)),
             steps=make((F,), "int32", fill), n_act=make((F,), "int32", fill))
    return o


def host_fill(shape, dt, fill):
    return np.full(shape, fill, dtype=dt)


def dev_fill(shape, dt, fill):
    import torch
    return torch.full(shape, fill, dtype=getattr(torch, dt), device=torch.device("cuda", 0))


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))         # (a copy: the shared scene's arrays are read-only)


def dev_fit(core, traj, bodies, pj, joints, axis_len=0.1, w_joint=1.0, iters=8):
    """mocap_fit_skeleton_dev into outputs pre-filled with the sentinel -> host arrays."""
    import torch
    R, F, _ = traj.shape
    B = len(bodies)
    d = [to_dev(traj), to_dev(pj["flag"].astype(np.int32)), to_dev(pj["quat"]), to_dev(pj["t_pose"])]
    o = outputs(B, F, dev_fill, SENTINEL)
    torch.cuda.synchronize()
    core.fit_skeleton_dev(F, R, d[0].data_ptr(), bodies, *[x.data_ptr() for x in d[1:]], joints, axis_len, w_joint, iters,
                          *[o[k].data_ptr() for k in OUT])
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def assert_equal(got, ref, what):
    for k in sk.INT_OUT:
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5].tolist())
    for k in sk.F64_OUT:
        g, r = got[k].reshape(ref[k].shape), ref[k]
        assert sk.same_bits(g, r), (what, k, np.argwhere(~((g == r) | (np.isnan(g) & np.isnan(r))))[:5].tolist())


def check(core, traj, bodies, pj, joints, what, **kw):
    ref = cpu.fit(traj, bodies, pj, joints, **kw)
    assert_equal(dev_fit(core, traj, bodies, pj, joints, **kw), ref, what)
    return ref


def chain(B):
    """Body b hangs on b - 1; every fourth body flies free."""
    return [-1 if b % 4 == 0 else b - 1 for b in range(B)]


# ---------------------------------------------------------------- 1. the device against the statement: frames, bodies, a round's seam
@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 255, 256, 257, 16385])
def test_frame_counts_around_a_tile(core, F, B):
    traj, bodies, joints, pj = cpu.tree(F + B, F, [-1, 0, 1, 1, 3][:B])
    ref = check(core, traj, bodies, pj, joints, (F, B), iters=3)
    if F >= 63:
        assert (ref["steps"] > 0).any() and (ref["n_act"] == B - 1).any() and (ref["n_act"] < B - 1).any()


@pytest.mark.parametrize("B", [2, 3, 5, 9, 64])
def test_body_counts_up_to_the_cap(core, B):
    traj, bodies, joints, pj = cpu.tree(100 + B, 257, chain(B))
    ref = check(core, traj, bodies, pj, joints, B, iters=3)
    assert (ref["steps"] > 0).any() and (ref["n_act"] > 0).any()


def test_a_rounds_seam_of_the_workspace(core):
    B = 64
    F = round_frames(B) + TILE + 1
    assert round_frames(B) == 5376 and B * F * (96 * 8 + 4) > WS_CAP      # two rounds: a full one, and a tile and a frame
    traj, bodies, joints, _ = jp.tree_session(164, F, chain(B), n_markers=[3] * B, sigma=0.0005)
    p = bsr.pose_rows(traj, bodies, INF)                         # (stage 1's tables are start poses as good as the jointed ones)
    ref = check(core, traj, bodies, p, joints, "seam", iters=1)
    assert (ref["steps"][round_frames(B) - 2:round_frames(B) + 2] > 0).all() and (ref["n_act"] < 48).any()


# ---------------------------------------------------------------- 2. the skeleton's shapes
def test_a_chain_of_64_is_the_deepest_elimination(core):
    traj, bodies, joints, pj = cpu.tree(41, 130, [-1] + list(range(63)), shares={0: 0.01, 1: 0.01})
    assert sk.forest(64, joints)["depth"][63] == 63
    ref = check(core, traj, bodies, pj, joints, "chain", iters=3)
    assert (ref["n_act"] == 63).any() and (ref["steps"] > 0).all()


def test_a_star_of_64_adds_63_complements_into_one_block(core):
    traj, bodies, joints, pj = cpu.tree(42, 130, [-1] + [0] * 63, shares={0: 0.01, 1: 0.01})
    assert sk.forest(64, joints)["order"] == list(range(1, 64)) + [0]
    ref = check(core, traj, bodies, pj, joints, "star", iters=3)
    assert (ref["n_act"] == 63).any() and (ref["steps"] > 0).all()


def test_two_components_one_with_no_active_body(core):
    traj, bodies, joints, pj = cpu.tree(43, 300, [-1, 0, -1, 2], n_markers=[4] * 4)
    pj = {k: v.copy() for k, v in pj.items()}
    pj["flag"][2:] = jp.FEW
    ref = check(core, traj, bodies, pj, joints, "two components")
    assert np.isnan(ref["quat"][2:]).all() and (ref["n_act"] <= 1).all() and (ref["steps"] > 0).any()


# ---------------------------------------------------------------- 3. active and inactive bodies
def test_frames_without_an_active_body_a_cut_chain_and_a_body_without_markers(core):
    F = 300
    traj, bodies, joints, pj = cpu.tree(44, F, [-1, 0, 1, 2, 3], n_markers=[4] * 5, shares={})
    pj = {k: v.copy() for k, v in pj.items()}
    f = np.arange(F)
    pj["flag"][:, f % 5 == 1] = jp.FEW                          # a frame with no active body
    pj["flag"][2, f % 5 == 2] = jp.DEGENERATE                   # an inactive body in the middle of the chain
    assert joints[0]["kind"] == jp.BALL and (joints[0]["a"], joints[0]["b"]) == (0, 1)
    traj[np.ix_(bodies[1][0], np.flatnonzero(f % 5 == 3))] = np.nan   # body 1 keeps its pose and loses every marker: a ball joint and a hinge hold it
    traj[np.ix_(bodies[0][0], np.flatnonzero(f % 5 == 4))] = np.nan   # the root the same: one ball joint, its block singular but for lam
    ref = check(core, traj, bodies, pj, joints, "active and inactive")
    none = f % 5 == 1
    assert (ref["n_act"][none] == 0).all() and (ref["steps"][none] == 0).all() and (ref["cost0"][none] == 0).all() and np.isnan(ref["quat"][:, none]).all()
    assert (ref["n_act"][f % 5 == 2] == 2).all() and (ref["steps"][f % 5 == 2] > 0).all()
    bare = f % 5 == 3
    assert np.isnan(ref["rms_s"][1, bare]).all() and np.isfinite(ref["quat"][1, bare]).all() and (ref["steps"][bare] > 0).any()
    assert np.isfinite(ref["quat"][0, f % 5 == 4]).all() and np.isfinite(ref["cost"][f % 5 == 4]).all()


# ---------------------------------------------------------------- 4. parameters, and values that are not numbers
@pytest.mark.parametrize("iters", [1, 2, 16])
def test_iters(core, iters):
    traj, bodies, joints, pj = cpu.tree(45, 257, [-1, 0, 1, 1, 3])
    ref = check(core, traj, bodies, pj, joints, iters, iters=iters)
    assert (ref["steps"] <= iters).all() and (ref["steps"] > 0).any() and (iters > 2 or (ref["steps"] == iters).any())


@pytest.mark.parametrize("w_joint", [1e-6, 1.0, 1e6])
def test_w_joint(core, w_joint):
    traj, bodies, joints, pj = cpu.tree(46, 257, [-1, 0, 1, 1, 3])
    ref = check(core, traj, bodies, pj, joints, w_joint, w_joint=w_joint, iters=4)
    assert (ref["steps"] > 0).any() and (ref["cost"] <= ref["cost0"]).all()


def test_nan_and_huge_values_in_a_marker_and_in_a_start_pose(core):
    F = 600
    traj, bodies, joints, pj = cpu.tree(47, F, [-1, 0, 1, 1, 3])
    pj = {k: v.copy() for k, v in pj.items()}
    f = np.arange(F)
    row = bodies[1][0][0]
    traj[row, f % 11 == 2, 1] = np.nan                       # a marker with one NaN is absent
    traj[row, f % 11 == 4, 0] = 1e200                        # finite: present, and the start cost is not finite
    traj[row, f % 11 == 6, 2] = -1e200
    pj["t_pose"][0, f % 7 == 5, 2] = 1e200                   # finite: the body is active, and the start cost is not finite
    pj["t_pose"][3, f % 7 == 6, 0] = -1e200
    pj["quat"][0, f % 13 == 1, 2] = np.nan                   # not finite: the body is inactive
    pj["t_pose"][2, f % 13 == 3, 1] = np.inf
    ref = check(core, traj, bodies, pj, joints, "not numbers", iters=4)
    bad = ~np.isfinite(ref["cost0"])
    assert bad.sum() > 100 and (ref["steps"][bad] == 0).all() and (ref["steps"][~bad] > 0).any()
    kept = bad & (pj["flag"][4] == jp.POSED)                 # a frame left alone keeps its start pose to the bit, up to the walk's sign
    assert kept.any() and np.array_equal(np.abs(ref["quat"][4, kept]), np.abs(pj["quat"][4, kept])) and np.array_equal(ref["t_pose"][4, kept], pj["t_pose"][4, kept])
    assert np.isnan(ref["quat"][0, f % 13 == 1]).all() and np.isnan(ref["quat"][2, f % 13 == 3]).all()


def test_sign_walk_across_tile_seams(core):
    F = 770
    traj, bodies, joints, pj = cpu.tree(48, F, [-1, 0, 1], n_markers=[4, 4, 4], shares={0: 0.1})
    pj = {k: v.copy() for k, v in pj.items()}
    rng = np.random.default_rng(48)
    pj["quat"][rng.uniform(size=(3, F)) < 0.5] *= -1.0       # the start's signs at random: the walk is the fit's own
    seams = [0, 1, 255, 256, 257, 511, 512, 513, 768, 769]
    pj["quat"][0, seams] = -np.abs(pj["quat"][0, seams])
    pj["flag"][1, [255, 512]] = jp.FEW                       # a carrying frame missing on either side of a seam
    pj["t_pose"][2, [256, 511], 0] = np.nan                  # ... and one that carries a flag and no pose
    ref = check(core, traj, bodies, pj, joints, "sign walk", iters=2)
    for b in range(3):                                       # one hemisphere along the frames with a pose, the first leading positive
        q = ref["quat"][b][np.isfinite(ref["quat"][b]).all(axis=1)]
        assert (np.einsum("fi,fi->f", q[1:], q[:-1]) >= 0).all() and q[0][np.flatnonzero(q[0])[0]] > 0


# ---------------------------------------------------------------- 5. forms
def test_host_and_device_forms_streams_and_repeated_calls_give_the_same_bytes(core):
    import torch
    traj, bodies, joints, pj = cpu.tree(49, 600, chain(9))
    host = core.fit_skeleton(traj, bodies, pj["flag"], pj["quat"], pj["t_pose"], joints, 0.1, 1.0, 4)
    one = dev_fit(core, traj, bodies, pj, joints, iters=4)
    two = dev_fit(core, traj, bodies, pj, joints, iters=4)
    stream = torch.cuda.Stream(device=0)
    try:
        core.set_stream(stream.cuda_stream)
        other = dev_fit(core, traj, bodies, pj, joints, iters=4)
    finally:
        core.set_stream(0)
    for k in OUT:
        assert host[k].tobytes() == one[k].tobytes() == two[k].tobytes() == other[k].tobytes(), k
        assert host[k].dtype == one[k].dtype and host[k].size == one[k].size
        assert not (one[k] == SENTINEL).any(), k
    assert_equal(host, cpu.fit(traj, bodies, pj, joints, iters=4), "host")


def test_chained_behind_the_three_stages_before_it_with_no_synchronise(core):
    """mocap_pose_rows_dev -> mocap_find_joints_dev -> mocap_pose_joints_dev -> mocap_fit_skeleton_dev on the context's stream with
    nothing in between (the joints are the statement's: they are host data)."""
    import torch
    _, traj, bodies, _, _, poses, _, _ = jcpu.scene(0.0, 0.0, jcpu.MAX_RMS)
    R, F, _ = traj.shape
    B = len(bodies)
    joints = jr.scene_joints(jr.find_joints(poses["flag"], poses["R"], poses["t_pose"], 30, 1e-4, 0.01))
    pj = jp.pose_joints(traj, bodies, poses["flag"], poses["quat"], poses["R"], poses["t_pose"], joints, jcpu.AXIS_LEN, jcpu.MAX_RMS, jcpu.ROUNDS)
    ref = cpu.fit(traj, bodies, pj, joints, iters=3)
    d_traj = to_dev(traj)
    p = {"quat": dev_fill((B, F, 4), "float64", -7.0), "R": dev_fill((B, F, 9), "float64", -7.0), "t_pose": dev_fill((B, F, 3), "float64", -7.0),
         "rms": dev_fill((B, F), "float64", -7.0)}
    p.update({k: dev_fill((B, F), "int32", SENTINEL) for k in ("n_used", "present", "flag")})
    fj = {k: dev_fill((B, B), "int32", SENTINEL) for k in ("cnt", "kind", "accepted")}
    fj.update({k: dev_fill((B, B, 3), "float64", -7.0) for k in ("lam", "centre", "axis")})
    fj.update(sep=dev_fill((B, B), "float64", -7.0), parent=dev_fill((B,), "int32", SENTINEL), n_joints=dev_fill((1,), "int32", SENTINEL))
    j = {k: dev_fill((B, F), "int32", SENTINEL) for k in ("flag", "hops", "via")}
    j.update(quat=dev_fill((B, F, 4), "float64", -7.0), R=dev_fill((B, F, 9), "float64", -7.0), t_pose=dev_fill((B, F, 3), "float64", -7.0),
             rms_j=dev_fill((B, F), "float64", -7.0))
    o = outputs(B, F, dev_fill, SENTINEL)
    torch.cuda.synchronize()
    core.pose_rows_dev(F, R, d_traj.data_ptr(), bodies, jcpu.MAX_RMS, *[p[k].data_ptr() for k in core.POSE_OUT])
    core.find_joints_dev(F, B, p["flag"].data_ptr(), p["R"].data_ptr(), p["t_pose"].data_ptr(), 30, 1e-4, 0.01,
                         *[fj[k].data_ptr() for k in core.JOINTS_OUT])
    core.pose_joints_dev(F, R, d_traj.data_ptr(), bodies, p["flag"].data_ptr(), p["quat"].data_ptr(), p["R"].data_ptr(),
                         p["t_pose"].data_ptr(), joints, jcpu.AXIS_LEN, jcpu.MAX_RMS, jcpu.ROUNDS, *[j[k].data_ptr() for k in core.JOINT_POSE_OUT])
    core.fit_skeleton_dev(F, R, d_traj.data_ptr(), bodies, j["flag"].data_ptr(), j["quat"].data_ptr(), j["t_pose"].data_ptr(), joints,
                          0.1, 1.0, 3, *[o[k].data_ptr() for k in OUT])
    core.synchronize()
    assert_equal({k: v.cpu().numpy() for k, v in o.items()}, ref, "chained")
    assert (ref["steps"] > 0).sum() > 1000


# ---------------------------------------------------------------- 6. refusals
def test_every_refusal_leaves_its_outputs_untouched(core):
    from mocap_core import capi
    from mocap_core.capi import _p
    F = 120
    traj, bodies, joints, pj = cpu.tree(50, F, [-1, 0, 1, 1, 3])
    traj = np.ascontiguousarray(traj)
    R = traj.shape[0]
    flag, quat, t = (np.ascontiguousarray(pj[k]) for k in ("flag", "quat", "t_pose"))

    def call(joints=joints, bodies=bodies, F=F, R=R, axis_len=0.1, w_joint=1.0, iters=8, null=None, J=None):
        Bn, n, rows, q = core._session_bodies(bodies)
        Jn, *arrays = core._joint_pose_arrays(joints)
        o = outputs(max(Bn, 1), max(F, 1), host_fill, SENTINEL)
        ptrs = [_p(traj), _p(n), _p(rows), _p(q), _p(flag), _p(quat), _p(t)] + [_p(a) for a in arrays] + [_p(o[k]) for k in OUT]
        if null is not None:
            ptrs[null] = None
        rc = core.lib.mocap_fit_skeleton(core._h, F, R, ptrs[0], Bn, *ptrs[1:7], Jn if J is None else J, *ptrs[7:14], axis_len, w_joint, iters,
                                         *ptrs[14:])
        assert all((o[k] == SENTINEL).all() for k in OUT)
        return rc

    def with_joint(i, **kw):
        return [dict(j, **kw) if n == i else j for n, j in enumerate(joints)]

    hinge = next(i for i, j in enumerate(joints) if j["kind"] == jp.HINGE)
    bad = [("a cycle", dict(joints=with_joint(3, a=2, b=3))), ("a duplicate pair", dict(joints=with_joint(3, a=1, b=0))),
           ("a FIXED kind", dict(joints=with_joint(0, kind=jr.FIXED))), ("an UNSEEN kind", dict(joints=with_joint(0, kind=jr.UNSEEN))),
           ("a bad axis norm", dict(joints=with_joint(hinge, axis_a=[0.0, 0.0, 1.001]))), ("a NaN axis", dict(joints=with_joint(hinge, axis_b=[NAN, 0.0, 1.0]))),
           ("axis_len 0", dict(axis_len=0.0)), ("axis_len NaN", dict(axis_len=NAN)), ("axis_len inf", dict(axis_len=INF)),
           ("axis_len < 0", dict(axis_len=-0.1)), ("iters 0", dict(iters=0)), ("iters 17", dict(iters=17)), ("iters -1", dict(iters=-1)),
           ("J = B", dict(joints=joints + [dict(joints[0], a=0, b=4)])), ("J = 0", dict(J=0)), ("w_joint 0", dict(w_joint=0.0)),
           ("w_joint NaN", dict(w_joint=NAN)), ("w_joint inf", dict(w_joint=INF)), ("w_joint < 0", dict(w_joint=-1.0)),
           ("a NaN centre", dict(joints=with_joint(1, c_b=[0.0, NAN, 0.0]))), ("a body outside", dict(joints=with_joint(0, b=5))),
           ("a = b", dict(joints=with_joint(0, a=1, b=1))), ("one body", dict(bodies=bodies[:1], joints=joints[:1])),
           ("a row used twice", dict(bodies=bodies[:4] + [bodies[3]])), ("n_frames 0", dict(F=0)), ("R 0", dict(R=0)), ("R too small", dict(R=R - 2))]
    for what, kw in bad:
        assert call(**kw) == capi.MOCAP_E_ARG, what
        assert b"mocap_fit_skeleton" in core.lib.mocap_last_error(core._h), what
    for i in range(22):                                                          # a null buffer, each in turn
        assert call(null=i) == capi.MOCAP_E_ARG, i
    with pytest.raises(capi.MocapError) as e:                                    # the device form refuses before anything is enqueued
        core.fit_skeleton_dev(F, R, 8, bodies, 8, 8, 8, joints, 0.1, 1.0, 17, 8, 8, 8, 8, 8, 8, 8, 8)
    assert e.value.code == capi.MOCAP_E_ARG
    assert capi.SK_MAX_ITERS == 16
    # the edges of what is accepted
    got = core.fit_skeleton(traj, bodies, flag, quat, t, joints, 1e-300, 5e-324, 16)
    assert_equal(got, cpu.fit(traj, bodies, pj, joints, axis_len=1e-300, w_joint=5e-324, iters=16), "edges")


# ---------------------------------------------------------------- 7. the helper on the five-body scene
def test_helper_numpy_resident_and_statement_on_the_scene(core):
    from mocap_core import helpers
    t, traj, bodies, joints, _, _, pj, ref = cpu.scene()
    blist = [{"rows": rows, "markers": q} for rows, q in bodies]
    par = dict(axis_len=cpu.AXIS_LEN, w_joint=cpu.W_JOINT, iters=cpu.ITERS, degree=2, W=8, n_min=5, max_gap=4)
    helpers.set_core(core)
    a = helpers.session_skeleton_fit(t, {"traj": traj}, blist, pj, joints, **par)
    res = {k: to_dev(np.ascontiguousarray(v)) for k, v in pj.items()}
    b = helpers.session_skeleton_fit(to_dev(t), {"traj": to_dev(traj)}, blist, res, {"joints": joints}, **par)
    b = {k: v.cpu().numpy() for k, v in b.items()}
    assert_equal(a, ref, "helper")
    assert set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype, k
    posed = jp.fill_flag(pj["flag"])
    assert np.array_equal(a["flag_posed"], posed) and np.array_equal(a["flag"], pj["flag"]) and np.array_equal(a["hops"], pj["hops"])
    # the smoothers take the fitted tables unchanged; the fill is mocap_fill_rows' over the mapped flag
    tr = core.smooth_tracks(t, ref["t_pose"], 2, 8, INF, 5, 4)
    rot = core.smooth_rotations(t, ref["quat"], 2, 8, INF, 5, 4)
    assert a["pos"].tobytes() == tr["pos"].tobytes() and a["quat_s"].tobytes() == rot["quat_s"].tobytes() and np.array_equal(a["flag_s"], rot["flag"])
    fill = bsr.fill_rows(traj, bodies, posed, ref["R"], ref["t_pose"], rot["flag"], rot["quat_s"], tr["pos"])
    assert np.array_equal(a["src"], fill["src"]) and jp.same_bits(a["filled"], fill["filled"])
    # the joints' series reads the result directly: every joint closes tighter than under the jointed poses
    after = helpers.session_joint_motion(t, {**a, "flag": a["flag_posed"]}, joints[:2])
    before = helpers.session_joint_motion(t, {**pj, "flag": posed}, joints[:2])
    assert np.array_equal(after["present"], before["present"]) and after["present"].sum() > 1000
    on = after["present"] != 0
    assert np.sqrt((after["gap"][on] ** 2).mean()) < 0.5 * np.sqrt((before["gap"][on] ** 2).mean())
