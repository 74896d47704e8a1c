"""Joints on the device (include/mocap_core.h, "joints"; csrc/joints.hip) against the plain statement of the contract
(tests/joints_reference.py): cnt, kind, accepted, parent and n_joints exactly; lam, sep, centre and axis bit for bit (any NaN equal to
any NaN), at the frame counts where the tree changes path and the body counts around a block of pairs; presence; every decision at its
edge with the parameter taken from the statement's own value; the series; the host and device forms, call after call, a second stream,
behind mocap_pose_rows_dev, the sentinel, the refusals; and both helpers on the planted five-body scene."""
import numpy as np
import pytest

import joints_reference as jr
import test_joints_reference_cpu as cpu

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
OUT = ("cnt", "kind", "accepted", "lam", "sep", "centre", "axis", "parent", "n_joints")
SERIES = ("present", "centre", "gap", "quat_rel", "twist")
SENTINEL = -7


def outputs(B, make, fill):
    """The nine outputs pre-filled with the sentinel; make(shape, dtype name, fill)."""
    o = {k: make((B, B), "int32", fill) for k in ("cnt", "kind", "accepted")}
    o.update({k: make((B, B, 3), "float64", float(fill)) for k in ("lam", "centre", "axis")})
    o.update(sep=make((B, B), "float64", float(fill)), parent=make((B,), "int32", fill), n_joints=make((1,), "int32", fill))
    return o


def series_outputs(J, F, make, fill):
    return {"present": make((J, F), "int32", fill), "centre": make((J, F, 3), "float64", float(fill)), "gap": make((J, F), "float64", float(fill)),
            "quat_rel": make((J, F, 4), "float64", float(fill)), "twist": make((J, F, 2), "float64", float(fill))}


def host_fill(shape, dt, fill):
    return np.full(shape, fill, dtype=dt)


def dev_fill(shape, dt, fill):
    import torch
    return torch.full(shape, fill, dtype=getattr(torch, dt), device=torch.device("cuda", 0))


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def dev_find(core, flag, Rm, t, min_common, tol_rank, max_sep=INF):
    """mocap_find_joints_dev into outputs pre-filled with the sentinel -> host arrays."""
    import torch
    B, F = flag.shape
    d = [to_dev(flag.astype(np.int32)), to_dev(Rm), to_dev(t)]
    o = outputs(B, dev_fill, SENTINEL)
    torch.cuda.synchronize()
    core.find_joints_dev(F, B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), min_common, tol_rank, max_sep, *[o[k].data_ptr() for k in OUT])
    core.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["n_joints"] = int(got["n_joints"][0])
    return got


def dev_series(core, flag, quat, Rm, t, joints):
    import torch
    B, F = flag.shape
    d = [to_dev(flag.astype(np.int32)), to_dev(quat), to_dev(Rm), to_dev(t)]
    o = series_outputs(len(joints), F, dev_fill, SENTINEL)
    torch.cuda.synchronize()
    core.joint_series_dev(F, B, *[x.data_ptr() for x in d], joints, *[o[k].data_ptr() for k in SERIES])
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def assert_equal(got, ref, what):
    for k in jr.INT_OUT:
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5].tolist())
    assert got["n_joints"] == ref["n_joints"], what
    for k in jr.F64_OUT:
        assert jr.same_bits(got[k], ref[k]), (what, k, np.argwhere(~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k]))))[:5].tolist())


def assert_series_equal(got, ref, what):
    assert np.array_equal(got["present"], ref["present"]), what
    for k in jr.SERIES_F64:
        assert jr.same_bits(got[k], ref[k]), (what, k)


# ---------------------------------------------------------------- 1. the device against the statement: frames, bodies
@pytest.mark.parametrize("B", [2, 8])
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 255, 256, 257, 16385])
def test_frame_counts_where_the_tree_changes_path(core, F, B):
    flag, Rm, t = jr.session(F + B, F, B)
    stats = {}
    ref = jr.find_joints(flag, Rm, t, 6, 1e-4, 0.01, stats=stats)
    assert_equal(dev_find(core, flag, Rm, t, 6, 1e-4, 0.01), ref, (F, B))
    assert stats["sweeps"] <= 9
    if F >= 63:
        assert ref["kind"][0, 1] == jr.BALL and ref["accepted"][0, 1]
    if F >= 63 and B == 8:
        assert ref["n_joints"] >= 3 and (ref["kind"][7] == jr.UNSEEN).all() and ref["cnt"][7, 7] == 0
        assert ref["cnt"][6, 6] < ref["cnt"][5, 5] and np.isinf(ref["sep"][5, 6])          # NaN frames left out, 1e200 frames kept


@pytest.mark.parametrize("B", [2, 3, 4, 5, 8, 9, 64])
def test_body_counts_around_a_block_and_at_the_cap(core, B):
    flag, Rm, t = jr.session(100 + B, 257, B)
    stats = {}
    ref = jr.find_joints(flag, Rm, t, 30, 1e-4, 0.01, stats=stats)
    assert_equal(dev_find(core, flag, Rm, t, 30, 1e-4, 0.01), ref, B)
    assert stats["sweeps"] <= 9
    if B >= 8:
        assert set(np.unique(ref["kind"])) >= {jr.UNSEEN, jr.HINGE, jr.BALL} and ref["n_joints"] >= B // 2


# ---------------------------------------------------------------- 2. presence
def test_presence_no_common_frame_and_min_common_at_a_pairs_own_count(core):
    flag, Rm, t = jr.session(21, 300, 4, dropout=0.2)
    flag[3], Rm[3], t[3] = flag[1], Rm[1], t[1]                                  # body 3 was never POSED: give it a pose ...
    flag[3, :150] = jr.FEW
    flag[0, 150:] = jr.FEW                                                       # ... and no frame in common with body 0
    base = jr.find_joints(flag, Rm, t, 6, 1e-4)
    assert base["cnt"][0, 3] == 0 and base["kind"][0, 3] == jr.UNSEEN and np.isnan(base["sep"][0, 3]) and np.isnan(base["lam"][0, 3]).all()
    assert base["cnt"][1, 3] > 30 and base["kind"][1, 3] == jr.FIXED
    assert_equal(dev_find(core, flag, Rm, t, 6, 1e-4), base, "no common frame")
    n = int(base["cnt"][0, 1])
    for min_common, kind in ((n, jr.BALL), (n + 1, jr.UNSEEN)):
        ref = jr.find_joints(flag, Rm, t, min_common, 1e-4)
        assert ref["kind"][0, 1] == kind
        assert_equal(dev_find(core, flag, Rm, t, min_common, 1e-4), ref, min_common)
    # a NaN in every POSED frame of a body: its pairs have no frame; in a single value of one frame: that frame alone is left out
    Rm2 = Rm.copy()
    Rm2[1, :, 2, 2] = np.nan
    t2 = t.copy()
    t2[2, 200, 1] = np.nan
    ref = jr.find_joints(flag, Rm2, t2, 6, 1e-4)
    assert (ref["cnt"][1] == 0).all() and ref["cnt"][2, 2] == base["cnt"][2, 2] - int(flag[2, 200] == jr.POSED)
    assert_equal(dev_find(core, flag, Rm2, t2, 6, 1e-4), ref, "NaN")
    # +-1e200 in POSED frames: finite, so the frames count; the sums overflow and what follows is the statement's
    t3 = t.copy()
    t3[1, ::2, 0], t3[1, 1::2, 0] = 1e200, -1e200
    Rm3 = Rm.copy()
    Rm3[2, :, 0, 0] = Rm3[0, :, 0, 0] = 1e200                                    # Rel_00 of (0, 2) is 1e400: infinite
    ref = jr.find_joints(flag, Rm3, t3, 6, 1e-4)
    assert ref["cnt"][0, 1] == n and ref["kind"][0, 2] == jr.SINGULAR and np.isnan(ref["lam"][0, 2]).all() and not ref["accepted"][0, 2]
    assert_equal(dev_find(core, flag, Rm3, t3, 6, 1e-4), ref, "1e200")


# ---------------------------------------------------------------- 3. decision edges
def test_tol_rank_and_max_sep_taken_from_the_statement(core):
    flag, Rm, t, _ = cpu.scene(3, True, 300)
    base = jr.find_joints(flag, Rm, t, 30, cpu.TOL_RANK, INF)
    assert base["kind"][1, 2] == jr.HINGE
    lam1, lam2, sep = float(base["lam"][1, 2, 0]), float(base["lam"][1, 2, 1]), float(base["sep"][1, 2])
    below = lambda x: float(np.nextafter(x, 0.0))
    for tol, kind in ((lam1, jr.HINGE), (below(lam1), jr.BALL), (lam2, jr.FIXED), (below(lam2), jr.HINGE)):
        ref = jr.find_joints(flag, Rm, t, 30, tol, INF)
        assert ref["kind"][1, 2] == kind, (tol, kind)
        assert_equal(dev_find(core, flag, Rm, t, 30, tol, INF), ref, ("tol_rank", tol))
    for max_sep, acc in ((sep, 1), (below(sep), 0)):
        ref = jr.find_joints(flag, Rm, t, 30, cpu.TOL_RANK, max_sep)
        assert ref["accepted"][1, 2] == acc and ref["parent"][2] == (1 if acc else -1)
        assert_equal(dev_find(core, flag, Rm, t, 30, cpu.TOL_RANK, max_sep), ref, ("max_sep", max_sep))


def test_axis_with_a_zero_first_component_and_the_exact_fixed_pair(core):
    F = 200
    th = 0.5 * np.sin(2 * np.pi * 0.9 * np.arange(F) / 120.0 + 0.3)
    z = np.array([0.0, 0.0, 1.0])
    flip = np.diag([1.0, -1.0, -1.0])
    Rm = np.stack([np.broadcast_to(np.eye(3), (F, 3, 3)), jr.rot_axis(z, th), jr.rot_axis(z, th) @ flip, np.broadcast_to(np.eye(3), (F, 3, 3))])
    Rm = np.where(np.abs(Rm) < 1e-15, 0.0, Rm)                                   # exact zeros and ones outside the rotating block
    c = np.array([[0.1, 0.2, 0.3], [-0.05, 0.1, 0.0], [0.02, -0.1, 0.05], [0.3, 0.0, 0.0]])
    t = np.zeros((4, F, 3))
    for b in (1, 2, 3):
        t[b] = c[0] - np.einsum("fij,j->fi", Rm[b], c[b])
    flag = np.full((4, F), jr.POSED, dtype=np.int32)
    ref = jr.find_joints(flag, Rm, t, 30, 1e-4, 0.01)
    for b in (1, 2):
        assert ref["kind"][0, b] == jr.HINGE and ref["lam"][0, b, 0] == 0.0
        assert ref["axis"][0, b].tolist() == [0.0, 0.0, 1.0] and ref["axis"][b, 0, :2].tolist() == [0.0, 0.0] and abs(ref["axis"][b, 0, 2]) == 1.0
    assert ref["axis"][1, 0, 2] == 1.0 and ref["axis"][2, 0, 2] == -1.0
    # Rel = I in every frame: M is the identity pattern, three eigenvalues exactly 0, FIXED, and a residual from what was kept
    assert ref["kind"][0, 3] == jr.FIXED and ref["lam"][0, 3].tolist() == [0.0, 0.0, 0.0] and np.isfinite(ref["sep"][0, 3]) and not ref["accepted"][0, 3]
    assert np.isnan(ref["axis"][0, 3]).all() and np.isfinite(ref["centre"][0, 3]).all()
    assert_equal(dev_find(core, flag, Rm, t, 30, 1e-4, 0.01), ref, "exact")


# ---------------------------------------------------------------- 4. the series
def series_case(seed=31, F=300):
    flag, Rm, t = jr.session(seed, F, 6, dropout=0.1)
    poses = jr.scene_poses(flag, Rm, t)
    s = 0.5 ** 0.5
    own, _ = jr.first_relative(poses["quat"], flag, 0, 1)
    joints = [dict(a=0, b=1, kind=jr.BALL, c_a=[0.1, 0.0, -0.1], c_b=[0.0, 0.2, 0.0], axis_b=[0.0, 0.0, 0.0], q_ref=[1.0, 0.0, 0.0, 0.0]),
              dict(a=1, b=2, kind=jr.HINGE, c_a=[0.0, 0.1, 0.0], c_b=[0.1, 0.0, 0.0], axis_b=[0.0, 0.6, 0.8], q_ref=[s, 0.0, s, 0.0]),
              dict(a=2, b=1, kind=jr.HINGE, c_a=[0.1, 0.0, 0.0], c_b=[0.0, 0.1, 0.0], axis_b=[1.0, 0.0, 0.0], q_ref=[1.0, 0.0, 0.0, 0.0]),
              dict(a=0, b=1, kind=jr.FIXED, c_a=[0.0, 0.0, 0.0], c_b=[0.0, 0.0, 0.0], axis_b=[0.0, 0.0, 0.0], q_ref=own.tolist()),
              dict(a=3, b=0, kind=jr.UNSEEN, c_a=[1.0, 2.0, 3.0], c_b=[-1.0, 0.0, 1.0], axis_b=[0.0, 0.0, 0.0], q_ref=[0.0, 0.0, 0.0, 1.0]),
              dict(a=2, b=3, kind=jr.SINGULAR, c_a=[0.0, 0.0, 0.0], c_b=[0.0, 0.0, 0.0], axis_b=[0.0, 0.0, 0.0], q_ref=[0.5, -0.5, 0.5, -0.5]),
              dict(a=0, b=5, kind=jr.HINGE, c_a=[0.0, 0.0, 0.0], c_b=[0.0, 0.0, 0.0], axis_b=[0.0, 0.0, 1.0], q_ref=[1.0, 0.0, 0.0, 0.0])]
    return flag, Rm, t, poses["quat"], joints


def test_series_every_kind_both_references_and_absent_frames(core):
    flag, Rm, t, quat, joints = series_case()
    ref = jr.joint_series(flag, quat, Rm, t, joints)
    assert 0 < ref["present"][0].sum() < flag.shape[1] and ref["present"][6].sum() == 0          # body 5 is never POSED
    assert np.isfinite(ref["twist"][1][ref["present"][1] == 1]).all() and np.isnan(ref["twist"][0]).all() and np.isnan(ref["twist"][3]).all()
    f0 = int(np.flatnonzero(ref["present"][3])[0])
    assert np.abs(ref["quat_rel"][3, f0] - [1.0, 0.0, 0.0, 0.0]).max() < 1e-15                       # a frame's own q_ref
    got = dev_series(core, flag, quat, Rm, t, joints)
    assert_series_equal(got, ref, "series")
    for k in SERIES:
        assert not (got[k] == SENTINEL).any(), k
    host = core.joint_series(flag, quat, Rm, t, joints)
    for k in SERIES:
        assert host[k].tobytes() == got[k].tobytes() and host[k].dtype == got[k].dtype, k


def test_series_half_turn_and_a_twist_of_no_length(core):
    """q_a the identity, q_b a half turn about x: quat_rel has w = 0.  Against the axis x the twist is (0, 1): a half turn; against z
    s = 0 as well, m = 0, and the twist is NaN."""
    F = 3
    flag = np.full((2, F), jr.POSED, dtype=np.int32)
    quat = np.zeros((2, F, 4))
    quat[0, :, 0] = 1.0
    quat[1, :, 1] = 1.0
    Rm = np.stack([np.broadcast_to(np.eye(3), (F, 3, 3)), np.broadcast_to(np.diag([1.0, -1.0, -1.0]), (F, 3, 3))])
    t = np.zeros((2, F, 3))
    t[1, :, 0] = 0.5
    unit = [1.0, 0.0, 0.0, 0.0]
    joints = [dict(a=0, b=1, kind=jr.HINGE, c_a=[0.5, 0.0, 0.0], c_b=[0.0, 0.0, 0.0], axis_b=[1.0, 0.0, 0.0], q_ref=unit),
              dict(a=0, b=1, kind=jr.HINGE, c_a=[0.5, 0.0, 0.0], c_b=[0.0, 0.0, 0.0], axis_b=[0.0, 0.0, 1.0], q_ref=unit)]
    ref = jr.joint_series(flag, quat, Rm, t, joints)
    assert ref["quat_rel"][0, 0].tolist() == [0.0, 1.0, 0.0, 0.0] and ref["twist"][0, 0].tolist() == [0.0, 1.0] and np.isnan(ref["twist"][1]).all()
    assert (ref["gap"] == 0.0).all() and ref["centre"][0, 0].tolist() == [0.5, 0.0, 0.0]
    assert_series_equal(dev_series(core, flag, quat, Rm, t, joints), ref, "half turn")


def test_series_tables_go_through_the_smoothers_unchanged(core):
    """centre [J][F][3] is a table mocap_smooth_tracks accepts, quat_rel [J][F][4] one mocap_smooth_rotations accepts: chained on the
    device with no copy in between, and equal to the smoothers' host forms over the statement's series."""
    import torch
    from mocap_core import capi
    flag, Rm, t, quat, joints = series_case()
    joints = joints[:4]
    J, (B, F) = len(joints), flag.shape
    times = 1.0 + np.arange(F) / 120.0
    par = (2, 8, INF, 4, 4)
    d = [to_dev(flag.astype(np.int32)), to_dev(quat), to_dev(Rm), to_dev(t), to_dev(times)]
    o = series_outputs(J, F, dev_fill, SENTINEL)
    sm = {k: dev_fill((J, F, 3), "float64", float(SENTINEL)) for k in ("pos", "vel", "acc", "omega")}
    sm.update(quat_s=dev_fill((J, F, 4), "float64", float(SENTINEL)))
    sm.update({k: dev_fill((J, F), "float64", float(SENTINEL)) for k in ("res", "res_rot")})
    sm.update({k: dev_fill((J, F), "int32", SENTINEL) for k in ("n_tr", "flag_tr", "n_rot", "flag_s")})
    torch.cuda.synchronize()
    core.joint_series_dev(F, B, *[x.data_ptr() for x in d[:4]], joints, *[o[k].data_ptr() for k in SERIES])
    core.smooth_tracks_dev(F, J, d[4].data_ptr(), o["centre"].data_ptr(), *par, *[sm[k].data_ptr() for k in ("pos", "vel", "acc", "res", "n_tr", "flag_tr")])
    core.smooth_rotations_dev(F, J, d[4].data_ptr(), o["quat_rel"].data_ptr(), *par, *[sm[k].data_ptr() for k in ("quat_s", "omega", "res_rot", "n_rot", "flag_s")])
    core.synchronize()
    ref = jr.joint_series(flag, quat, Rm, t, joints)
    tr = core.smooth_tracks(times, ref["centre"], *par)
    rot = core.smooth_rotations(times, ref["quat_rel"], *par)
    assert jr.same_bits(sm["pos"].cpu().numpy(), tr["pos"]) and np.array_equal(sm["flag_tr"].cpu().numpy(), tr["flag"])
    assert jr.same_bits(sm["quat_s"].cpu().numpy(), rot["quat_s"]) and np.array_equal(sm["flag_s"].cpu().numpy(), rot["flag"])
    assert (tr["flag"] == capi.TS_SMOOTHED).sum() > F and (rot["flag"] == capi.TS_SMOOTHED).sum() > F


# ---------------------------------------------------------------- 5. forms
def test_host_and_device_forms_streams_and_repeated_calls_give_the_same_bytes(core):
    import torch
    flag, Rm, t = jr.session(5, 600, 9)
    host = core.find_joints(flag, Rm, t, 30, 1e-4, 0.01)
    one = dev_find(core, flag, Rm, t, 30, 1e-4, 0.01)
    two = dev_find(core, flag, Rm, t, 30, 1e-4, 0.01)
    stream = torch.cuda.Stream(device=0)
    try:
        core.set_stream(stream.cuda_stream)
        other = dev_find(core, flag, Rm, t, 30, 1e-4, 0.01)
    finally:
        core.set_stream(0)
    for k in OUT[:-1]:
        assert host[k].tobytes() == one[k].tobytes() == two[k].tobytes() == other[k].tobytes(), k
        assert host[k].dtype == one[k].dtype and host[k].shape == one[k].shape
        assert not (one[k] == SENTINEL).any(), k
    assert host["n_joints"] == one["n_joints"] == two["n_joints"] == other["n_joints"] != SENTINEL
    assert_equal(host, jr.find_joints(flag, Rm, t, 30, 1e-4, 0.01), "host")


def test_chained_behind_pose_rows_with_no_synchronise(core):
    """mocap_pose_rows_dev -> mocap_find_joints_dev -> mocap_joint_series_dev on the context's stream with nothing in between (the
    joints of the series are the statement's: they are host data)."""
    import torch
    import body_session_reference as bsr
    flag0, Rm0, t0, _ = cpu.scene(4, True, 400)
    rng = np.random.default_rng(8)
    B, F = flag0.shape
    bodies, rows = [], []
    for b in range(B):
        q = bsr.template(rng, 4)
        bodies.append((list(range(len(rows), len(rows) + 4)), q))
        for m in range(4):
            rows.append(np.einsum("fij,j->fi", Rm0[b], q[m]) + t0[b])
    traj = np.array(rows)
    traj[rng.uniform(size=traj.shape[:2]) < 0.1] = np.nan
    R = traj.shape[0]
    poses = bsr.pose_rows(traj, bodies, INF)
    ref = jr.find_joints(poses["flag"], poses["R"], poses["t_pose"], 30, cpu.TOL_RANK, cpu.MAX_SEP)
    assert ref["parent"].tolist() == [-1, 0, 1, 1, -1]
    joints = jr.scene_joints(ref)
    for j in joints:
        j["q_ref"], _ = jr.first_relative(poses["quat"], poses["flag"], j["a"], j["b"])
    ref_series = jr.joint_series(poses["flag"], poses["quat"], poses["R"], poses["t_pose"], joints)
    d_traj = to_dev(traj)
    p = {"quat": dev_fill((B, F, 4), "float64", -7.0), "R": dev_fill((B, F, 9), "float64", -7.0), "t_pose": dev_fill((B, F, 3), "float64", -7.0),
         "rms": dev_fill((B, F), "float64", -7.0)}
    p.update({k: dev_fill((B, F), "int32", SENTINEL) for k in ("n_used", "present", "flag")})
    o = outputs(B, dev_fill, SENTINEL)
    s = series_outputs(len(joints), F, dev_fill, SENTINEL)
    torch.cuda.synchronize()
    core.pose_rows_dev(F, R, d_traj.data_ptr(), bodies, INF, *[p[k].data_ptr() for k in core.POSE_OUT])
    core.find_joints_dev(F, B, p["flag"].data_ptr(), p["R"].data_ptr(), p["t_pose"].data_ptr(), 30, cpu.TOL_RANK, cpu.MAX_SEP, *[o[k].data_ptr() for k in OUT])
    core.joint_series_dev(F, B, p["flag"].data_ptr(), p["quat"].data_ptr(), p["R"].data_ptr(), p["t_pose"].data_ptr(), joints,
                          *[s[k].data_ptr() for k in SERIES])
    core.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["n_joints"] = int(got["n_joints"][0])
    assert_equal(got, ref, "chained")
    assert_series_equal({k: v.cpu().numpy() for k, v in s.items()}, ref_series, "chained series")


def test_every_refusal_leaves_its_outputs_untouched(core):
    from mocap_core import capi
    from mocap_core.capi import _p
    F, B = 120, 3
    flag, Rm, t = jr.session(3, F, B)
    flag = np.ascontiguousarray(flag, dtype=np.int32)
    ok = dict(F=F, B=B, n=30, tol=1e-4, sep=INF)
    bad = [("F 0", dict(F=0)), ("F above the cap", dict(F=capi.RG_MAX_FRAMES + 1)), ("B 1", dict(B=1)), ("B 65", dict(B=65)),
           ("min_common 5", dict(n=5)), ("tol_rank 0", dict(tol=0.0)), ("tol_rank < 0", dict(tol=-1e-4)), ("tol_rank 1", dict(tol=1.0)),
           ("tol_rank inf", dict(tol=INF)), ("tol_rank NaN", dict(tol=NAN)), ("max_sep 0", dict(sep=0.0)), ("max_sep < 0", dict(sep=-1.0)),
           ("max_sep NaN", dict(sep=NAN))]
    for what, kw in bad:
        a, o = {**ok, **kw}, outputs(B, host_fill, SENTINEL)
        rc = core.lib.mocap_find_joints(core._h, a["F"], a["B"], _p(flag), _p(Rm), _p(t), a["n"], a["tol"], a["sep"], *[_p(o[k]) for k in OUT])
        assert rc == capi.MOCAP_E_ARG, (what, rc)
        assert all((o[k] == SENTINEL).all() for k in OUT), what
        assert b"mocap_find_joints" in core.lib.mocap_last_error(core._h), what
    o = outputs(B, host_fill, SENTINEL)
    ptrs = [_p(flag), _p(Rm), _p(t), 30, 1e-4, INF] + [_p(o[k]) for k in OUT]
    for i in (0, 1, 2, *range(6, len(ptrs))):                                    # a null buffer, each in turn
        args = ptrs[:i] + [None] + ptrs[i + 1:]
        assert core.lib.mocap_find_joints(core._h, F, B, *args) == capi.MOCAP_E_ARG, i
    assert all((o[k] == SENTINEL).all() for k in OUT)
    with pytest.raises(capi.MocapError) as e:                                    # the device form refuses before anything is enqueued
        core.find_joints_dev(F, B, 8, 8, 8, 5, 1e-4, INF, 8, 8, 8, 8, 8, 8, 8, 8, 8)
    assert e.value.code == capi.MOCAP_E_ARG
    # the series: one refusal per rule of the joint table, and the buffers
    quat = jr.scene_poses(flag, Rm, t)["quat"]
    good = dict(a=0, b=1, kind=jr.HINGE, c_a=[0.1, 0.0, 0.0], c_b=[0.0, 0.1, 0.0], axis_b=[0.0, 0.0, 1.0], q_ref=[1.0, 0.0, 0.0, 0.0])
    bad = [("no joints", []), ("65 joints", [good] * 65), ("a outside", [{**good, "a": 3}]), ("b outside", [good, {**good, "b": -1}]),
           ("a = b", [{**good, "a": 1}]), ("kind", [{**good, "kind": 5}]), ("c_a NaN", [{**good, "c_a": [0.0, NAN, 0.0]}]),
           ("c_b inf", [{**good, "c_b": [0.0, 0.0, INF]}]), ("axis NaN", [{**good, "axis_b": [NAN, 0.0, 1.0]}]),
           ("q_ref NaN", [{**good, "q_ref": [NAN, 0.0, 0.0, 0.0]}]), ("q_ref no unit", [{**good, "q_ref": [1.0, 0.1, 0.0, 0.0]}])]
    for what, joints in bad:
        J, *arrays = core._joint_arrays(joints)
        if what == "axis NaN":
            arrays[5][0, 0] = NAN                                                # (_joint_arrays passes a hinge's axis through)
        o = series_outputs(max(J, 1), F, host_fill, SENTINEL)
        rc = core.lib.mocap_joint_series(core._h, F, B, _p(flag), _p(quat), _p(Rm), _p(t), J, *[_p(x) for x in arrays], *[_p(o[k]) for k in SERIES])
        assert rc == capi.MOCAP_E_ARG, (what, rc)
        assert all((o[k] == SENTINEL).all() for k in SERIES), what
        assert b"mocap_joint_series" in core.lib.mocap_last_error(core._h), what
    J, *arrays = core._joint_arrays([good])
    o = series_outputs(1, F, host_fill, SENTINEL)
    ptrs = [_p(flag), _p(quat), _p(Rm), _p(t), J] + [_p(x) for x in arrays] + [_p(o[k]) for k in SERIES]
    for i in (0, 1, 2, 3, *range(5, len(ptrs))):
        args = ptrs[:i] + [None] + ptrs[i + 1:]
        assert core.lib.mocap_joint_series(core._h, F, B, *args) == capi.MOCAP_E_ARG, i
    for Fb, Bb in ((0, B), (capi.RG_MAX_FRAMES + 1, B), (F, 1), (F, 65)):
        assert core.lib.mocap_joint_series(core._h, Fb, Bb, *ptrs) == capi.MOCAP_E_ARG
    assert all((o[k] == SENTINEL).all() for k in SERIES)
    # the edges of what is accepted
    assert_equal(core.find_joints(flag, Rm, t, 6, 1e-300, 1e-300), jr.find_joints(flag, Rm, t, 6, 1e-300, 1e-300), "edges")
    near_one = float(np.nextafter(1.0, 0.0))
    assert_equal(core.find_joints(flag, Rm, t, F, near_one, INF), jr.find_joints(flag, Rm, t, F, near_one, INF), "edges")


# ---------------------------------------------------------------- 6. the helpers on the planted scene
@pytest.mark.parametrize("noisy", [False, True])
def test_helpers_numpy_resident_and_statement_on_the_five_body_scene(core, noisy):
    import torch
    from mocap_core import helpers
    flag, Rm, t, truth = cpu.scene(3, noisy)
    F = flag.shape[1]
    times = 2.0 + np.arange(F) / 120.0
    poses = jr.scene_poses(flag, Rm, t)
    resident = {k: to_dev(v) for k, v in poses.items()}
    kw = dict(min_common=cpu.MIN_COMMON, tol_rank=cpu.TOL_RANK, max_sep=cpu.MAX_SEP)
    helpers.set_core(core)
    found = helpers.session_joints(poses, **kw)
    found_res = helpers.session_joints(resident, **kw)
    motion = helpers.session_joint_motion(times, poses, found, degree=2, W=8, n_min=5, max_gap=4)
    motion_res = helpers.session_joint_motion(to_dev(times), resident, found_res["joints"], degree=2, W=8, n_min=5, max_gap=4)
    ref = jr.find_joints(flag, Rm, t, cpu.MIN_COMMON, cpu.TOL_RANK, cpu.MAX_SEP)
    for got in (found, found_res):
        assert_equal(got["pairs"], ref, "helper")
        assert got["parent"].tolist() == [-1, 0, 1, 1, -1]
        assert [(j["a"], j["b"], j["kind"], j["frames"]) for j in got["joints"]] == [(0, 1, jr.BALL, F), (1, 2, jr.HINGE, F), (1, 3, jr.BALL, F)]
    for a, b in zip(found["joints"], found_res["joints"]):
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("centre_a", "centre_b", "axis_a", "axis_b", "sep"))
    # against the planted truth, at the CPU file's bounds
    fig = cpu.scene_figures(ref, truth)
    bound = cpu.NOISY if noisy else cpu.CLEAN
    assert all(fig[k] <= bound[k] for k in fig), (fig, bound)
    joints = jr.scene_joints(ref)
    for j in joints:
        j["q_ref"], f0 = jr.first_relative(poses["quat"], flag, j["a"], j["b"])
    assert jr.same_bits(motion["q_ref"], np.array([j["q_ref"] for j in joints]))
    series = jr.joint_series(flag, poses["quat"], Rm, t, joints)
    assert_series_equal(motion, series, "helper series")
    assert_series_equal({k: motion_res[k].cpu().numpy() for k in SERIES}, series, "resident series")
    for k in ("pos", "vel", "acc", "quat_s", "omega", "flag_s"):
        assert motion[k].tobytes() == motion_res[k].cpu().numpy().tobytes(), k
    want = jr.unwrapped_angle(series["twist"], series["present"])
    for angle in (motion["angle"], motion_res["angle"].cpu().numpy()):
        assert np.isnan(angle[0]).all() and np.isnan(angle[2]).all()
        assert np.abs(angle[1] - want[1]).max() <= 1e-12                          # arctan2 and the unwrapping: libm's, torch's
    err = cpu.hinge_angle_error({**series, "twist": motion["twist"]}, joints, truth, f0)
    bound = cpu.ANGLE_NOISY if noisy else cpu.ANGLE_CLEAN
    assert np.abs(err).max() <= bound["max"] and np.sqrt((err ** 2).mean()) <= bound["rms"]
    # the ball joint's centre is where body 0 carries the planted one; every frame was smoothed
    planted = np.einsum("fij,j->fi", Rm[0], truth["ball_a"]) + t[0]
    assert np.abs(motion["centre"][0] - planted).max() <= (1e-12 if not noisy else cpu.MAX_SEP)
    assert (motion["flag_s"] == 1).all() and np.isfinite(motion["pos"]).all() and np.isfinite(motion["quat_s"]).all()
