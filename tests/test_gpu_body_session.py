"""Body trajectories on the device (include/mocap_core.h, "body trajectories"; csrc/body_session.hip) against the plain statement of
the contract (tests/body_session_reference.py): integers exactly, every double bit for bit (any NaN equal to any NaN), outputs
pre-filled with a sentinel.  Frame counts around the tiles of 256 and around 65 536 frames = 256 tiles, where a lane of the sign
scans' (and of the good-time scan's) tile pass starts to own two tiles instead of one; body and row counts up to the cap; every rule
of stage 1 at its edge with the parameter taken from the statement's own value; the sign rule through more than a turn, at d = 0
and at w = 0; the smoother's flags, degrees, windows and its n2 rule; every source of stage 3 and the filled table fed back; every
refusal; the host and device forms, call after call, a second stream, behind the gather; and a tracked session end to end."""
import numpy as np
import pytest

import body_session_reference as bs
import rigid_body_reference as rbr
import rigid_groups_reference as rg
import track_smooth_reference as ts

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
SENTINEL = -7
POSE_OUT = ("n_used", "present", "quat", "R", "t_pose", "rms", "flag")
ROT_OUT = ("quat_s", "omega", "res", "n_used", "flag")
POSE_SHAPE = {"n_used": ((), "int32"), "present": ((), "int32"), "flag": ((), "int32"), "quat": ((4,), "float64"),
              "R": ((3, 3), "float64"), "t_pose": ((3,), "float64"), "rms": ((), "float64")}
ROT_SHAPE = {"quat_s": ((4,), "float64"), "omega": ((3,), "float64"), "res": ((), "float64"), "n_used": ((), "int32"),
             "flag": ((), "int32")}
PAR = dict(degree=2, W=8, span=INF, n_min=4, max_gap=8)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _full(shape, dt):
    import torch
    return torch.full(shape, SENTINEL, dtype=getattr(torch, dt), device=_dev())


def _up(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _ptr(x):
    return 0 if x is None else x.data_ptr()


def dev_pose(core, traj, bodies, max_rms=INF):
    import torch
    R, F, _ = traj.shape
    d_traj = _up(traj)
    o = {k: _full((len(bodies), F) + tail, dt) for k, (tail, dt) in POSE_SHAPE.items()}
    torch.cuda.synchronize()
    core.pose_rows_dev(F, R, d_traj.data_ptr(), bodies, max_rms, *[o[k].data_ptr() for k in POSE_OUT])
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def dev_rot(core, t, quat, degree, W, span, n_min, max_gap):
    import torch
    B, F, _ = quat.shape
    d_t, d_q = _up(t), _up(quat)
    o = {k: _full((B, F) + tail, dt) for k, (tail, dt) in ROT_SHAPE.items()}
    torch.cuda.synchronize()
    core.smooth_rotations_dev(F, B, d_t.data_ptr(), d_q.data_ptr(), degree, W, span, n_min, max_gap, *[o[k].data_ptr() for k in ROT_OUT])
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def dev_fill(core, traj, bodies, flag, Rm, t_pose, flag_s=None, quat_s=None, pos_s=None):
    import torch
    R, F, _ = traj.shape
    d = [_up(a) for a in (traj, flag, Rm, t_pose, flag_s, quat_s, pos_s)]
    o = {"filled": _full((R, F, 3), "float64"), "src": _full((R, F), "int32")}
    torch.cuda.synchronize()
    core.fill_rows_dev(F, R, d[0].data_ptr(), bodies, *[_ptr(x) for x in d[1:]], o["filled"].data_ptr(), o["src"].data_ptr())
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def assert_same(got, ref, keys, what):
    for k in keys:
        if ref[k].dtype == np.int32:
            assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5].tolist())
        else:
            assert bs.same_bits(got[k], ref[k]), (what, k, np.argwhere(~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k]))))[:5].tolist())


def session(seed, F, n_markers):
    """Bodies of n_markers[b] markers in body order, then three rows of no body: a loose marker, an all-NaN row and a row of
    +-1e200; 10 % dropout.  With two or more bodies the last body's last marker is a +-1e200 row as well: its fits overflow."""
    t, traj, bodies, truth = bs.make_session(seed, F, n_markers, n_loose=3, dropout=0.10)
    R = traj.shape[0]
    huge = 1e200 * np.where(np.arange(F)[:, None] % 2 == 0, 1.0, -0.5) * np.ones((1, 3))
    traj[R - 1] = huge
    traj[R - 2] = np.nan
    if len(n_markers) >= 2:
        traj[bodies[-1][0][-1]] = np.where(np.arange(F)[:, None] % 3 == 0, huge, np.nan)
    return t, traj, bodies, truth


def all_stages(core, t, traj, bodies, what, max_rms=INF, par=PAR):
    """Each stage on the device against the statement, every stage fed with the statement's own outputs of the stage before."""
    ref = bs.pose_rows(traj, bodies, max_rms)
    assert_same(dev_pose(core, traj, bodies, max_rms), ref, POSE_OUT, (what, "pose"))
    rot = bs.smooth_rotations(t, ref["quat"], **par)
    assert_same(dev_rot(core, t, ref["quat"], **par), rot, ROT_OUT, (what, "rot"))
    tr = ts.smooth(t, ref["t_pose"], **par)
    fill = bs.fill_rows(traj, bodies, ref["flag"], ref["R"], ref["t_pose"], rot["flag"], rot["quat_s"], tr["pos"])
    assert_same(dev_fill(core, traj, bodies, ref["flag"], ref["R"], ref["t_pose"], rot["flag"], rot["quat_s"], tr["pos"]), fill,
                ("filled", "src"), (what, "fill"))
    return ref, rot, tr, fill


# ---------------------------------------------------------------- 1. the device against the statement: frames, bodies, rows
@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 255, 256, 257, 600])
def test_frame_counts_around_the_tiles(core, F):
    t, traj, bodies, _ = session(F, F, (3, 8))
    ref, rot, _, fill = all_stages(core, t, traj, bodies, F)
    if F == 600:
        assert {bs.POSED, bs.FEW} <= set(np.unique(ref["flag"])) and {ts.SMOOTHED, ts.FILLED, 0} <= set(np.unique(rot["flag"]))
        assert set(np.unique(fill["src"])) == {0, 1, 2, 3}


@pytest.mark.parametrize("F", [65536, 65537])
def test_frame_counts_where_a_lane_of_the_tile_scans_owns_two_tiles(core, F):
    """256 tiles: one per lane of the scan over tiles; 257: two for some.  One body of three markers, heavy dropout, so that POSED
    frames lie tiles apart and the previous POSED frame and the parity come through the tile pass."""
    t, traj, bodies, _ = bs.make_session(F, F, (3,), n_loose=0, dropout=0.0)
    rng = np.random.default_rng(F)
    keep = np.zeros(F, dtype=bool)
    keep[rng.choice(F, 900, replace=False)] = True
    keep[[0, 255, 256, F - 1]] = True
    keep[300:600] = True
    traj[0, ~keep] = np.nan
    ref = bs.pose_rows(traj, bodies, INF, raw=True)
    assert (ref["flag"] == bs.POSED).sum() == keep.sum()
    assert (ref["quat"][0, keep, 0] != ref["quat_raw"][0, keep, 0]).any()                   # the rule has flipped some
    assert_same(dev_pose(core, traj, bodies), ref, POSE_OUT, F)
    rot = bs.smooth_rotations(t, ref["quat"], **PAR)
    assert_same(dev_rot(core, t, ref["quat"], **PAR), rot, ROT_OUT, F)


@pytest.mark.parametrize("B,N", [(1, 3), (1, 8), (2, 8), (8, 3), (8, 8), (64, 3)])
def test_body_and_row_counts(core, B, N):
    t, traj, bodies, _ = session(10 * B + N, 300, (N,) * B)
    assert 6 <= traj.shape[0] <= 200
    ref, _, _, _ = all_stages(core, t, traj, bodies, (B, N))
    assert (ref["flag"] == bs.POSED).any()
    if B >= 2:                                                                                 # the overflowing fits are in
        assert not np.isfinite(ref["rms"][-1][ref["present"][-1] >> (N - 1) & 1 == 1]).all() or N == 3


# ---------------------------------------------------------------- 2. stage 1 at the edges of its rules
def test_two_and_three_present_a_body_never_posed_and_posed_frames_tiles_apart(core):
    F = 1400
    t, traj, bodies, _ = bs.make_session(3, F, (4, 3, 5), n_loose=1, dropout=0.0)
    r0 = bodies[0][0]
    traj[r0[0], 100:200] = np.nan                                                              # three present
    traj[r0[1], 150:200] = np.nan                                                              # two present
    traj[bodies[1][0][2]] = np.nan                                                             # never three: never posed
    posed_at = [3, 255, 256, 700, 1300]
    hide = np.ones(F, dtype=bool)
    hide[posed_at] = False
    for r in bodies[2][0][:3]:
        traj[r, hide] = np.nan                                                                 # two present but at five frames
    ref = bs.pose_rows(traj, bodies, INF)
    assert (ref["n_used"][0, 100:150] == 3).all() and (ref["flag"][0, 100:150] == bs.POSED).all()
    assert (ref["n_used"][0, 150:200] == 2).all() and (ref["flag"][0, 150:200] == bs.FEW).all()
    assert (ref["flag"][1] == bs.FEW).all() and np.isnan(ref["quat"][1]).all()
    assert np.flatnonzero(ref["flag"][2] == bs.POSED).tolist() == posed_at
    assert_same(dev_pose(core, traj, bodies), ref, POSE_OUT, "edges")


def _threshold_y():
    """The smallest y at which (0,0,0), (1,0,0), (0.5, y, 0) is a spanning triple, by bisection on the statement's own test."""
    lo, hi = 0.0, 1.0
    while np.nextafter(lo, hi) < hi:
        mid = 0.5 * (lo + hi)
        if rbr.triple_spans([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, mid, 0.0]):
            hi = mid
        else:
            lo = mid
    assert rbr.triple_spans([0, 0, 0], [1.0, 0, 0], [0.5, hi, 0]) and not rbr.triple_spans([0, 0, 0], [1.0, 0, 0], [0.5, lo, 0])
    return lo, hi


def test_present_subset_on_each_side_of_the_posable_threshold(core):
    """Markers 0, 1, 2 nearly in line, at the threshold and one double below it; marker 3 makes the full set posable.  Where marker
    3 is hidden the subset {0, 1, 2} is POSED with the one template and DEGENERATE with the other."""
    below, at = _threshold_y()
    F = 64
    rng = np.random.default_rng(2)
    Rm, c = bs.rigid_motion(rng, np.arange(F) / 120.0)
    for y, want in ((at, bs.POSED), (below, bs.DEGENERATE)):
        q = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, y, 0.0], [0.3, 0.2, 0.4]])
        traj = np.einsum("fij,nj->nfi", Rm, q) + c[None]
        traj[3, 20:40] = np.nan
        bodies = [([0, 1, 2, 3], q)]
        ref = bs.pose_rows(traj, bodies, INF)
        assert (ref["flag"][0, 20:40] == want).all() and (ref["flag"][0, :20] == bs.POSED).all() and (ref["present"][0, 20:40] == 7).all()
        assert_same(dev_pose(core, traj, bodies), ref, POSE_OUT, y)


def test_max_rms_equal_to_a_frames_own_rms_and_one_double_below(core):
    t, traj, bodies, _ = bs.make_session(4, 300, (5, 4), n_loose=0, sigma=0.001, dropout=0.05)
    base = bs.pose_rows(traj, bodies, INF)
    f = 130
    assert base["flag"][0, f] == bs.POSED
    own = float(base["rms"][0, f])
    for max_rms, want in ((own, bs.POSED), (float(np.nextafter(own, 0.0)), bs.RMS)):
        ref = bs.pose_rows(traj, bodies, max_rms)
        assert ref["flag"][0, f] == want and ref["rms"][0, f] == own and np.isnan(ref["quat"][0, f]).all() == (want == bs.RMS)
        assert {bs.POSED, bs.RMS} <= set(np.unique(ref["flag"]))
        assert_same(dev_pose(core, traj, bodies, max_rms), ref, POSE_OUT, max_rms)


# ---------------------------------------------------------------- 3. the sign rule
def _turning(F, q, angles, axis=(0.0, 0.0, 1.0)):
    k = np.asarray(axis) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rm = np.eye(3)[None] + np.sin(angles)[:, None, None] * K + (1 - np.cos(angles))[:, None, None] * (K @ K)
    return np.einsum("fij,nj->nfi", Rm, q)


def test_a_body_turning_through_more_than_a_turn_keeps_one_hemisphere(core):
    F = 700
    q = bs.template(np.random.default_rng(5), 4)
    traj = _turning(F, q, np.linspace(0.0, 5.0 * np.pi, F), axis=(0.2, -0.5, 1.0))
    traj[:, 300:320] = np.nan                                                                  # a gap in the middle of the turn
    bodies = [([0, 1, 2, 3], q)]
    ref = bs.pose_rows(traj, bodies, INF, raw=True)
    p = np.flatnonzero(ref["flag"][0] == bs.POSED)
    d = (ref["quat"][0, p[1:]] * ref["quat"][0, p[:-1]]).sum(axis=1)
    assert (d > 0.9).all() and (ref["quat"][0, p, 0] < -0.9).any() and (ref["quat"][0, p, 0] > 0.9).any()
    assert (np.sign(ref["quat_raw"][0, p, 0]) != np.sign(ref["quat"][0, p, 0])).any()
    assert_same(dev_pose(core, traj, bodies), ref, POSE_OUT, "turn")


def test_a_half_turn_with_d_exactly_zero_does_not_flip_and_a_first_frame_with_w_zero(core):
    """Frames: turned by 170 and 190 degrees about z (the walk arrives in the hemisphere w < 0), the template itself (computed
    (1, 0, 0, 0): d < 0, negated), then the exact half turn (-x, -y, z) (computed (0, 0, 0, 1): d is exactly 0, the sign state
    stays: (0, 0, 0, -1)).  A second body starts on the half turn: w = 0, its first non-zero component decides."""
    q = np.array([[0.25, 0.0, 0.0], [-0.125, 0.25, 0.0], [-0.125, -0.25, 0.125], [0.0, 0.0, -0.125]])
    half = q * np.array([-1.0, -1.0, 1.0])
    lead = _turning(2, q, np.deg2rad([170.0, 190.0]))
    a = np.concatenate([lead, q[:, None], half[:, None], q[:, None]], axis=1)                  # body 0: five frames
    b = np.concatenate([np.full((4, 3, 3), np.nan), half[:, None], q[:, None]], axis=1) + 5.0
    traj = np.concatenate([a, b])
    bodies = [([0, 1, 2, 3], q), ([4, 5, 6, 7], q)]
    ref = bs.pose_rows(traj, bodies, INF, raw=True)
    assert ref["quat_raw"][0, 2].tolist() == [1.0, 0.0, 0.0, 0.0] and ref["quat_raw"][0, 3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert ref["quat"][0, 1, 0] < 0 and ref["quat"][0, 2].tolist() == [-1.0, -0.0, -0.0, -0.0]
    assert ref["quat"][0, 3].tolist() == [-0.0, -0.0, -0.0, -1.0] and ref["quat"][0, 4, 0] == -1.0
    assert ref["flag"][1].tolist() == [bs.FEW] * 3 + [bs.POSED] * 2 and ref["quat"][1, 3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert_same(dev_pose(core, traj, bodies), ref, POSE_OUT, "half turn")


# ---------------------------------------------------------------- 4. the rotation smoother
@pytest.mark.parametrize("degree,W,max_gap", [(1, 1, 0), (1, 1, 1), (2, 8, 0), (2, 8, 8), (3, 32, 0), (3, 32, 32), (2, 32, 5), (1, 32, 32)])
def test_degrees_windows_gaps_bad_time_stamps_and_every_flag(core, degree, W, max_gap):
    F = 600
    t, traj, bodies, _ = bs.make_session(20 + degree, F, (4, 5, 3), n_loose=0, dropout=0.12)
    traj[:4, 200:260] = np.nan                                                                 # body 0 away across a tile edge
    alone = np.zeros(F, dtype=bool)
    alone[380:520] = True
    alone[[420, 450, 480]] = False
    traj[4:9, alone] = np.nan                                                                  # body 1 away but for three lone frames: FEW
    quat = bs.pose_rows(traj, bodies, INF)["quat"]
    t[40], t[41], t[300] = NAN, t[39], t[298]                                                  # not finite, repeated, going back
    t[520] = INF
    par = dict(degree=degree, W=W, span=0.2 if W == 32 else INF, n_min=degree + 1 if W == 1 else degree + 2, max_gap=max_gap)
    ref = bs.smooth_rotations(t, quat, **par)
    want = {0, ts.SMOOTHED, ts.FEW, ts.BAD_TIME} | ({ts.FILLED} if max_gap else set())
    assert want <= set(np.unique(ref["flag"])), np.unique(ref["flag"])
    assert_same(dev_rot(core, t, quat, **par), ref, ROT_OUT, par)
    tr = ts.smooth(t, bs.pose_rows(traj, bodies, INF)["t_pose"], **par)
    assert np.array_equal(tr["flag"], ref["flag"]) and np.array_equal(tr["n_used"], ref["n_used"])


def test_a_failed_pivot_and_the_n2_rule(core):
    """SINGULAR twice over.  A pivot: the first and the last stamp are -1.7e308 and 1.7e308, so in the last frame's window
    s = -inf, h = inf and u = NaN.  n2: q and -q one frame either side of a missing frame at t = 0, 1, 2 cancel in a degree-1
    window: c_0 = 0 exactly, n2 = 0 (the statement says so)."""
    F = 30
    rng = np.random.default_rng(8)
    quat = rng.standard_normal((2, F, 4))
    quat /= np.linalg.norm(quat, axis=2, keepdims=True)
    t = np.arange(F, dtype=np.float64)
    t[0], t[F - 1] = -1.7e308, 1.7e308
    par = dict(degree=2, W=32, span=INF, n_min=4, max_gap=0)
    ref = bs.smooth_rotations(t, quat, **par)
    assert (ref["flag"][:, F - 1] == ts.SINGULAR).all() and (ref["flag"][:, 5] == ts.SMOOTHED).all()
    assert_same(dev_rot(core, t, quat, **par), ref, ROT_OUT, "pivot")
    t = np.arange(F, dtype=np.float64)
    quat[0, 10], quat[0, 11] = NAN, -quat[0, 9]
    quat[1, 11] = NAN
    par = dict(degree=1, W=1, span=INF, n_min=2, max_gap=1)
    ref = bs.smooth_rotations(t, quat, coeffs=True, **par)
    assert ref["flag"][0, 10] == ts.SINGULAR and (ref["c0"][0, 10] == 0.0).all() and np.isnan(ref["quat_s"][0, 10]).all()
    assert ref["flag"][1, 11] == ts.FILLED and ref["n_used"][0, 10] == 2
    assert_same(dev_rot(core, t, quat, **par), ref, ROT_OUT, "n2")


# ---------------------------------------------------------------- 5. stage 3
def test_every_source_with_and_without_the_smoothers_and_the_filled_table_fed_back(core):
    F = 400
    t, traj, bodies, _ = bs.make_session(31, F, (4, 5), n_loose=3, dropout=0.02)
    traj[-2] = np.nan
    traj[bodies[0][0][0], 100:160] = np.nan                                                    # hidden for 60 frames, three others seen
    traj[:4, 300:305] = np.nan                                                                 # the whole body away for five frames
    ref, rot, tr, fill = all_stages(core, t, traj, bodies, "fill")
    r = bodies[0][0][0]
    assert (fill["src"][r, 100:160] == bs.SRC_RIGID).sum() >= 50 and (fill["src"][:4, 300:305] == bs.SRC_RIGID_FILLED).all()
    assert (fill["src"][-3:] <= bs.SRC_MEASURED).all() and (fill["src"][-2] == bs.SRC_NONE).all()                # rows of no body
    without = bs.fill_rows(traj, bodies, ref["flag"], ref["R"], ref["t_pose"])
    assert (without["src"][:4, 300:305] == bs.SRC_NONE).all() and set(np.unique(without["src"])) == {0, 1, 2}
    assert_same(dev_fill(core, traj, bodies, ref["flag"], ref["R"], ref["t_pose"]), without, ("filled", "src"), "no smoothers")
    # the filled table is a table the other stages read
    filled = fill["filled"]
    again = core.smooth_tracks(t, filled, **PAR)
    want = ts.smooth(t, filled, **PAR)
    assert all(ts.same_bits(again[k], want[k]) for k in ts.FIELDS) and np.array_equal(again["flag"], want["flag"])
    groups = core.rigid_groups(filled[:-2], 30, 0.003)
    want = rg.rigid_groups(filled[:-2], 30, 0.003)
    assert np.array_equal(groups["group_of"], want["group_of"]) and rg.same_bits(groups["spread"], want["spread"])
    assert groups["group_of"][:4].tolist() == [0] * 4


# ---------------------------------------------------------------- 6. refusals
def _host(shape_table, lead):
    return {k: np.full(lead + tail, SENTINEL, dtype=dt) for k, (tail, dt) in shape_table.items()}


def test_every_refusal_leaves_its_outputs_untouched(core):
    from mocap_core import capi
    from mocap_core.capi import _p
    F = 40
    t, traj, bodies, _ = bs.make_session(9, F, (3, 4), n_loose=1, dropout=0.0)
    R = traj.shape[0]
    good = bs.pose_rows(traj, bodies, INF)
    lib, h = core.lib, core._h

    def table(bb):
        return core._session_bodies(bb)

    def moved(b, m, row):
        bb = [(list(r), np.array(q)) for r, q in bodies]
        bb[b][0][m] = row
        return bb

    def marker(b, m, value):
        bb = [(list(r), np.array(q)) for r, q in bodies]
        bb[b][1][m] = value
        return bb

    line = [(list(bodies[0][0]), np.array([[0.0, 0, 0], [0.1, 0, 0], [0.3, 0, 0]])), bodies[1]]
    many = [([0, 1, 2], bodies[0][1])] * 65
    bad_bodies = [("a row below 0", moved(0, 1, -1)), ("a row at R", moved(1, 3, R)), ("a row twice in one body", moved(1, 0, bodies[1][0][1])),
                  ("a row shared by two bodies", moved(1, 2, bodies[0][0][0])), ("a NaN coordinate", marker(0, 2, [0.1, NAN, 0.0])),
                  ("an infinite coordinate", marker(1, 0, [INF, 0.0, 0.0])), ("a body that is a line", line), ("B = 65", many),
                  ("B = 0", []), ("two markers", [([0, 1], bodies[0][1][:2]), bodies[1]]),
                  ("nine markers", [(list(range(9)), np.vstack([bodies[1][1]] * 3)[:9] + np.arange(9)[:, None])])]

    def pose(bb, F_=F, R_=R, max_rms=INF, null=None, traj_=traj):
        o = _host(POSE_SHAPE, (max(len(bb), 1), F))
        B, n, rows, q = table(bb)
        ptrs = [None if k == null else _p(o[k]) for k in POSE_OUT]
        rc = lib.mocap_pose_rows(h, F_, R_, _p(traj_), B, _p(n), _p(rows), _p(q), max_rms, *ptrs)
        assert rc == capi.MOCAP_E_ARG and all((v == SENTINEL).all() for v in o.values())
        assert b"mocap_pose_rows" in lib.mocap_last_error(h)

    def fill(bb, F_=F, R_=R, null=None, opt=(None, None, None)):
        o = {"filled": np.full((R, F, 3), float(SENTINEL)), "src": np.full((R, F), SENTINEL, dtype=np.int32)}
        B, n, rows, q = table(bb)
        req = {"traj": traj, "flag": good["flag"], "R": good["R"], "t_pose": good["t_pose"]}
        a = [None if k == null else _p(v) for k, v in req.items()]
        outs = [None if k == null else _p(o[k]) for k in ("filled", "src")]
        rc = lib.mocap_fill_rows(h, F_, R_, a[0], B, _p(n), _p(rows), _p(q), a[1], a[2], a[3], *[_p(x) for x in opt], *outs)
        assert rc == capi.MOCAP_E_ARG and all((v == SENTINEL).all() for v in o.values())
        assert b"mocap_fill_rows" in lib.mocap_last_error(h)

    for what, bb in bad_bodies:
        pose(bb)
        fill(bb)
    for kw in (dict(F_=0), dict(F_=-1), dict(R_=0), dict(R_=capi.TS_MAX_ROWS + 1), dict(F_=2 ** 31 // R + 1)):
        pose(bodies, **kw)
        fill(bodies, **kw)
    for max_rms in (0.0, -1.0, NAN):
        pose(bodies, max_rms=max_rms)
    for k in POSE_OUT:
        pose(bodies, null=k)
    pose(bodies, traj_=None)
    for k in ("traj", "flag", "R", "t_pose", "filled", "src"):
        fill(bodies, null=k)
    rot_ref = bs.smooth_rotations(t, good["quat"], **PAR)
    tr = ts.smooth(t, good["t_pose"], **PAR)
    three = (rot_ref["flag"], rot_ref["quat_s"], tr["pos"])
    for i in range(3):                                                                         # one or two of the three given
        fill(bodies, opt=tuple(None if j == i else three[j] for j in range(3)))
        fill(bodies, opt=tuple(three[j] if j == i else None for j in range(3)))

    def rot(F_=F, B_=2, degree=2, W=8, span=INF, n_min=4, max_gap=0, null=None, t_=t):
        o = _host(ROT_SHAPE, (2, F))
        a = [None if null == "t" else _p(t_), None if null == "quat" else _p(good["quat"])]
        ptrs = [None if k == null else _p(o[k]) for k in ROT_OUT]
        rc = lib.mocap_smooth_rotations(h, F_, B_, *a, degree, W, span, n_min, max_gap, *ptrs)
        assert rc == capi.MOCAP_E_ARG and all((v == SENTINEL).all() for v in o.values())
        assert b"mocap_smooth_rotations" in lib.mocap_last_error(h)

    for kw in (dict(F_=0), dict(B_=0), dict(B_=65), dict(F_=2 ** 31 // 2 + 1), dict(degree=0), dict(degree=4), dict(W=0), dict(W=33),
               dict(span=0.0), dict(span=-1.0), dict(span=NAN), dict(n_min=2), dict(n_min=18), dict(max_gap=-1), dict(max_gap=9),
               dict(t_=np.full(F, NAN))):
        rot(**kw)
    for k in ("t", "quat") + ROT_OUT:
        rot(null=k)
    for call in (lambda: core.pose_rows_dev(F, R, 8, moved(1, 2, bodies[0][0][0]), INF, 8, 8, 8, 8, 8, 8, 8),
                 lambda: core.smooth_rotations_dev(F, 2, 8, 8, 2, 8, INF, 2, 0, 8, 8, 8, 8, 8),
                 lambda: core.fill_rows_dev(F, R, 8, many, 8, 8, 8, 0, 0, 0, 8, 8)):
        with pytest.raises(capi.MocapError) as e:                                              # the device forms refuse before anything is enqueued
            call()
        assert e.value.code == capi.MOCAP_E_ARG
    assert_same(core.pose_rows(traj, bodies), good, POSE_OUT, "after the refusals")


# ---------------------------------------------------------------- 7. forms, repeats, streams, chaining
def test_host_and_device_forms_streams_and_repeated_calls_give_the_same_bytes(core):
    import torch
    t, traj, bodies, _ = session(12, 600, (4, 8, 3))
    ref = bs.pose_rows(traj, bodies, 0.01)
    rot = bs.smooth_rotations(t, ref["quat"], **PAR)
    tr = ts.smooth(t, ref["t_pose"], **PAR)
    fill_in = (traj, bodies, ref["flag"], ref["R"], ref["t_pose"], rot["flag"], rot["quat_s"], tr["pos"])

    def three():
        return (dev_pose(core, traj, bodies, 0.01), dev_rot(core, t, ref["quat"], **PAR), dev_fill(core, *fill_in))

    host = (core.pose_rows(traj, bodies, max_rms=0.01), core.smooth_rotations(t, ref["quat"], **PAR), core.fill_rows(*fill_in))
    one, two = three(), three()
    stream = torch.cuda.Stream(device=0)
    try:
        core.set_stream(stream.cuda_stream)
        other = three()
    finally:
        core.set_stream(0)
    for i, keys in enumerate((POSE_OUT, ROT_OUT, ("filled", "src"))):
        for k in keys:
            assert host[i][k].tobytes() == one[i][k].tobytes() == two[i][k].tobytes() == other[i][k].tobytes(), k
            assert host[i][k].dtype == one[i][k].dtype and host[i][k].shape == one[i][k].shape, k
            assert not (one[i][k] == SENTINEL).any(), k                                        # every byte was written
    assert_same(host[0], ref, POSE_OUT, "host")
    assert_same(host[1], rot, ROT_OUT, "host")
    assert_same(host[2], bs.fill_rows(*fill_in), ("filled", "src"), "host")


def test_chained_behind_the_gather_and_through_all_stages_without_a_synchronise(core):
    import torch
    dev = _dev()
    t, traj, bodies, _ = session(14, 300, (4, 5))
    R, F, _ = traj.shape
    B = len(bodies)
    rng = np.random.default_rng(9)
    K = 16
    xyz, ids, n_pts = np.full((F, K, 3), np.nan), np.full((F, K), -1, dtype=np.int32), np.zeros(F, dtype=np.int32)
    for f in range(F):
        there = rng.permutation(np.flatnonzero(np.isfinite(traj[:, f, 0])))
        xyz[f, :there.size], ids[f, :there.size], n_pts[f] = traj[there, f], there + 3, there.size
    relabel = np.concatenate([[-1, -1, -1], np.arange(R)]).astype(np.int32)
    assert bs.same_bits(ts.gather(xyz, n_pts, ids, relabel, R), traj)
    d = [torch.from_numpy(a).to(dev) for a in (xyz, n_pts, ids, relabel, t)]
    rows = _full((R, F, 3), "float64")
    p = {k: _full((B, F) + tail, dt) for k, (tail, dt) in POSE_SHAPE.items()}
    r = {k: _full((B, F) + tail, dt) for k, (tail, dt) in ROT_SHAPE.items()}
    s = {k: _full((B, F, 3), "float64") for k in ("pos", "vel", "acc")}
    s.update(res=_full((B, F), "float64"), n_used=_full((B, F), "int32"), flag=_full((B, F), "int32"))
    o = {"filled": _full((R, F, 3), "float64"), "src": _full((R, F), "int32")}
    par = (PAR["degree"], PAR["W"], PAR["span"], PAR["n_min"], PAR["max_gap"])
    torch.cuda.synchronize()
    core.gather_tracks_dev(F, K, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 0, relabel.size, d[3].data_ptr(), R, rows.data_ptr())
    core.pose_rows_dev(F, R, rows.data_ptr(), bodies, INF, *[p[k].data_ptr() for k in POSE_OUT])
    core.smooth_tracks_dev(F, B, d[4].data_ptr(), p["t_pose"].data_ptr(), *par, *[s[k].data_ptr() for k in ("pos", "vel", "acc", "res", "n_used", "flag")])
    core.smooth_rotations_dev(F, B, d[4].data_ptr(), p["quat"].data_ptr(), *par, *[r[k].data_ptr() for k in ROT_OUT])
    core.fill_rows_dev(F, R, rows.data_ptr(), bodies, p["flag"].data_ptr(), p["R"].data_ptr(), p["t_pose"].data_ptr(), r["flag"].data_ptr(),
                       r["quat_s"].data_ptr(), s["pos"].data_ptr(), o["filled"].data_ptr(), o["src"].data_ptr())
    core.synchronize()
    ref = bs.pose_rows(traj, bodies, INF)
    rot = bs.smooth_rotations(t, ref["quat"], **PAR)
    tr = ts.smooth(t, ref["t_pose"], **PAR)
    assert_same({k: v.cpu().numpy() for k, v in p.items()}, ref, POSE_OUT, "chained")
    assert_same({k: v.cpu().numpy() for k, v in r.items()}, rot, ROT_OUT, "chained")
    assert np.array_equal(s["flag"].cpu().numpy(), rot["flag"]) and bs.same_bits(s["pos"].cpu().numpy(), tr["pos"])
    fill = bs.fill_rows(traj, bodies, ref["flag"], ref["R"], ref["t_pose"], rot["flag"], rot["quat_s"], tr["pos"])
    assert_same({k: v.cpu().numpy() for k, v in o.items()}, fill, ("filled", "src"), "chained")


# ---------------------------------------------------------------- 8. a tracked session end to end
def test_tracked_session_to_body_trajectories(core):
    """The flight of tests/rigid_groups_reference.py (a 4-marker and a 5-marker body, two loose markers, a static one, every marker
    hidden once for 10 .. 25 frames): track_markers -> session_trajectories(stitch=...) -> find_rigid_groups -> learn_session_bodies
    -> session_body_poses, NumPy and resident, equal to each other and to the statement; a marker hidden for longer than W frames
    while three others of its body are seen has no hole in `filled`, and `src` says RIGID."""
    import torch
    from mocap_core import capi, helpers
    t, xyz, n_pts, slot_of, owner, templates, truth = rg.flight_scene()
    dev = _dev()
    W = 8
    core.set_world_transform(None)
    core.set_marker_tracker(**rg.FLIGHT_TRACKER)
    helpers.set_core(core)
    try:
        mk = core.track_markers(t, xyz, n_pts)
        kw = dict(hits=mk["hits"], degree=2, W=W, n_min=5, max_gap=4, **rg.FLIGHT_TABLE)
        ses = helpers.session_trajectories(t, xyz, n_pts, mk["id"], stitch=rg.FLIGHT_STITCH, **kw)
        res = helpers.session_trajectories(*[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (t, xyz, n_pts, mk["id"])],
                                           stitch=rg.FLIGHT_STITCH, **{**kw, "hits": torch.from_numpy(mk["hits"]).to(dev)})
        groups = helpers.find_rigid_groups(ses, **rg.FLIGHT_GROUPS)
        learned, skipped = helpers.learn_session_bodies({"xyz": xyz, "n_pts": n_pts, "id": mk["id"]}, ses, groups)
        par = dict(max_rms=0.005, degree=2, W=W, n_min=5, max_gap=4)
        got = helpers.session_body_poses(t, ses, learned, **par)
        resident = helpers.session_body_poses(torch.from_numpy(t).to(dev), res, learned, **par)
        no_fill = helpers.session_body_poses(t, ses, learned, fill=False, **par)
        with pytest.raises(ValueError):
            helpers.session_body_poses(t, ses, [{"markers": learned[0]["markers"]}])
    finally:
        core.set_marker_tracker(T_max=0)
    assert skipped == [] and len(learned) == 2 and "filled" not in no_fill and set(no_fill) == set(got) - {"filled", "src"}
    assert all(torch.is_tensor(v) and v.is_cuda for v in resident.values()) and set(resident) == set(got)
    for k, v in got.items():
        assert v.tobytes() == resident[k].cpu().numpy().tobytes(), k
    traj = ses["traj"]
    bodies = [(b["rows"], b["markers"]) for b in learned]
    ref = bs.pose_rows(traj, bodies, 0.005)
    sm = dict(degree=2, W=W, span=INF, n_min=5, max_gap=4)
    rot = bs.smooth_rotations(t, ref["quat"], **sm)
    tr = ts.smooth(t, ref["t_pose"], **sm)
    fill = bs.fill_rows(traj, bodies, ref["flag"], ref["R"], ref["t_pose"], rot["flag"], rot["quat_s"], tr["pos"])
    assert_same(got, ref, POSE_OUT, "flight")
    assert_same({"quat_s": got["quat_s"], "omega": got["omega"], "res": got["res_rot"], "flag": got["flag_s"]}, rot,
                ("quat_s", "omega", "res", "flag"), "flight")
    assert_same(got, tr, ("pos", "vel", "acc"), "flight")
    assert_same(got, fill, ("filled", "src"), "flight")
    # a long occlusion with three others seen: filled rigidly, within a millimetre of where the marker really was
    marker = [[m for m in range(len(owner)) if np.array_equal(np.isfinite(row[:, 0]), slot_of[m] >= 0)][0] for row in traj]
    checked = 0
    for b, (rows, _) in enumerate(bodies):
        for r in rows:
            hidden = np.flatnonzero(~np.isfinite(traj[r, :, 0]))
            others = np.isfinite(traj[[x for x in rows if x != r]][:, hidden, 0]).sum(axis=0)
            if hidden.size > W and (others >= 3).all() and (ref["flag"][b, hidden] == bs.POSED).all():
                assert (got["src"][r, hidden] == capi.BP_SRC_RIGID).all() and np.isfinite(got["filled"][r, hidden]).all()
                # 0.5 mm of noise on three or four markers some 0.1 m apart and on the learned template: the pose puts a marker
                # 0.2 m from their centroid within about a millimetre per axis; the bound is five of those
                assert np.abs(got["filled"][r, hidden] - truth[marker[r], hidden]).max() < 0.005
                checked += 1
    assert checked >= 1
