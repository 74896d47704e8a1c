"""GPU: the calibration tail (reference index.py: `determine-scale` :290-309, `acquire-floor` :158-194, `set-origin` :197-210)
over a capture as the frame path leaves it -- mocap_determine_scale(_dev), mocap_floor_factor(_dev) and the three seams of
mocap_core.helpers -- against what the reference's own handlers emitted (tests/golden/calib_tail_session.npz,
scripts/make_calib_tail_golden.py) and against NumPy on the same arrays for every shape at which a reduction changes path.

Gates.  pair_dist: bit for bit (sqrt(((dx*dx + dy*dy) + dz*dz)), NumPy's order for three elements, no fused multiply-add).
scale_factor and the scaled t: 1e-13 relative -- two pairwise-style sums of n <= 1e5 positive terms differ by at most about
2 (ceil(log2 n) + 16) 2^-53 ~ 7e-15.  Factor: R^T R = A^T A to 1e-12 of max |A^T A| against a longdouble product (Givens QR is
backward stable: the error is a small multiple of eps |A|^2).  to_world: 1e-9 absolute (tests/test_calib_tail_cpu.py).  RMS
residual: 1e-9 relative of lstsq's."""
import numpy as np
import pytest
from scipy import linalg

from conftest import load_golden

pytestmark = pytest.mark.gpu

WG = 256      # frames per workgroup (csrc/kernels.hpp kCalibThreads)


# ---------------------------------------------------------------------------------------------------------------- NumPy side
def valid_frames(n_pts, status, K_max):
    ok = (n_pts >= 0) & (n_pts <= K_max)
    return ok if status is None else ok & (status == 0)


def expect_scale(xyz, n_pts, status, actual=0.15):
    ok = valid_frames(n_pts, status, xyz.shape[1])
    pair = ok & (n_pts == 2)
    pd = np.full(len(n_pts), np.nan)
    if xyz.shape[1] >= 2:
        d = xyz[:, 0] - xyz[:, 1]
        with np.errstate(invalid="ignore"):
            pd[pair] = np.sqrt(np.sum(d ** 2, axis=1))[pair]
    mean = np.mean(pd[pair]) if pair.any() else np.nan
    return pd, (actual / mean if pair.any() else np.nan), mean, int(pair.sum()), int((~ok).sum())


def expect_points(xyz, n_pts, status):
    ok = valid_frames(n_pts, status, xyz.shape[1])
    n = np.where(ok, n_pts, 0)
    return xyz[np.arange(xyz.shape[1])[None, :] < n[:, None]]


def check_scale(got, xyz, n_pts, status):
    pd, scale, mean, pairs, skipped = expect_scale(xyz, n_pts, status)
    assert np.array_equal(np.isnan(got["pair_dist"]), np.isnan(pd))
    assert got["pair_dist"][~np.isnan(pd)].tobytes() == pd[~np.isnan(pd)].tobytes()
    assert got["pairs"] == pairs and got["skipped"] == skipped
    if pairs == 0:
        assert np.isnan(got["scale_factor"]) and np.isnan(got["mean_distance"])
    else:
        print(f"scale {abs(got['scale_factor'] - scale) / scale:.2e}  mean {abs(got['mean_distance'] - mean) / mean:.2e} (gate 1e-13)")
        assert abs(got["scale_factor"] - scale) <= 1e-13 * scale
        assert abs(got["mean_distance"] - mean) <= 1e-13 * mean


def check_factor(factor, pts):
    R = factor[:16].reshape(4, 4)
    assert factor[16] == len(pts)
    assert np.array_equal(np.tril(R, -1), np.zeros((4, 4))) and (np.diag(R) >= 0).all()
    A = np.c_[pts[:, 0], pts[:, 1], np.ones(len(pts)), pts[:, 2]].astype(np.longdouble)
    AtA = A.T @ A
    RtR = R.astype(np.longdouble).T @ R.astype(np.longdouble)
    scale = float(np.abs(AtA).max()) if len(pts) else 1.0
    err = float(np.abs(RtR - AtA).max()) / scale if len(pts) else float(np.abs(RtR).max())
    print(f"R^T R - A^T A: {err:.2e} (gate 1e-12), {len(pts)} points")
    assert err <= 1e-12


def make_capture(F, K_max, seed, offset=(2.0, -1.5, 0.7)):
    """Random capture: 0 .. min(K_max, 4) points per frame on a plane tilted by 12 degrees, 2 mm of noise; NaN beyond n_pts."""
    rng = np.random.default_rng(seed)
    n_pts = rng.integers(0, min(K_max, 4) + 1, F).astype(np.int32)
    uv = rng.uniform(-1, 1, (F, K_max, 2))
    xyz = np.concatenate([uv, (0.17 * uv[..., 0] - 0.1277 * uv[..., 1])[..., None]], axis=-1) + offset + rng.normal(0, 0.002, (F, K_max, 3))
    xyz[np.arange(K_max)[None, :] >= n_pts[:, None]] = np.nan
    return xyz, n_pts


# ---------------------------------------------------------------------------------------------------------------- golden
@pytest.fixture(scope="module")
def golden():
    return load_golden("calib_tail_session")


@pytest.mark.parametrize("rec", [0, 1])
def test_scale_matches_the_reference_handler(core, golden, rec):
    g = golden
    xyz, n_pts = g["xyz"][rec], g["n_pts"][rec]
    got = core.determine_scale(xyz, n_pts, None, float(g["actual_distance"][0]), want_pair_dist=True)
    check_scale(got, xyz, n_pts, None)
    ref = float(g["scaled_t"][rec][1, 0])          # pose 1's t starts with exactly 1.0: the handler's scale_factor itself
    print(f"record {rec}: scale_factor {got['scale_factor']!r} vs the reference's {ref!r}: {abs(got['scale_factor'] - ref) / ref:.2e}")
    assert abs(got["scale_factor"] - ref) <= 1e-13 * ref
    assert got["pairs"] == int((n_pts == 2).sum()) and got["skipped"] == 0


@pytest.mark.parametrize("rec", [0, 1])
def test_floor_matches_the_reference_handler(core, golden, rec):
    g = golden
    xyz, n_pts = g["xyz"][rec], g["n_pts"][rec]
    pts = expect_points(xyz, n_pts, None)
    factor = core.floor_factor(xyz, n_pts)
    check_factor(factor, pts)
    W, info, rc = core.floor_from_factor(factor)
    A = np.c_[pts[:, :2], np.ones(len(pts))]
    fit = linalg.lstsq(A, pts[:, 2])[0]
    rms = np.sqrt(np.sum((A @ fit - pts[:, 2]) ** 2) / len(pts))
    err = np.abs(W - g["floor_to_world"][rec]).max()
    print(f"record {rec}: to_world {err:.2e} (gate 1e-9)  rms {abs(info['rms_residual'] - rms) / rms:.2e} (gate 1e-9)")
    assert rc == 0 and err <= 1e-9
    assert abs(info["rms_residual"] - rms) <= 1e-9 * rms
    assert (np.abs(np.array([info["a"], info["b"], info["c"]]) - fit) <= 1e-10 * np.abs(fit)).all()


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("F,K_max", [(63, 8), (64, 8), (65, 8), (WG - 1, 8), (WG, 8), (WG + 1, 8), (70000, 8), (300, 1), (300, 2)])
def test_shapes_where_the_reductions_change_path(core, F, K_max):
    xyz, n_pts = make_capture(F, K_max, seed=F + K_max)
    got = core.determine_scale(xyz, n_pts, None, want_pair_dist=True)
    check_scale(got, xyz, n_pts, None)
    if K_max == 1:
        assert got["pairs"] == 0 and np.isnan(got["scale_factor"])
    else:
        assert got["pairs"] > 0
    check_factor(core.floor_factor(xyz, n_pts), expect_points(xyz, n_pts, None))


@pytest.mark.parametrize("n", [2, 3])
def test_single_frame(core, n):
    xyz = np.array([[[2.0, -1.5, 0.7], [2.25, -1.25, 0.75], [1.5, -1.0, 0.5], [np.nan] * 3]])
    xyz[0, n:] = np.nan
    n_pts = np.array([n], dtype=np.int32)
    got = core.determine_scale(xyz, n_pts, None, want_pair_dist=True)
    check_scale(got, xyz, n_pts, None)
    assert got["pairs"] == (1 if n == 2 else 0)
    check_factor(core.floor_factor(xyz, n_pts), xyz[0, :n])


# ---------------------------------------------------------------------------------------------------------------- valid slots
def test_valid_slot_rule(core):
    F, K_max = 700, 6
    rng = np.random.default_rng(11)
    xyz, n_pts = make_capture(F, K_max, seed=12)
    status = np.zeros(F, dtype=np.int32)
    flagged = rng.choice(F, 60, replace=False)
    status[flagged[:20]] = rng.choice([1, 2, 4, 34, 50], 20)       # flagged frames: real points, not to be used
    n_pts[flagged[20:40]] = rng.integers(K_max + 1, 200, 20)         # frames that need more slots than K_max: nothing was written
    xyz[flagged[20:40]] = np.nan
    n_pts[flagged[40:]] = -rng.integers(1, 5, 20)
    xyz[flagged[40:]] = np.nan
    for st, skipped in ((status, 60), (None, 40)):
        got = core.determine_scale(xyz, n_pts, st, want_pair_dist=True)
        check_scale(got, xyz, n_pts, st)
        assert got["skipped"] == skipped and np.isfinite(got["scale_factor"])
        factor = core.floor_factor(xyz, n_pts, st)
        assert np.isfinite(factor).all()                           # no NaN slot was read
        check_factor(factor, expect_points(xyz, n_pts, st))


# ---------------------------------------------------------------------------------------------------------------- determinism
def _dev_calls(core, xyz, n_pts, status):
    import torch
    dev = torch.device("cuda", 0)
    d_xyz, d_n = torch.from_numpy(xyz).to(dev), torch.from_numpy(n_pts).to(dev)
    d_st = None if status is None else torch.from_numpy(status).to(dev)
    F, K_max = xyz.shape[:2]
    d_pd = torch.zeros(F, dtype=torch.float64, device=dev)
    d_res = torch.zeros(4, dtype=torch.float64, device=dev)
    d_fac = torch.zeros(17, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    core.determine_scale_dev(F, K_max, d_xyz.data_ptr(), d_n.data_ptr(), 0 if d_st is None else d_st.data_ptr(), 0.15,
                             d_pd.data_ptr(), d_res.data_ptr())
    core.floor_factor_dev(F, K_max, d_xyz.data_ptr(), d_n.data_ptr(), 0 if d_st is None else d_st.data_ptr(), d_fac.data_ptr())
    core.synchronize()
    return d_pd.cpu().numpy(), d_res.cpu().numpy(), d_fac.cpu().numpy()


def test_bits_do_not_depend_on_the_call(core):
    import torch
    xyz, n_pts = make_capture(5000, 8, seed=21)
    status = (np.random.default_rng(22).random(5000) < 0.05).astype(np.int32)
    host = core.determine_scale(xyz, n_pts, status, want_pair_dist=True)
    host_res = np.array([host["scale_factor"], host["mean_distance"], host["pairs"], host["skipped"]])
    host_fac = core.floor_factor(xyz, n_pts, status)
    again = core.determine_scale(xyz, n_pts, status, want_pair_dist=True)
    assert again["pair_dist"].tobytes() == host["pair_dist"].tobytes() and again["scale_factor"] == host["scale_factor"]
    assert core.floor_factor(xyz, n_pts, status).tobytes() == host_fac.tobytes()
    pd, res, fac = _dev_calls(core, xyz, n_pts, status)
    assert pd.tobytes() == host["pair_dist"].tobytes() and res.tobytes() == host_res.tobytes() and fac.tobytes() == host_fac.tobytes()
    stream = torch.cuda.Stream(device=0)
    try:
        core.set_stream(stream.cuda_stream)
        pd2, res2, fac2 = _dev_calls(core, xyz, n_pts, status)
    finally:
        core.set_stream(0)
    assert pd2.tobytes() == pd.tobytes() and res2.tobytes() == res.tobytes() and fac2.tobytes() == fac.tobytes()


def test_chained_behind_track_frame_dev(core, golden):
    """A 4-camera synthetic session (two markers 0.4 m apart in some frames, three on a tilted floor in others) through
    mocap_track_frame_dev with a world matrix; its device buffers go straight into the two _dev calls, whose results equal the
    host forms on the copied-back arrays bit for bit."""
    import torch
    from mocap_core import synth
    rig = synth.ring_rig(4)

    def floor(p):
        p = p.copy()
        if p.shape[1] == 2:
            p[:, 1, :2] = p[:, 0, :2] + 0.4 * np.array([0.6, 0.8])
        p[..., 2] = 0.17 * p[..., 0] - 0.1277 * p[..., 1]
        return p

    parts = [synth.make_blob_stream(rig, 150, m, seed=30 + m, dropout=0.0, half_extent=0.5, m_max=3, world=floor)[:2] for m in (2, 3)]
    blobs = np.concatenate([p[0] for p in parts])
    counts = np.concatenate([p[1] for p in parts])
    F, C, M, K = blobs.shape[0], 4, 3, 8
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.set_world_transform(golden["floor_to_world"][0])
    try:
        dev = torch.device("cuda", 0)
        d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
        o = dict(xyz=torch.full((F, K, 3), float("nan"), dtype=torch.float64, device=dev), err=torch.zeros((F, K), dtype=torch.float64, device=dev),
                 corr=torch.zeros((F, K, C), dtype=torch.int16, device=dev), n=torch.zeros(F, dtype=torch.int32, device=dev),
                 st=torch.zeros(F, dtype=torch.int32, device=dev), res=torch.zeros(4, dtype=torch.float64, device=dev),
                 fac=torch.zeros(17, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        core.track_frame_dev(F, M, d_b.data_ptr(), d_c.data_ptr(), 5.0, K, 1 << 20, o["xyz"].data_ptr(), o["err"].data_ptr(),
                             o["corr"].data_ptr(), o["n"].data_ptr(), o["st"].data_ptr())
        core.determine_scale_dev(F, K, o["xyz"].data_ptr(), o["n"].data_ptr(), o["st"].data_ptr(), 0.15, 0, o["res"].data_ptr())
        core.floor_factor_dev(F, K, o["xyz"].data_ptr(), o["n"].data_ptr(), o["st"].data_ptr(), o["fac"].data_ptr())
        core.synchronize()
        h = {k: v.cpu().numpy() for k, v in o.items()}
    finally:
        core.set_world_transform(None)
    assert (h["n"][:150] == 2).sum() > 100 and (h["n"][150:] == 3).sum() > 100 and not h["st"].any()
    host = core.determine_scale(h["xyz"], h["n"], h["st"])
    assert h["res"].tobytes() == np.array([host["scale_factor"], host["mean_distance"], host["pairs"], host["skipped"]]).tobytes()
    assert host["pairs"] > 100 and abs(host["mean_distance"] - 0.4) < 0.02
    assert h["fac"].tobytes() == core.floor_factor(h["xyz"], h["n"], h["st"]).tobytes()
    check_factor(h["fac"], expect_points(h["xyz"], h["n"], h["st"]))


# ---------------------------------------------------------------------------------------------------------------- seam
class Recorder:
    def __init__(self):
        self.events = []

    def emit(self, name, payload):
        self.events.append((name, payload))


def test_seam_emits_the_reference_events(core, golden):
    import torch
    from mocap_core import helpers, synth
    g, rec = golden, 0
    helpers.set_core(core)
    xyz, n_pts = g["xyz"][rec], g["n_pts"][rec]
    object_points = [xyz[f, :n_pts[f]].tolist() for f in range(len(n_pts))]
    poses = lambda: [{"R": g["pose_R"][rec][i].tolist(), "t": g["pose_t"][rec][i].tolist()} for i in range(4)]   # noqa: E731
    sock = Recorder()
    try:
        # determine-scale: the ragged list, the host arrays and the resident tensors give the same bits
        helpers.determine_scale({"objectPoints": object_points, "cameraPoses": poses()}, sock)
        name, payload = sock.events[-1]
        assert name == "camera-pose" and list(payload.keys()) == ["error", "camera_poses"] and payload["error"] is None
        assert all(list(p.keys()) == ["R", "t"] for p in payload["camera_poses"])
        got_t = np.array([p["t"] for p in payload["camera_poses"]])
        assert np.array_equal(np.array([p["R"] for p in payload["camera_poses"]]), g["pose_R"][rec])
        assert (np.abs(got_t - g["scaled_t"][rec]) <= 1e-13 * np.abs(g["scaled_t"][rec])).all()
        dev = torch.device("cuda", 0)
        resident = {"xyz": torch.from_numpy(xyz).to(dev), "n_pts": torch.from_numpy(n_pts).to(dev)}
        for capture in ({"xyz": xyz, "n_out": n_pts, "status": np.zeros(len(n_pts), dtype=np.int32)}, resident):
            helpers.determine_scale({"objectPoints": capture, "cameraPoses": poses()}, sock)
            assert np.array_equal(np.array([p["t"] for p in sock.events[-1][1]["camera_poses"]]), got_t)
        # acquire-floor
        W, info = helpers.acquire_floor({"objectPoints": object_points}, sock)
        name, payload = sock.events[-1]
        assert name == "to-world-coords-matrix" and list(payload.keys()) == ["to_world_coords_matrix"]
        assert np.abs(np.array(payload["to_world_coords_matrix"]) - g["floor_to_world"][rec]).max() <= 1e-9
        assert not info["degenerate"] and info["points"] == n_pts.sum()
        W_res, _ = helpers.acquire_floor({"objectPoints": resident}, sock)
        assert W_res.tobytes() == W.tobytes()
        # ... and a following track_frame returns points in the new world frame
        rig = synth.ring_rig(4)
        blobs, counts, _ = synth.make_blob_stream(rig, 1, 4, seed=41, dropout=0.0)
        helpers.set_camera_params([{"intrinsic_matrix": k.tolist()} for k in rig["K"]])
        pose_dicts = synth.rig_to_pose_dicts(rig)
        _, in_world, _ = helpers.track_frame(synth.frame_to_reference_lists(blobs[0], counts[0]), pose_dicts, is_locating_objects=False)
        helpers.set_to_world_coords_matrix(None)
        _, in_cam0, _ = helpers.track_frame(synth.frame_to_reference_lists(blobs[0], counts[0]), pose_dicts, is_locating_objects=False)
        assert len(in_cam0) >= 3 and in_world.shape == in_cam0.shape
        hom = np.c_[in_cam0 * [-1, -1, 1], np.ones(len(in_cam0))] @ W.T                 # helpers.py:96-103
        want = (hom[:, :3] / hom[:, 3:])[:, [0, 2, 1]]
        assert np.abs(in_world - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        # set-origin
        W2 = helpers.set_origin({"objectPoint": g["origin_point"][rec].tolist(), "toWorldCoordsMatrix": g["floor_to_world"][rec].tolist()}, sock)
        name, payload = sock.events[-1]
        assert name == "to-world-coords-matrix" and list(payload.keys()) == ["to_world_coords_matrix"]
        assert np.array(payload["to_world_coords_matrix"]).tobytes() == g["origin_to_world"][rec].tobytes() == W2.tobytes()
    finally:
        helpers.set_to_world_coords_matrix(None)
