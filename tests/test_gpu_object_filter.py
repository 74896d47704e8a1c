"""GPU: the object filter (`filtered_objects`, reference helpers.py:109 -> KalmanFilter.py / LowPassFilter.py):
mocap_filter_objects / mocap_track_frame_filtered / helpers.KalmanFilter against what the reference's own two modules returned
for a 700-frame two-drone session (tests/golden/objfilter_two_drones.npz, scripts/make_objfilter_golden.py), against a NumPy
restatement for the quirks, against itself for any cut of a session into calls, and against the staged calls for the fused path.

Tolerances.  `d` = the largest difference between the reference run with a float32 cv.KalmanFilter (what it is) and with a
float64 one, per output: the scale at which float32 rounding moves this recurrence.  Another order of float32 operations is an
independent rounding path through the same contracting filter, hence 4 d for "pos" and "vel"; the low-passed velocities are
rounded to float32 once more (one ulp on top).  The heading never passes through float32: 300 terms x 1.1e-16 x sum|h| is
about 1e-13 relative, asserted at 1e-12.  The golden session's d comes from the fixture; every quirk case computes its own d
from the restatement below at both precisions, the way the fixture's was made."""
import json

import numpy as np
import pytest
from scipy.signal import butter, lfilter

from conftest import load_golden

pytestmark = pytest.mark.gpu

D = 2
B_LP, A_LP = butter(5, 20 / (60.0 / 2), btype="low")


# ---------------------------------------------------------------------------------------------------------------- restatement
def restate(t, pos, heading, drone, n_obj, dtype, resets=None, num_objects=D, buffer_size=300):
    """predict_location frame by frame as KalmanFilter.py:50-100 does it, cv.KalmanFilter(9, 6) at `dtype`:
    -> chosen [F][D], fpos [F][D][3], fvel [F][D][3], fheading [F][D] (float64 arrays; NaN / -1 = drone absent).
    resets: {frame: now} -- reset() called before that frame."""
    F = len(t)
    O_max = pos.shape[1]
    A = np.eye(9, dtype=dtype)
    H = np.eye(6, 9, dtype=dtype)
    Q = np.eye(9, dtype=dtype) * dtype(1e-2)
    R = np.eye(6, dtype=dtype)
    post = [np.zeros((9, 1), dtype=dtype) for _ in range(num_objects)]
    cov = [np.zeros((9, 9), dtype=dtype) for _ in range(num_objects)]
    prev_pos = [np.zeros(3, dtype=np.float32) for _ in range(num_objects)]
    buf = [np.empty((0, 4)) for _ in range(num_objects)]     # heading | vel x, y | vel z: appended together, one window
    prev_time = 0.0
    chosen = np.full((F, num_objects), -1, dtype=np.int32)
    fpos, fvel, fhead = (np.full(s, np.nan) for s in ((F, num_objects, 3), (F, num_objects, 3), (F, num_objects)))
    for f in range(F):
        if resets and f in resets:
            prev_time = resets[f] - 20
            for d in range(num_objects):
                post[d] = np.zeros((9, 1), dtype=dtype)
                prev_pos[d] = np.zeros(3, dtype=np.float32)
        dt = t[f] - prev_time
        prev_time = t[f]
        n = min(int(n_obj[f]), O_max)
        for d in range(num_objects):
            cand = [j for j in range(n) if drone[f, j] == d]
            if not cand:
                continue
            A[:3, 3:6] = dt * np.eye(3)
            A[3:6, 6:9] = dt * np.eye(3)
            A[:3, 6:9] = 0.5 * dt ** 2 * np.eye(3)
            if np.all(post[d] == 0):
                post[d][0:3, 0] = pos[f, cand[0]]
            pre = A @ post[d]
            cov_pre = (A @ cov[d]) @ A.T + Q
            dist = np.sqrt(np.sum((pos[f, cand] - pre[:3, 0]) ** 2, axis=1))
            j = cand[int(np.argmin(dist))]
            new_pos = pos[f, j].astype(np.float32)
            new_vel = ((new_pos - prev_pos[d]) / np.float32(dt)).astype(np.float32)
            prev_pos[d] = new_pos
            z = np.concatenate((new_pos, new_vel)).astype(dtype).reshape(6, 1)
            t2 = H @ cov_pre
            gain = np.linalg.solve(t2 @ H.T + R, t2).astype(dtype).T
            post[d] = pre + gain @ (z - H @ pre)
            cov[d] = cov_pre - gain @ t2
            buf[d] = np.vstack((buf[d], [[heading[f, j], pre[3, 0], pre[4, 0], pre[5, 0]]]))
            low = lfilter(B_LP, A_LP, buf[d], axis=0)[-1]
            if buf[d].shape[0] >= buffer_size:
                buf[d] = buf[d][(-buffer_size) // 2:]
            chosen[f, d] = j
            fpos[f, d] = pre[:3, 0]
            fvel[f, d] = low[1:4].astype(dtype)
            fhead[f, d] = low[0]
    return chosen, fpos, fvel, fhead


def check(got, want, d_pos, d_vel, heading_scale):
    """got: the core's outputs; want: (chosen, fpos, fvel, fheading) of the float32 reference."""
    chosen, fpos, fvel, fhead = want
    assert np.array_equal(got["chosen"], chosen)
    have = chosen >= 0
    assert np.isnan(got["fpos"][~have]).all() and np.isnan(got["fvel"][~have]).all() and np.isnan(got["fheading"][~have]).all()
    e_pos = np.abs(got["fpos"][have].astype(np.float64) - fpos[have]).max()
    e_vel = np.abs(got["fvel"][have].astype(np.float64) - fvel[have])
    e_head = np.abs(got["fheading"][have] - fhead[have]).max()
    ulp = float(np.spacing(np.float32(np.abs(fvel[have][:, :2]).max())))
    print(f"fpos {e_pos:.3e} (4d = {4 * d_pos:.3e})  fvel xy {e_vel[:, :2].max():.3e} z {e_vel[:, 2].max():.3e} (4d = {4 * d_vel:.3e}, "
          f"ulp {ulp:.1e})  fheading {e_head:.3e} (bound {1e-12 * heading_scale:.1e})")
    assert e_pos <= 4 * d_pos
    assert e_vel[:, 2].max() <= 4 * d_vel
    assert e_vel[:, :2].max() <= 4 * d_vel + ulp
    assert e_head <= 1e-12 * heading_scale


def run_calls(core, g, chunk, resets=None):
    """The session in calls of `chunk` frames (a reset cuts a call short), on a fresh filter."""
    core.set_object_filter(D)
    F = len(g["t"])
    cuts = sorted(set(range(0, F, chunk)) | set(resets or ()) | {F})
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if resets and lo in resets:
            core.reset_object_filter(resets[lo])
        parts.append(core.filter_objects(g["t"][lo:hi], g["pos"][lo:hi], g["heading"][lo:hi], g["drone"][lo:hi], g["n_obj"][lo:hi]))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


@pytest.fixture(scope="module")
def session(core):
    g = load_golden("objfilter_two_drones")
    resets = {int(g["reset_frame"][0]): float(g["reset_t"][0])}
    return g, resets, run_calls(core, g, len(g["t"]), resets)      # the whole session: one call up to the reset, one after


# ---------------------------------------------------------------------------------------------------------------- golden
def test_session_matches_the_reference_modules(session):
    g, _, got = session
    assert got["fpos"].dtype == np.float32 and got["fvel"].dtype == np.float32 and got["fheading"].dtype == np.float64
    check(got, (g["chosen"], g["fpos"], g["fvel"], g["fheading"]), float(g["d"][1]), float(g["d"][2]),
          max(1.0, float(np.abs(g["heading"]).max())))


@pytest.mark.parametrize("chunk", [1, 7, 64, 299])
def test_any_cut_into_calls_is_bit_identical(core, session, chunk):
    """State carry and the hand-over of the low-pass history between calls."""
    g, resets, whole = session
    got = run_calls(core, g, chunk, resets)
    for k in ("chosen", "fpos", "fvel", "fheading"):
        assert got[k].tobytes() == whole[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------------------- quirks
def _two_drone_frames(F, O_max=3, seed=3, t0=1.7e9):
    """A short session: drone 0 on a unit circle, drone 1 on a slower one, each with a decoy 0.3 m away listed after it."""
    rng = np.random.default_rng(seed)
    t = t0 + np.cumsum(rng.uniform(0.013, 0.021, F))
    s = t - t[0]
    pos = np.zeros((F, O_max, 3))
    heading = np.zeros((F, O_max))
    drone = np.full((F, O_max), -1, dtype=np.int32)
    pos[:, 0] = np.stack([np.cos(0.8 * s), np.sin(0.8 * s), 1.0 + 0.2 * np.sin(0.5 * s)], axis=1)
    pos[:, 1] = np.stack([-0.5 + 0.5 * np.sin(0.5 * s), 0.4 * np.cos(0.7 * s), 0.8 + 0.0 * s], axis=1)
    pos[:, 2] = pos[:, 0] + np.array([0.0, 0.0, 0.3])
    pos += rng.normal(0.0, 1e-3, pos.shape)
    heading[:, 0], heading[:, 1], heading[:, 2] = 0.9 * np.sin(0.4 * s), 0.7 * np.cos(0.3 * s), 0.2
    drone[:, 0], drone[:, 1], drone[:, 2] = 0, 1, 0
    return {"t": t, "pos": pos, "heading": heading, "drone": drone, "n_obj": np.full(F, 3, dtype=np.int32)}


def _case(name):
    resets = None
    if name == "first_call_at_1p7e9":          # the first dt is `now` itself: harmless, the covariance is still zero
        g = _two_drone_frames(60)
    elif name == "zero_state_reinitialises":   # a candidate at exactly (0, 0, 0) leaves statePost all zero: the NEXT frame
        g = _two_drone_frames(60)              # takes "not initialised" again and starts from ITS candidate 0 (the decoy here)
        g["pos"][0, 0] = 0.0
        g["n_obj"][0] = 1
        g["pos"][1, [0, 2]] = g["pos"][1, [2, 0]]
    elif name == "absent_for_40_frames":       # no predict, no output, state untouched -- then one long dt
        g = _two_drone_frames(100)
        g["drone"][30:70, 1] = 5               # (an index nobody filters: the object is there, the drone is not)
    elif name == "reset_keeps_covariance_and_buffers":
        g = _two_drone_frames(80)
        resets = {40: float(0.5 * (g["t"][39] + g["t"][40]))}
    elif name == "more_objects_than_slots":    # the locator counts what it had no slot for: n_obj > O_max means O_max
        g = _two_drone_frames(60)
        g["n_obj"][::3] = 7
    return g, resets


@pytest.mark.parametrize("name", ["first_call_at_1p7e9", "zero_state_reinitialises", "absent_for_40_frames",
                                  "reset_keeps_covariance_and_buffers", "more_objects_than_slots"])
def test_quirk(core, name):
    g, resets = _case(name)
    args = (g["t"], g["pos"], g["heading"], g["drone"], g["n_obj"])
    want = restate(*args, np.float32, resets)
    w64 = restate(*args, np.float64, resets)
    assert np.array_equal(want[0], w64[0])
    have = want[0] >= 0
    if name == "absent_for_40_frames":
        assert not have[30:70, 1].any() and have[70:, 1].all()
    if name == "zero_state_reinitialises":
        assert want[0][1, 0] == 0 and np.abs(want[1][1, 0] - g["pos"][1, 0]).max() < 1e-6   # frame 1 starts from its first candidate
    got = run_calls(core, g, len(g["t"]), resets)
    check(got, want, np.abs(want[1] - w64[1])[have].max(), np.abs(want[2] - w64[2])[have].max(),
          max(1.0, float(np.abs(g["heading"]).max())))


# ---------------------------------------------------------------------------------------------------------------- fused path
def test_track_frame_filtered_equals_the_staged_calls_bitwise(core):
    g = load_golden("track_apptsx_chain")
    core.set_cameras(g["K"], g["R"], g["t"])
    core.set_world_transform(g["to_world"])
    try:
        frames = np.argsort(-g["ref_nobj"], kind="stable")[:8]          # the 8 frames with the most objects, one time stamp each
        assert g["ref_nobj"][frames].min() > 0
        stamps = 1.7e9 + np.arange(1, 9) / 60.0
        core.set_object_filter(D)
        fused = [core.track_frame_filtered(g["blobs"][f:f + 1], g["counts"][f:f + 1], [now], K_max=48, O_max=8)
                 for f, now in zip(frames, stamps)]
        core.set_object_filter(D)
        n_filtered = 0
        for (f, now), one in zip(zip(frames, stamps), fused):
            plain = core.track_frame(g["blobs"][f:f + 1], g["counts"][f:f + 1], K_max=48, O_max=8)
            for k in plain:
                assert one[k].tobytes() == plain[k].tobytes(), k
            staged = core.filter_objects([now], plain["pos"], plain["heading"], plain["droneIndex"], plain["n_obj"])
            for k in staged:
                assert one[k].tobytes() == staged[k].tobytes(), k
            n_filtered += int((staged["chosen"] >= 0).sum())
        assert n_filtered >= 8
    finally:
        core.set_world_transform(None)


def test_helpers_kalman_filter_has_the_reference_seam(core):
    from mocap_core import helpers, synth
    g = load_golden("track_apptsx_chain")
    helpers.set_core(core)
    helpers.set_camera_params([{"intrinsic_matrix": g["K"][i].tolist()} for i in range(4)])
    helpers.set_to_world_coords_matrix(g["to_world"])
    try:
        poses = [{"R": g["R"][i].tolist(), "t": g["t"][i].tolist()} for i in range(4)]
        f = int(np.argmax(g["ref_nobj"]))
        kf = helpers.KalmanFilter(D)
        assert kf.num_objects == D
        ip = synth.frame_to_reference_lists(g["blobs"][f], g["counts"][f], as_int=True)
        errors, object_points, objects = helpers.track_frame(ip, poses)
        filtered = kf.predict_location(objects, now=1.7e9)
        assert filtered and [o["droneIndex"] for o in filtered] == sorted({o["droneIndex"] for o in objects if o["droneIndex"] < D})
        for o in filtered:
            assert list(o) == ["pos", "vel", "heading", "droneIndex"]
            assert isinstance(o["pos"], np.ndarray) and o["pos"].dtype == np.float32 and o["pos"].shape == (3,)
            assert isinstance(o["vel"], np.ndarray) and o["vel"].dtype == np.float32 and o["vel"].shape == (3,)
            assert isinstance(o["heading"], float) and isinstance(o["droneIndex"], int)
        payload = helpers.object_points_payload(errors, object_points, objects, filtered)
        json.dumps(payload)
        assert payload["filtered_objects"][0]["pos"] == filtered[0]["pos"].tolist()
        assert kf.predict_location([], now=1.7e9 + 0.02) == []
        # the same frame through the one-call form, on a fresh filter: the same four values
        kf.reset(now=1.7e9 + 1.0)
        kf = helpers.KalmanFilter(D)
        ip = synth.frame_to_reference_lists(g["blobs"][f], g["counts"][f], as_int=True)
        e2, p2, o2, f2 = helpers.track_frame_filtered(ip, poses, now=1.7e9)
        assert np.array_equal(e2, errors) and np.array_equal(p2, object_points) and len(o2) == len(objects)
        assert len(f2) == len(filtered)
        for x, y in zip(f2, filtered):
            assert x["droneIndex"] == y["droneIndex"] and x["heading"] == y["heading"]
            assert np.array_equal(x["pos"], y["pos"]) and np.array_equal(x["vel"], y["vel"])
    finally:
        helpers.set_to_world_coords_matrix(None)


# ---------------------------------------------------------------------------------------------------------------- errors
def test_errors(core):
    from mocap_core import capi
    g = _two_drone_frames(4)
    args = (g["t"], g["pos"], g["heading"], g["drone"], g["n_obj"])
    core.set_object_filter(0)                                     # off = as before mocap_set_object_filter
    with pytest.raises(capi.MocapError, match="mocap_set_object_filter has not been called") as e:
        core.filter_objects(*args)
    assert e.value.code == capi.MOCAP_E_ARG
    with pytest.raises(capi.MocapError) as e:
        core.reset_object_filter(1.0)
    assert e.value.code == capi.MOCAP_E_ARG
    chain = load_golden("track_apptsx_chain")
    core.set_cameras(chain["K"], chain["R"], chain["t"])
    with pytest.raises(capi.MocapError, match="mocap_set_object_filter has not been called") as e:
        core.track_frame_filtered(chain["blobs"][:1], chain["counts"][:1], [1.0])
    assert e.value.code == capi.MOCAP_E_ARG
    for kw in ({"num_objects": 9}, {"num_objects": 2, "b": np.ones(17), "a": np.ones(17)}, {"num_objects": 2, "buffer_size": 1025}):
        with pytest.raises(capi.MocapError) as e:
            core.set_object_filter(**kw)
        assert e.value.code == capi.MOCAP_E_LIMIT, kw
    core.set_object_filter(D)                                     # the limits themselves are accepted
    core.set_object_filter(8, np.ones(16) / 16, np.r_[1.0, np.zeros(15)], buffer_size=1024)
    core.set_object_filter(0)
