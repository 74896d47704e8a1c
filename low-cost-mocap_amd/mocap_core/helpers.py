"""Host-side mirror of the reference's hot-path seam (computer_code/api/helpers.py:203-421).

Same function names, argument conventions, return shapes and error behaviour as the four
module-level functions `api/index.py:1` imports from `helpers`, so the Flask/socket.io
layer, the UI and the drone path are untouched (INTEGRATION.md shows the 6-line patch):

    find_point_correspondance_and_object_points(image_points, camera_poses, frames)   helpers.py:339
    triangulate_points(image_points, camera_poses)                                    helpers.py:330
    calculate_reprojection_errors(image_points, object_points, camera_poses)          helpers.py:203
    bundle_adjustment(image_points, camera_poses, socketio)                           helpers.py:244
  (+ the singular forms triangulate_point / calculate_reprojection_error)

Everything numeric runs in the HIP core through the C ABI (mocap_core.capi); this file only
converts between the reference's nested lists / None sentinels and the packed arrays of
include/mocap_core.h.  There is no CPU fallback: without the .so or a GPU these raise.

Intrinsics: the reference reads them from the `Cameras` singleton (helpers.py:215,295,340);
here `set_camera_params()` takes the same list of {"intrinsic_matrix": 3x3, ...} dicts
(the content of api/camera-params.json).
"""
import os
import threading
import time

import numpy as np

from . import capi

# Bundle adjustment through the reference's seam (helpers.bundle_adjustment, index.py:272) defaults to the mode that
# reproduces the reference's poses BIT FOR BIT: its own scipy.optimize.least_squares call, residuals evaluated on the GPU
# (seconds per calibration; the reference takes minutes).  "resident" -- the whole trust-region loop inside the core,
# milliseconds, the mode the BA iterations/s metric measures -- lands inside the reference's own run-to-run spread but
# not inside north_star's 1e-5 on rigs where the reference itself is not reproducible to 1e-5 (8 cameras: the reference
# moves 1.7e-3 under a 1e-15 nudge of its start vector, resident mode 2.3e-3 from it).  Opt in with
# set_bundle_adjustment_mode("resident").
DEFAULT_BA_MODE = "scipy"

_state = {
    "core": None,
    "ba_core": None,         # bundle adjustment's own context (own stream, own lock inside the library): a calibration never blocks the frame loop
    "ba_lock": threading.Lock(),   # one calibration at a time (the reference's handler is not re-entrant either)
    "camera_params": None,   # list of dicts like api/camera-params.json
    "cam_key": None,         # bytes of (K, R, t) currently uploaded
    "lock": threading.Lock(),
    "ba_mode": DEFAULT_BA_MODE,   # "scipy" (reference optimizer, GPU residuals) | "resident" (LM loop in the core)
    "ba_blas_threads": None,      # None: the process's BLAS settings are left alone (as the reference does); n: pinned for the solve
    "img_key": None,         # (rows, cols, K, dist, rot) of the lens model currently uploaded
    "to_world": None,        # last Cameras.to_world_coords_matrix handed to set_to_world_coords_matrix
    "overlay": 0,            # capi.OVERLAY_* bits of set_preview_overlay: the drawings on the preview, off by default
    "centroid": capi.CENTROID_REFERENCE,   # capi.CENTROID_* of set_centroid_mode: integer centroids by default
    "bodies": None,          # set_rigid_bodies: (names, marker arrays, tol, max_rms, work_cap), None = no body registered
    "markers": None,         # set_marker_tracker: (gate, max_missed, vel_alpha, T_max), None = tracker off
    "body_tracker": None,    # set_body_tracker: (gate, max_missed, vel_alpha), None = tracker off
    "consolidate": capi.CONSOLIDATE_OFF,   # capi.CONSOLIDATE_* of set_point_consolidation: the reference's points by default
    "refine": 0,             # set_point_refinement: Levenberg-Marquardt steps per object point, 0 = the reference's DLT points
}


def get_core(device_id=0):
    if _state["core"] is None:
        _state["core"] = capi.MocapCore(device_id)
    return _state["core"]


def set_preview_overlay(flags):
    """The reference's drawings on the preview, painted on the device: capi.OVERLAY_CONTOURS (cv.drawContours,
    helpers.py:148) | capi.OVERLAY_CENTRES (cv.circle, helpers.py:157) | capi.OVERLAY_EPILINES (drawlines, helpers.py:365).
    0 (default) = bare frames.  camera_read_find_dots, get_frames_jpeg and camera_read_track then return annotated pictures;
    with OVERLAY_EPILINES find_point_correspondance_and_object_points draws the lines into the frames it is handed.  The
    coordinate label of helpers.py:156 (cv.putText) is not drawn."""
    flags = int(flags)
    if flags & ~(capi.OVERLAY_CONTOURS | capi.OVERLAY_CENTRES | capi.OVERLAY_EPILINES):
        raise ValueError(f"unknown preview overlay bit in {flags:#x}")
    with _state["lock"]:
        _state["overlay"] = flags


def set_centroid_mode(mode):
    """What camera_read_find_dots, get_frames_jpeg and camera_read_track return as image points: capi.CENTROID_REFERENCE
    (default) = the reference's int(m10 / m00) as Python ints; capi.CENTROID_WEIGHTED = the grey-weighted sub-pixel centroid
    of include/mocap_core.h (mocap_set_centroid_mode) as floats.  Contours, their order and the counts are the same."""
    mode = int(mode)
    if mode not in (capi.CENTROID_REFERENCE, capi.CENTROID_WEIGHTED):
        raise ValueError(f"unknown centroid mode {mode}")
    with _state["lock"]:
        _state["centroid"] = mode


def set_point_consolidation(on):
    """Each blob supports at most one object point (mocap_set_point_consolidation, include/mocap_core.h): with `on` true
    track_frame*, camera_read_track and the payload built from them return a frame's points compacted to a set in which no two
    share an image blob -- one point per marker instead of the reference's twins.  Off by default; remembered, and applied to a
    core handed over later.  find_point_correspondance_and_object_points stays the reference's function."""
    mode = capi.CONSOLIDATE_BLOBS if on else capi.CONSOLIDATE_OFF
    with _state["lock"]:
        _state["consolidate"] = mode
        if _state["core"] is not None:
            _state["core"].set_point_consolidation(mode)


def set_point_refinement(iters):
    """Least-squares object points with each camera's own intrinsic matrix (mocap_set_point_refinement, include/mocap_core.h):
    with iters in 1 .. capi.REFINE_MAX_ITERS, find_point_correspondance_and_object_points, track_frame*, camera_read_track and the
    payload built from them return each point moved from the reference's DLT point to the minimum of its reprojection error by
    that many Levenberg-Marquardt steps (4 reach the optimum), and its error taken there.  0 (default) = the reference's points.
    Remembered, and applied to a core handed over later."""
    iters = int(iters)
    if not 0 <= iters <= capi.REFINE_MAX_ITERS:
        raise ValueError(f"point refinement takes 0 .. {capi.REFINE_MAX_ITERS} iterations, not {iters}")
    with _state["lock"]:
        _state["refine"] = iters
        if _state["core"] is not None:
            _state["core"].set_point_refinement(iters)


def _apply_overlay(core):
    """The module switches -> the context (callers hold the lock); a core handed over by set_core gets them on first use."""
    if getattr(core, "preview_overlay", 0) != _state["overlay"]:
        core.set_preview_overlay(_state["overlay"])
    if getattr(core, "centroid_mode", capi.CENTROID_REFERENCE) != _state["centroid"]:
        core.set_centroid_mode(_state["centroid"])
    return core


def _points_list(core, blobs_c, n):
    """One camera's stored centroids -> the list _find_dot returns: ints (helpers.py:153-154), floats in weighted mode."""
    if not n:
        return [[None, None]]
    if core.centroid_mode == capi.CENTROID_WEIGHTED:
        return blobs_c[:n].astype(np.float64).tolist()
    return blobs_c[:n].astype(np.int64).tolist()


def _ba_core():
    """Bundle adjustment runs on its own context of the same GPU: the reference's frame loop (helpers.py:68-135, MJPEG
    thread) keeps running while calculate_camera_pose -> bundle_adjustment (index.py:229-277) runs in a socket handler
    thread; one context means one internal lock and one stream, i.e. a calibration of seconds in front of every frame."""
    if _state["ba_core"] is None:
        _state["ba_core"] = capi.MocapCore(get_core().device_id)
    return _state["ba_core"]


def set_core(core):
    """Use an existing MocapCore (e.g. one per GPU in a frame-sharded run)."""
    with _state["lock"]:
        if _state["ba_core"] is not None and (core is None or core.device_id != _state["ba_core"].device_id):
            _state["ba_core"] = None
        _state["core"] = core
        _state["cam_key"] = None      # cameras, lens model and world transform live in the context:
        _state["img_key"] = None      # re-upload them to the new one on first use
        if core is not None and _state["to_world"] is not None:
            core.set_world_transform(_state["to_world"])


def set_camera_params(camera_params):
    """camera_params: list of {"intrinsic_matrix": 3x3 list, ...} (api/camera-params.json)."""
    _state["camera_params"] = [dict(p) for p in camera_params]
    _state["cam_key"] = None
    _state["img_key"] = None


def set_bundle_adjustment_blas_threads(n):
    """Mode "scipy" spends its host time in SciPy's SVD of the m x n Jacobian.  On a many-core host OpenBLAS's default thread
    count makes that SVD slower, not faster (1 000 points x 50 parameters: 1.1 s per calibration with 64 spinning threads on a
    shared 256-thread box, 0.23 s with one -- bench.py ba.default_mode.one_blas_thread), and its last bits depend on the thread
    count either way.  n = 1 pins the BLAS for the duration of a solve (threadpoolctl); None (default) leaves the process's
    settings alone, like the reference."""
    _state["ba_blas_threads"] = None if n is None else int(n)


def set_bundle_adjustment_mode(mode):
    assert mode in ("resident", "scipy")
    _state["ba_mode"] = mode


class bundle_adjustment_mode:
    """with helpers.bundle_adjustment_mode("resident"): ...  -- the previous mode comes back whatever happens inside."""

    def __init__(self, mode):
        assert mode in ("resident", "scipy")
        self.mode = mode

    def __enter__(self):
        self.prev = _state["ba_mode"]
        _state["ba_mode"] = self.mode
        return self

    def __exit__(self, *exc):
        _state["ba_mode"] = self.prev
        return False


def _intrinsics(C):
    params = _state["camera_params"]
    if params is None:
        raise RuntimeError("set_camera_params() has not been called (the reference loads camera-params.json)")
    if len(params) < C:
        raise IndexError("fewer camera_params entries than camera poses")  # the reference raises IndexError
    return np.array([np.array(params[i]["intrinsic_matrix"], dtype=np.float64) for i in range(C)])


def _pose_arrays(camera_poses):
    R = np.array([np.array(p["R"], dtype=np.float64).reshape(3, 3) for p in camera_poses])
    t = np.array([np.array(p["t"], dtype=np.float64).reshape(3) for p in camera_poses])
    return R, t


def _upload_cameras(camera_poses):
    """mocap_set_cameras only when (K, R, t) changed -- replaces the per-call rebuild of P = K[R|t]
    (helpers.py:305-308, :351-355) and the per-root fundamentalFromProjections (helpers.py:362)."""
    core = get_core()
    R, t = _pose_arrays(camera_poses)
    K = _intrinsics(len(camera_poses))
    key = K.tobytes() + R.tobytes() + t.tobytes()
    if key != _state["cam_key"]:
        core.set_cameras(K, R, t)
        _state["cam_key"] = key
    if getattr(core, "point_consolidation", capi.CONSOLIDATE_OFF) != _state["consolidate"]:   # a core handed over by set_core
        core.set_point_consolidation(_state["consolidate"])
    if getattr(core, "point_refinement", 0) != _state["refine"]:
        core.set_point_refinement(_state["refine"])
    return core


def _obs_array(image_points, C):
    """(N, C, 2) list / object ndarray with None -> float64 with NaN."""
    arr = np.asarray(image_points, dtype=object).reshape(-1, C, 2)
    out = np.full(arr.shape, np.nan)
    mask = np.vectorize(lambda v: v is not None)(arr) if arr.size else np.zeros(arr.shape, bool)
    out[mask] = arr[mask].astype(np.float64)
    bad = ~(mask[..., 0] & mask[..., 1])
    out[bad] = np.nan
    return out


# ----------------------------------------------------------------------------- triangulation
def triangulate_points(image_points, camera_poses):
    """helpers.py:330-336.  Rows with fewer than two views are [None, None, None]."""
    C = len(camera_poses)
    with _state["lock"]:
        core = _upload_cameras(camera_poses)
        obs = _obs_array(image_points, C)
        if obs.shape[0] == 0:
            return np.array([])
        xyz, _ = core.triangulate(obs)
    missing = np.isnan(xyz[:, 0])
    if not missing.any():
        return xyz
    out = xyz.astype(object)
    out[missing] = None
    return out


def triangulate_points_refined(image_points, camera_poses, iters=None):
    """triangulate_points with the point refinement of include/mocap_core.h behind it (mocap_triangulate_refined): each row's DLT
    point moved to the minimum of its reprojection error, every camera with its own intrinsic matrix.  iters: None = the count of
    set_point_refinement, or 4 when that is off.  Rows the stage does not refine -- fewer than two views, a start behind a
    camera -- are [None, None, None]."""
    C = len(camera_poses)
    with _state["lock"]:
        core = _upload_cameras(camera_poses)
        obs = _obs_array(image_points, C)
        if obs.shape[0] == 0:
            return np.array([])
        xyz, _, _ = core.triangulate_refined(obs, iters=(_state["refine"] or 4) if iters is None else int(iters))
    missing = np.isnan(xyz[:, 0])
    if not missing.any():
        return xyz
    out = xyz.astype(object)
    out[missing] = None
    return out


def triangulate_point(image_points, camera_poses):
    """helpers.py:293-327."""
    res = triangulate_points([image_points], camera_poses)
    row = res[0]
    return [None, None, None] if row[0] is None else np.asarray(row, dtype=np.float64)


def calculate_reprojection_errors(image_points, object_points, camera_poses):
    """helpers.py:203-211: entries with fewer than two views are skipped (the result may be shorter).
    The errors are those of the object points PASSED IN (mocap_reproject), as the function's contract says; the
    reference's three call sites happen to pass the triangulation of the same observations."""
    C = len(camera_poses)
    with _state["lock"]:
        core = _upload_cameras(camera_poses)
        obs = _obs_array(image_points, C)
        if obs.shape[0] == 0:
            return np.array([])
        op = np.asarray(object_points, dtype=object).reshape(obs.shape[0], 3)
        xyz = np.full(op.shape, np.nan)
        ok = np.vectorize(lambda v: v is not None)(op).all(axis=1)
        xyz[ok] = op[ok].astype(np.float64)
        err = core.reproject(obs, xyz)
    return err[~np.isnan(err)]


def calculate_reprojection_error(image_points, object_point, camera_poses):
    """helpers.py:214-241: None when fewer than two cameras see the point."""
    e = calculate_reprojection_errors([image_points], [object_point], camera_poses)
    return None if e.size == 0 else e[0]


# ----------------------------------------------------------------------------- frame path
def pack_frame(image_points, M_max=None, strict=False):
    """Nested lists of one frame -> (blobs f32 [1][C][M][2], counts i32 [1][C], rounded: bool).

    The C ABI's frame path carries blob coordinates as float32.  The reference measures point-line distances on whatever
    image_points holds (helpers.py:367-373: int64 for _find_dot's int() centroids, float64 for floats).  Integer centroids
    (the reference's own, |x| < 2^24) and float32-valued sub-pixel centroids are carried exactly.  Any other float64
    coordinate is rounded to the nearest float32 (2e-5 px at 320 px; `rounded` says so) -- or refused with strict=True.
    NaN / infinite coordinates are always refused."""
    C = len(image_points)
    n = [len(p) for p in image_points]
    M = max(1, max(n) if n else 1) if M_max is None else M_max
    blobs = np.full((1, C, M, 2), np.nan, dtype=np.float32)
    counts = np.zeros((1, C), dtype=np.int32)
    rounded = False
    for c, pts in enumerate(image_points):
        if pts:
            exact = np.asarray(pts, dtype=np.float64)
            if not np.isfinite(exact).all():
                raise ValueError(f"image point of camera {c} is NaN or infinite")
            as_f32 = exact.astype(np.float32)
            if not np.array_equal(as_f32.astype(np.float64), exact):
                if strict:
                    bad = exact[as_f32.astype(np.float64) != exact][0]
                    raise ValueError(f"image point coordinate {bad!r} (camera {c}) is not representable in float32: the core's "
                                     "blob arrays are float32 (include/mocap_core.h)")
                rounded = True
            blobs[0, c, :len(pts)] = as_f32
        counts[0, c] = len(pts)
    return blobs, counts, rounded


def find_point_correspondance_and_object_points(image_points, camera_poses, frames):
    """helpers.py:339-421.  `image_points` is mutated like the reference does (the [None, None]
    sentinel of an empty camera is removed, helpers.py:342-346).  `frames` is returned as it came -- the very
    objects -- unless set_preview_overlay has capi.OVERLAY_EPILINES on: then the points' epipolar lines are drawn into
    the frames on the device (helpers.py:365, drawlines; contract in include/mocap_core.h, mocap_draw_epilines) and the
    drawn copies are returned; entries that are None are skipped."""
    for image_points_i in image_points:
        try:
            image_points_i.remove([None, None])
        except Exception:
            pass
    with _state["lock"]:
        core = _upload_cameras(camera_poses)
        blobs, counts, _ = pack_frame(image_points)
        res = core.match_triangulate_auto(blobs, counts, gate_px=5.0)
        if _state["refine"] and int(res["status"][0]) == 0:      # set_point_refinement: the staged call on the frame's own arrays
            res.update({k: v for k, v in core.refine_points(blobs, counts, res["xyz"], res["err"], res["corr"], res["n_out"], res["status"],
                                                           iters=_state["refine"]).items() if k != "info"})
        if _state["overlay"] & capi.OVERLAY_EPILINES and int(res["status"][0]) == 0:
            frames = _draw_epilines(core, frames, blobs, counts, res)
    if int(res["status"][0]) != 0:
        # still over a cap after the worst-case re-submit (> 2^24 candidate groups for one root, > 2^32 per
        # frame, C*M > 1024 roots): the reference would enumerate the full product; an empty answer would be
        # silently wrong
        raise capi.MocapError(_status_message(int(res["status"][0])))
    k = int(res["n_out"][0])
    if k == 0:
        return np.array([]), np.array([]), frames
    return res["err"][0, :k].copy(), res["xyz"][0, :k].copy(), frames


def _draw_epilines(core, frames, blobs, counts, res):
    """frames: one S x S x 3 BGR picture or None per camera -> the list with the frame's epipolar lines drawn."""
    have = [i for i, f in enumerate(frames) if f is not None]
    if not have or len(frames) != core.C:
        return frames
    shape = np.asarray(frames[have[0]]).shape
    bgr = np.zeros((1, core.C) + shape, dtype=np.uint8)
    for i in have:
        bgr[0, i] = frames[i]
    drawn = core.draw_epilines(bgr, blobs, counts, res["corr"], res["n_out"], res["status"])
    return [drawn[0, i] if f is not None else None for i, f in enumerate(frames)]


def find_point_correspondance_and_object_points_batch(blobs, counts, camera_poses, gate_px=5.0, K_max=None):
    """Batch form on the packed layout (many frames per call); also returns the correspondence indices."""
    with _state["lock"]:
        core = _upload_cameras(camera_poses)
        return core.match_triangulate_auto(blobs, counts, gate_px=gate_px, K_max=K_max)


# ----------------------------------------------------------------------------- after the path
# ----------------------------------------------------------------------------- before the path
def camera_read_find_dots(raw_frames, M_max=64, want_frames=True):
    """The per-camera body of Cameras._camera_read (helpers.py:71-82) + Cameras._find_dot
    (helpers.py:143-163) for one set of raw frames (what pseyepy's Camera.read() returns):
    returns (frames, image_points) with frames = the processed BGR frames the reference streams
    (bare by default; with the contours and centre marks of helpers.py:148,157 under set_preview_overlay,
    never with the coordinate label of helpers.py:156) and image_points = per camera [[x, y], ...] or [[None, None]]
    (helpers.py:158-159) -- ready for find_point_correspondance_and_object_points.
    Lens model and rotation come from set_camera_params() (camera-params.json entries)."""
    raw = np.ascontiguousarray(np.asarray(raw_frames, dtype=np.uint8))
    C, rows, cols = raw.shape[0], raw.shape[1], raw.shape[2]
    params = _state["camera_params"]
    if params is None or len(params) < C:
        raise RuntimeError("set_camera_params() has not been called with one entry per camera")
    K = np.array([np.array(params[i]["intrinsic_matrix"], dtype=np.float64) for i in range(C)])
    dist = np.array([np.array(params[i]["distortion_coef"], dtype=np.float64).ravel()[:5] for i in range(C)])
    rot = np.array([int(params[i].get("rotation", 0)) for i in range(C)], dtype=np.int32)
    with _state["lock"]:
        core = _apply_overlay(get_core())
        key = (rows, cols, K.tobytes(), dist.tobytes(), rot.tobytes())
        if _state["img_key"] != key:
            core.set_image_params(rows, cols, K, dist, rot)
            _state["img_key"] = key
        res = core.find_blobs(raw[None], M_max=M_max, want_processed=want_frames)
        if (res["status"] & capi.BLOB_ST_POINT_OVERFLOW).any():     # more dots than slots: ask again
            res = core.find_blobs(raw[None], M_max=int(res["n_contours"].max()) + 1, want_processed=want_frames)
    if (res["status"] & capi.BLOB_ST_CAP_OVERFLOW).any():
        cams = np.nonzero(res["status"][0] & capi.BLOB_ST_CAP_OVERFLOW)[0].tolist()
        raise capi.MocapError(f"camera(s) {cams}: more contours than the blob stage's largest tables hold "
                              "(BLOB_ST_CAP_OVERFLOW); no centroids were produced for them")
    image_points = []
    for c in range(C):
        image_points.append(_points_list(core, res["blobs"][0, c], int(res["counts"][0, c])))
    frames = [f for f in res["processed"][0]] if want_frames else [None] * C
    return frames, image_points


def get_frames_jpeg(raw_frames, M_max=64, quality=95):
    """The MJPEG preview of the reference (index.py:55-56: cameras.get_frames(), i.e. np.hstack of the processed frames,
    then cv.imencode('.jpg', frames)) for one set of raw frames: returns (jpeg_bytes, image_points).  The processed frames
    are encoded where the blob stage leaves them, on the device; only the file (about 1 % of the frames) comes back.
    jpeg_bytes is what the generator yields in place of cv.imencode(...)[1].tostring() (with the drawings
    set_preview_overlay has switched on, as camera_read_find_dots); image_points as camera_read_find_dots."""
    raw = np.ascontiguousarray(np.asarray(raw_frames, dtype=np.uint8))
    C, rows, cols = raw.shape[0], raw.shape[1], raw.shape[2]
    params = _state["camera_params"]
    if params is None or len(params) < C:
        raise RuntimeError("set_camera_params() has not been called with one entry per camera")
    K = np.array([np.array(params[i]["intrinsic_matrix"], dtype=np.float64) for i in range(C)])
    dist = np.array([np.array(params[i]["distortion_coef"], dtype=np.float64).ravel()[:5] for i in range(C)])
    rot = np.array([int(params[i].get("rotation", 0)) for i in range(C)], dtype=np.int32)
    with _state["lock"]:
        core = _apply_overlay(get_core())
        key = (rows, cols, K.tobytes(), dist.tobytes(), rot.tobytes())
        if _state["img_key"] != key:
            core.set_image_params(rows, cols, K, dist, rot)
            _state["img_key"] = key
        res = core.find_blobs_jpeg(raw[None], M_max=M_max, quality=quality)
        if (res["status"] & capi.BLOB_ST_POINT_OVERFLOW).any():     # more dots than slots: ask again
            res = core.find_blobs_jpeg(raw[None], M_max=int(res["n_contours"].max()) + 1, quality=quality)
    if (res["status"] & capi.BLOB_ST_CAP_OVERFLOW).any():
        cams = np.nonzero(res["status"][0] & capi.BLOB_ST_CAP_OVERFLOW)[0].tolist()
        raise capi.MocapError(f"camera(s) {cams}: more contours than the blob stage's largest tables hold "
                              "(BLOB_ST_CAP_OVERFLOW); no centroids were produced for them")
    image_points = []
    for c in range(C):
        image_points.append(_points_list(core, res["blobs"][0, c], int(res["counts"][0, c])))
    return res["jpeg"][0], image_points


def set_to_world_coords_matrix(to_world_coords_matrix):
    """Cameras.to_world_coords_matrix (helpers.py:40,100): with a matrix set, the frame path returns
    world coordinates -- the loop at helpers.py:96-103 runs fused in the kernel's store.  None = off
    (camera-0 coordinates, exactly what find_point_correspondance_and_object_points returns upstream)."""
    with _state["lock"]:
        _state["to_world"] = None if to_world_coords_matrix is None else np.array(to_world_coords_matrix, dtype=np.float64)
        get_core().set_world_transform(to_world_coords_matrix)


def locate_objects(object_points, errors):
    """helpers.py:424-480: list of {"pos", "heading", "error", "droneIndex"} for one frame."""
    P = np.asarray(object_points, dtype=np.float64).reshape(-1, 3)
    if P.shape[0] == 0:
        return []
    E = np.asarray(errors, dtype=np.float64).reshape(-1)
    with _state["lock"]:
        res = get_core().locate_objects(P[None], E[None], [P.shape[0]], O_max=max(1, P.shape[0]))
    return [{"pos": res["pos"][0, j].copy(), "heading": float(res["heading"][0, j]),
             "error": float(res["error"][0, j]), "droneIndex": int(res["droneIndex"][0, j])}
            for j in range(int(res["n_obj"][0]))]


def _objects_list(res, f=0):
    return [{"pos": res["pos"][f, j].copy(), "heading": float(res["heading"][f, j]),
             "error": float(res["error"][f, j]), "droneIndex": int(res["droneIndex"][f, j])}
            for j in range(min(int(res["n_obj"][f]), res["pos"].shape[1]))]


def track_frame(image_points, camera_poses, is_locating_objects=True, O_max=8):
    """The body of the reference's live loop after _find_dot in ONE core call (helpers.py:94-108):
    find_point_correspondance_and_object_points -> world coordinates (needs set_to_world_coords_matrix; without it the
    points stay in camera-0 coordinates) -> locate_objects.  Returns (errors, object_points, objects) -- exactly the
    three values the loop holds at helpers.py:109 before the Kalman filter -- ready for object_points_payload().
    `image_points` is mutated like the reference does (helpers.py:342-346)."""
    for image_points_i in image_points:
        try:
            image_points_i.remove([None, None])
        except Exception:
            pass
    with _state["lock"]:
        core = _upload_cameras(camera_poses)
        blobs, counts, _ = pack_frame(image_points)
        res = core.track_frame(blobs, counts, gate_px=5.0, O_max=O_max if is_locating_objects else 0)
    if int(res["status"][0]) != 0:
        raise capi.MocapError(_status_message(int(res["status"][0])))
    k = int(res["n_pts"][0])
    if k == 0:
        return np.array([]), np.array([]), []
    return res["err"][0, :k].copy(), res["xyz"][0, :k].copy(), (_objects_list(res) if is_locating_objects else [])


def set_rigid_bodies(bodies, tol=0.01, max_rms=0.005, work_cap=0):
    """Registers the rigid bodies the core looks for (mocap_set_rigid_bodies, include/mocap_core.h): `bodies` = a list of
    {"name": str, "markers": [[x, y, z], ...]} in body coordinates, 3 .. 8 markers each, at most 8 bodies; an empty list
    switches the stage off.  tol (gate on every marker-to-marker distance) and max_rms (largest accepted residual of the fit)
    are in the unit of the object points.  A registration the core refuses raises capi.MocapError and changes nothing."""
    names = [str(b["name"]) for b in bodies]
    markers = [np.asarray(b["markers"], dtype=np.float64).reshape(-1, 3) for b in bodies]
    with _state["lock"]:
        get_core().set_rigid_bodies(markers, tol=tol, max_rms=max_rms, work_cap=work_cap)
        _state["bodies"] = (names, markers, float(tol), float(max_rms), int(work_cap)) if bodies else None


def _default_selection(ids, n_pts, status):
    """learn_rigid_body's sel=None rule: the track ids present (among a frame's first n_pts slots) in at least half of the
    valid frames, ascending."""
    F, K_max = ids.shape
    valid = (n_pts >= 0) & (n_pts <= K_max)
    if status is not None:
        valid &= status == 0
    n_valid = int(valid.sum())
    live = valid[:, None] & (np.arange(K_max)[None, :] < n_pts[:, None]) & (ids >= 0)
    frames, seen = np.nonzero(live)
    pairs = np.unique(np.stack([frames, ids[frames, seen]], axis=1), axis=0) if frames.size else np.zeros((0, 2), dtype=np.int64)
    found, counts = np.unique(pairs[:, 1], return_counts=True)
    sel = [int(i) for i, c in zip(found, counts) if 2 * int(c) >= n_valid]
    if not 3 <= len(sel) <= capi.RB_MAX_MARKERS:
        raise ValueError(f"learn_rigid_body: {len(sel)} track ids are present in at least half of the {n_valid} valid frames, a body "
                         f"has 3 .. {capi.RB_MAX_MARKERS} markers (frames per id: {dict(zip(found.tolist(), counts.tolist()))}); pass sel")
    return sel


def learn_rigid_body(capture, sel=None, name="body", **kw):
    """A body's marker set learned from a capture of it in motion (mocap_learn_rigid_body, include/mocap_core.h).  capture =
    {"xyz" [F][K_max][3], "n_pts" | "n_out" [F], "id" [F][K_max], "status" [F] (optional)}: the frame path's points and the marker
    tracker's ids, as NumPy arrays or as torch tensors on the core's GPU (those are read in place, only the result crosses PCIe).
    sel = the track ids of the body's markers; None = the ids present in at least half of the valid frames (ValueError unless that
    gives 3 .. 8).  kw: ref_frame, iters, max_rms.  Returns MocapCore.learn_rigid_body's dict plus "name" and "sel": hand it to
    set_rigid_bodies([learned], tol=...) with tol < learned["min_pair_distance"] / 2.  No frame that shows every selected marker
    raises capi.MocapError."""
    xyz = capture["xyz"]
    n_pts = capture["n_pts"] if "n_pts" in capture else capture["n_out"]
    ids, status = capture["id"], capture.get("status")
    ref_frame, iters, max_rms = int(kw.pop("ref_frame", -1)), int(kw.pop("iters", 4)), float(kw.pop("max_rms", float("inf")))
    if kw:
        raise TypeError(f"learn_rigid_body: unexpected arguments {sorted(kw)}")
    resident = getattr(xyz, "is_cuda", False)
    if resident:
        import torch
        F, K_max = xyz.shape[0], xyz.shape[1]
        assert xyz.dtype == torch.float64 and xyz.is_contiguous() and xyz.dim() == 3 and xyz.shape[2] == 3
        assert n_pts.dtype == torch.int32 and n_pts.is_contiguous() and n_pts.is_cuda and n_pts.numel() == F
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.is_cuda and tuple(ids.shape) == (F, K_max)
        assert status is None or (status.dtype == torch.int32 and status.is_contiguous() and status.is_cuda and status.numel() == F)
    with _state["lock"]:
        core = get_core()
        if resident:
            if xyz.device.index != core.device_id or any(t is not None and t.device != xyz.device for t in (n_pts, ids, status)):
                raise ValueError(f"the capture lives on {xyz.device}, the core on GPU {core.device_id}: a resident capture is read in place")
            torch.cuda.current_stream(xyz.device).synchronize()      # whatever torch itself still has queued on these buffers
        if sel is None:
            host = (lambda t: None if t is None else t.cpu().numpy()) if resident else (lambda a: None if a is None else np.asarray(a))
            sel = _default_selection(host(ids).astype(np.int32), host(n_pts).astype(np.int32).reshape(-1), host(status))
        sel = [int(i) for i in sel]
        if resident:
            result = torch.empty(capi.LB_RESULT, dtype=torch.float64, device=xyz.device)
            core.learn_rigid_body_dev(F, K_max, xyz.data_ptr(), n_pts.data_ptr(), ids.data_ptr(), 0 if status is None else status.data_ptr(),
                                      sel, ref_frame, iters, max_rms, result.data_ptr())
            core.synchronize()
            learned = core.learned_body(result.cpu().numpy(), len(sel))
        else:
            learned = core.learn_rigid_body(np.asarray(xyz), np.asarray(n_pts), np.asarray(ids), sel,
                                            None if status is None else np.asarray(status), ref_frame, iters, max_rms)
    if learned["status"] & capi.LB_ST_NO_REF:
        raise capi.MocapError(f"learn_rigid_body: no valid frame of the capture shows all {len(sel)} selected markers {sel}"
                              + (f" (ref_frame {ref_frame} does not)" if ref_frame >= 0 else "")
                              + ": capture again with every marker in view at once, or pass ref_frame = a frame that shows them all")
    learned["name"], learned["sel"] = str(name), sel
    return learned


def track_table(ids, hits=None, min_len=10, min_hits=0):
    """Which track ids of a session get a trajectory row (plain NumPy, on the host).  ids [F][K_max] as the marker tracker writes
    them (-1 = no track), hits [F][K_max] or None: a sighting counts when its id is >= 0 and, with hits given, its hits >= min_hits.
    Returns (relabel int32 [n_ids], rows int32 [R]): the ids with at least min_len sightings in ascending order, rows[r] = the id of
    row r, relabel[i] = the row of id i or -1 -- what mocap_gather_tracks takes.  n_ids = the largest id seen + 1 (1 for none)."""
    ids = np.asarray(ids)
    seen = ids >= 0
    if hits is not None:
        seen &= np.asarray(hits) >= min_hits
    counts = np.bincount(ids[seen].astype(np.int64).ravel(), minlength=1)
    rows = np.nonzero(counts >= max(int(min_len), 1))[0].astype(np.int32)
    relabel = np.full(counts.size, -1, dtype=np.int32)
    relabel[rows] = np.arange(rows.size, dtype=np.int32)
    return relabel, rows


def stitch_table(relabel, row_of):
    """The relabel of the second gather (plain NumPy, on the host): relabel [n_ids] as track_table gives it, row_of [R] as
    mocap_stitch_tracks gives it -> relabel2 int32 [n_ids], relabel2[i] = row_of[relabel[i]] where relabel[i] >= 0, else -1: every id
    of a chain lands on the chain's one row, an id whose row was empty on none."""
    relabel, row_of = np.asarray(relabel, dtype=np.int32), np.asarray(row_of, dtype=np.int32)
    out = np.full(relabel.shape, -1, dtype=np.int32)
    has = relabel >= 0
    out[has] = row_of[relabel[has]]
    return out


def _stitch_report(rows, st, t_at):
    """ids, links, fragments of a stitched session from the [R] outputs of mocap_stitch_tracks (host arrays); t_at(frames) -> the
    time stamps of those frames."""
    heads = [r for r in range(rows.size) if st["row_of"][r] >= 0 and st["chain"][r] == r]      # ascending: the order of row_of
    ids, links = [], []
    for r in heads:
        chain = [r]
        while st["next"][chain[-1]] >= 0:
            chain.append(int(st["next"][chain[-1]]))
        ids.append(rows[chain])
        links += [(p, q) for p, q in zip(chain[:-1], chain[1:])]
    if links:
        p, q = np.array(links).T
        dt = t_at(st["ext"][q, 0]) - t_at(st["ext"][p, 1])
        links = [(int(rows[a]), int(rows[b]), float(st["cost"][a]), float(d)) for a, b, d in zip(p, q, dt)]
    return ids, links, st["ext"]


def session_trajectories(t, xyz, n_pts, ids, hits=None, min_hits=0, min_len=10, degree=2, W=8, span=float("inf"), n_min=None,
                         max_gap=0, stitch=None):
    """A recorded session as one smoothed, gap-filled time series per marker ("trajectories", include/mocap_core.h): track_table ->
    mocap_gather_tracks -> mocap_smooth_tracks.  t [F], xyz [F][K_max][3], n_pts [F] (the frame path's), ids, hits [F][K_max] (the
    marker tracker's), as NumPy arrays or as torch tensors on the core's GPU (those are read in place: only ids and hits are copied to
    the host, for the table, and the results stay resident as torch tensors).  Returns {"ids" [R] the track id of each row, "relabel",
    "traj", "pos", "vel", "acc" [R][F][3], "res", "n_used", "flag" [R][F]}.  No id with min_len sightings raises ValueError; more than
    capi.TS_MAX_ROWS of them is the core's MOCAP_E_ARG.
    stitch = {"fit_frames", "max_dt", "gate", "gate_rate"} ("track stitching", include/mocap_core.h): a marker that was hidden for
    longer than the tracker's max_missed came back under a new id; the gathered rows go through mocap_stitch_tracks, stitch_table
    maps every id of a chain to the chain's row, and a second gather with R = n_chains feeds the smoother: one row per marker.  Only
    the [R] outputs of the stitching come to the host.  Then "ids" is a list of arrays, the track ids of each row in time order,
    "relabel" the second gather's, and the dict gains "links": [(from id, to id, cost, dt seconds)] and "fragments": ext int32
    [fragments][3] of the first gather's rows (first and last present frame, number present), in the order of track_table's rows."""
    resident = getattr(xyz, "is_cuda", False)
    host = (lambda a: None if a is None else a.cpu().numpy()) if resident else (lambda a: None if a is None else np.asarray(a))
    relabel, rows = track_table(host(ids), host(hits), min_len=min_len, min_hits=min_hits)
    R = int(rows.size)
    if R == 0:
        raise ValueError(f"session_trajectories: no track id has {min_len} sightings in this session")
    n_min = min(int(degree) + 2, 2 * int(W) + 1) if n_min is None else int(n_min)
    report = None

    def restitch(st, t_at):
        """-> (the second gather's relabel, its R)"""
        nonlocal report
        if st["n_chains"] < 1:
            raise ValueError("session_trajectories: no row of this session has a sample with a good time stamp")
        report = _stitch_report(rows, st, t_at)
        return stitch_table(relabel, st["row_of"]), int(st["n_chains"])

    with _state["lock"]:
        core = get_core()
        if not resident:
            traj = core.gather_tracks(xyz, n_pts, ids, relabel, R, hits=hits, min_hits=min_hits)
            if stitch is not None:
                t_host = np.asarray(t, dtype=np.float64).reshape(-1)
                st = core.stitch_tracks(t, traj, stitch["fit_frames"], stitch["max_dt"], stitch["gate"], stitch["gate_rate"])
                relabel, R = restitch(st, lambda f: t_host[f])
                traj = core.gather_tracks(xyz, n_pts, ids, relabel, R, hits=hits, min_hits=min_hits)
            out = core.smooth_tracks(t, traj, degree=degree, W=W, span=span, n_min=n_min, max_gap=max_gap)
        else:
            import torch
            F, K_max = xyz.shape[0], xyz.shape[1]
            assert xyz.dtype == torch.float64 and xyz.is_contiguous() and xyz.dim() == 3 and xyz.shape[2] == 3
            assert t.dtype == torch.float64 and t.is_contiguous() and t.is_cuda and t.numel() == F
            assert n_pts.dtype == torch.int32 and n_pts.is_contiguous() and n_pts.is_cuda and n_pts.numel() == F
            for a in (ids, hits):
                assert a is None or (a.dtype == torch.int32 and a.is_contiguous() and a.is_cuda and tuple(a.shape) == (F, K_max))
            if xyz.device.index != core.device_id:
                raise ValueError(f"the session lives on {xyz.device}, the core on GPU {core.device_id}: a resident session is read in place")
            dev = xyz.device
            tables = []                                           # device copies of relabel: alive until the last synchronize

            def gather():
                tables.append(torch.from_numpy(relabel).to(dev))
                rows_dev = torch.empty((R, F, 3), dtype=torch.float64, device=dev)
                torch.cuda.current_stream(dev).synchronize()      # whatever torch itself still has queued on these buffers
                core.gather_tracks_dev(F, K_max, xyz.data_ptr(), n_pts.data_ptr(), ids.data_ptr(), 0 if hits is None else hits.data_ptr(),
                                       min_hits, relabel.size, tables[-1].data_ptr(), R, rows_dev.data_ptr())
                return rows_dev

            if stitch is not None:
                traj = gather()
                d = {"ext": torch.empty((R, 3), dtype=torch.int32, device=dev), "cost": torch.empty(R, dtype=torch.float64, device=dev),
                     "n_chains": torch.empty(1, dtype=torch.int32, device=dev)}
                d.update({k: torch.empty(R, dtype=torch.int32, device=dev) for k in ("next", "prev", "chain", "row_of")})
                torch.cuda.current_stream(dev).synchronize()
                core.stitch_tracks_dev(F, R, t.data_ptr(), traj.data_ptr(), stitch["fit_frames"], stitch["max_dt"], stitch["gate"],
                                       stitch["gate_rate"], *[d[k].data_ptr() for k in core.STITCH_OUT])
                core.synchronize()
                st = {k: v.cpu().numpy() for k, v in d.items()}
                st["n_chains"] = int(st["n_chains"][0])
                relabel, R = restitch(st, lambda f: t[torch.from_numpy(np.asarray(f, dtype=np.int64)).to(dev)].cpu().numpy())
            traj = gather()
            out = {k: torch.empty((R, F, 3), dtype=torch.float64, device=dev) for k in ("pos", "vel", "acc")}
            out["res"] = torch.empty((R, F), dtype=torch.float64, device=dev)
            out["n_used"], out["flag"] = (torch.empty((R, F), dtype=torch.int32, device=dev) for _ in range(2))
            torch.cuda.current_stream(dev).synchronize()      # whatever torch itself still has queued on these buffers
            core.smooth_tracks_dev(F, R, t.data_ptr(), traj.data_ptr(), degree, W, span, n_min, max_gap,
                                   *[out[k].data_ptr() for k in ("pos", "vel", "acc", "res", "n_used", "flag")])
            core.synchronize()
    out.update(ids=rows, relabel=relabel, traj=traj)
    if report is not None:
        out.update(ids=report[0], links=report[1], fragments=report[2])
    return out


def find_rigid_groups(session, tol=0.003, min_common=30, max_dist=float("inf"), min_travel=0.0):
    """The rigid bodies of a recorded session ("rigid groups", include/mocap_core.h): the rows of session["traj"] -- the gathered
    samples, not the smoothed or filled ones -- whose mutual distances stay put.  session = what session_trajectories returns, NumPy
    or resident (a resident traj is read in place; only the [R] and [R][R] outputs come to the host).  Two rows are linked when they
    share min_common frames over which their distance has a standard deviation <= tol and a mean <= max_dist; min_travel (the
    diagonal of a row's bounding box) keeps markers that lie still out.  Returns a list of {"rows": the group's rows ascending,
    "ids": the track id of each row (with a stitched session: the array of ids each row went through), "size", "conflicts": pairs
    inside the group that share min_common frames and are NOT rigid -- a linkage, or two bodies bridged --, "max_spread": the largest
    standard deviation over its links, "dist" [size][size]: the mean distances}, ordered by lowest row."""
    traj = session["traj"]
    resident = getattr(traj, "is_cuda", False)
    with _state["lock"]:
        core = get_core()
        if not resident:
            res = core.rigid_groups(traj, min_common, tol, max_dist=max_dist, min_travel=min_travel)
        else:
            import torch
            R, F = traj.shape[0], traj.shape[1]
            assert traj.dtype == torch.float64 and traj.is_contiguous() and traj.dim() == 3 and traj.shape[2] == 3
            if traj.device.index != core.device_id:
                raise ValueError(f"the session lives on {traj.device}, the core on GPU {core.device_id}: a resident session is read in place")
            dev = traj.device
            d = {"cnt": torch.empty((R, R), dtype=torch.int32, device=dev), "n_groups": torch.empty(1, dtype=torch.int32, device=dev)}
            d.update({k: torch.empty((R, R), dtype=torch.float64, device=dev) for k in ("dist", "spread")})
            d.update({k: torch.empty(R, dtype=torch.float64, device=dev) for k in ("travel", "gspread")})
            d.update({k: torch.empty(R, dtype=torch.int32, device=dev) for k in ("group_of", "gsize", "ghead", "gconf")})
            torch.cuda.current_stream(dev).synchronize()      # whatever torch itself still has queued on these buffers
            core.rigid_groups_dev(F, R, traj.data_ptr(), min_common, tol, max_dist, min_travel, *[d[k].data_ptr() for k in core.RIGID_OUT])
            core.synchronize()
            res = {k: v.cpu().numpy() for k, v in d.items()}
            res["n_groups"] = int(res["n_groups"][0])
    ids = session["ids"]
    groups = []
    for g in range(res["n_groups"]):
        rows = np.flatnonzero(res["group_of"] == g)
        groups.append({"rows": rows.tolist(), "ids": [ids[r].tolist() if np.ndim(ids[r]) else int(ids[r]) for r in rows],
                       "size": int(res["gsize"][g]), "conflicts": int(res["gconf"][g]), "max_spread": float(res["gspread"][g]),
                       "dist": res["dist"][np.ix_(rows, rows)].copy()})
    return groups


def learn_session_bodies(capture, session, groups=None, names=None, **learn_kw):
    """From a session's rigid groups to registered bodies: every group with 3 .. capi.RB_MAX_MARKERS rows and no conflict goes
    through learn_rigid_body.  capture = learn_rigid_body's (the same frames the session was made of, NumPy or resident), session =
    session_trajectories' dict, groups = find_rigid_groups' list (None: found with its defaults), names = one per group (default
    "body<g>").  The capture's ids are relabelled through session["relabel"] -- an id >= 0 inside the table becomes its row,
    everything else -1; plain indexing, on the device for a resident capture -- and the learner is called with sel = the group's
    rows, so a stitched marker with several ids is one marker.  Returns (learned, skipped): learned = learn_rigid_body's dicts
    (plus "rows"), ready for set_rigid_bodies(learned, tol=...); skipped = [(group, reason)]."""
    if groups is None:
        groups = find_rigid_groups(session)
    relabel = np.ascontiguousarray(session["relabel"], dtype=np.int32)
    ids = capture["id"]
    if getattr(ids, "is_cuda", False):
        import torch
        table = torch.from_numpy(relabel).to(ids.device)
        inside = (ids >= 0) & (ids < relabel.size)
        rows_of = torch.where(inside, table[ids.clamp(0, relabel.size - 1).long()], torch.full_like(ids, -1)).contiguous()
    else:
        ids = np.asarray(ids)
        inside = (ids >= 0) & (ids < relabel.size)
        rows_of = np.where(inside, relabel[np.clip(ids, 0, relabel.size - 1)], -1).astype(np.int32)
    relabelled = {**capture, "id": rows_of}
    learned, skipped = [], []
    for g, group in enumerate(groups):
        if not 3 <= group["size"] <= capi.RB_MAX_MARKERS:
            skipped.append((group, f"{group['size']} rows: a body has 3 .. {capi.RB_MAX_MARKERS} markers"))
        elif group["conflicts"]:
            skipped.append((group, f"{group['conflicts']} pairs inside the group are not rigid: a linkage, or bodies bridged by a marker"))
        else:
            try:
                body = learn_rigid_body(relabelled, sel=group["rows"], name=names[g] if names is not None else f"body{g}", **learn_kw)
            except capi.MocapError as e:
                skipped.append((group, str(e)))
                continue
            body["rows"] = list(group["rows"])
            learned.append(body)
    return learned, skipped


def session_body_poses(t, session, bodies, max_rms=float("inf"), degree=2, W=8, span=float("inf"), n_min=None, max_gap=0, fill=True):
    """The motion of a session's rigid bodies ("body trajectories", include/mocap_core.h): mocap_pose_rows over session["traj"],
    mocap_smooth_tracks over the body origins, mocap_smooth_rotations over the quaternions and, with fill, mocap_fill_rows.
    t [F] = the session's time stamps, session = session_trajectories' dict, bodies = learn_session_bodies' `learned` list (its
    "rows" and "markers" are used), NumPy or resident: a resident traj (and t) is read in place and every result stays a torch
    tensor on that GPU.  degree .. max_gap are the smoothers' (both get the same).  Returns {"quat" [B][F][4], "R" [B][F][3][3],
    "t_pose" [B][F][3], "rms", "n_used", "present", "flag" [B][F] (capi.BP_*): the pose per frame; "pos", "vel", "acc" [B][F][3]: the
    body origin smoothed; "quat_s" [B][F][4], "omega" [B][F][3] (rad/s, world axes), "res_rot", "flag_s" [B][F] (capi.TS_*): the
    orientation smoothed; with fill "filled" [R][F][3], "src" [R][F] (capi.BP_SRC_*): the session's rows with hidden markers put
    where the body's pose says they are}."""
    for b, body in enumerate(bodies):
        if not isinstance(body, dict) or "rows" not in body or "markers" not in body:
            raise ValueError(f"session_body_poses: body {b} has no 'rows': pass learn_session_bodies' list (learn_rigid_body's dict "
                             "does not say which session rows its markers are)")
    if not bodies:
        raise ValueError("session_body_poses: no bodies")
    traj = session["traj"]
    resident = getattr(traj, "is_cuda", False)
    n_min = min(int(degree) + 2, 2 * int(W) + 1) if n_min is None else int(n_min)
    par = (int(degree), int(W), float(span), n_min, int(max_gap))
    B = len(bodies)
    with _state["lock"]:
        core = get_core()
        if not resident:
            o = core.pose_rows(traj, bodies, max_rms=max_rms)
            tr = core.smooth_tracks(t, o["t_pose"], *par)
            rot = core.smooth_rotations(t, o["quat"], *par)
            out = {**o, "pos": tr["pos"], "vel": tr["vel"], "acc": tr["acc"], "quat_s": rot["quat_s"], "omega": rot["omega"],
                   "res_rot": rot["res"], "flag_s": rot["flag"]}
            if fill:
                out.update(core.fill_rows(traj, bodies, o["flag"], o["R"], o["t_pose"], rot["flag"], rot["quat_s"], tr["pos"]))
        else:
            import torch
            R, F = traj.shape[0], traj.shape[1]
            assert traj.dtype == torch.float64 and traj.is_contiguous() and traj.dim() == 3 and traj.shape[2] == 3
            if traj.device.index != core.device_id:
                raise ValueError(f"the session lives on {traj.device}, the core on GPU {core.device_id}: a resident session is read in place")
            dev = traj.device
            t = t if getattr(t, "is_cuda", False) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(dev)
            assert t.dtype == torch.float64 and t.is_contiguous() and t.numel() == F

            def f64(*shape):
                return torch.empty(shape, dtype=torch.float64, device=dev)

            def i32(*shape):
                return torch.empty(shape, dtype=torch.int32, device=dev)

            out = {"quat": f64(B, F, 4), "R": f64(B, F, 3, 3), "t_pose": f64(B, F, 3), "rms": f64(B, F), "n_used": i32(B, F),
                   "present": i32(B, F), "flag": i32(B, F), "pos": f64(B, F, 3), "vel": f64(B, F, 3), "acc": f64(B, F, 3),
                   "quat_s": f64(B, F, 4), "omega": f64(B, F, 3), "res_rot": f64(B, F), "flag_s": i32(B, F)}
            ws = {"res": f64(B, F), "n_tr": i32(B, F), "flag_tr": i32(B, F), "n_rot": i32(B, F)}
            if fill:
                out.update(filled=f64(R, F, 3), src=i32(R, F))
            torch.cuda.current_stream(dev).synchronize()      # whatever torch itself still has queued on these buffers
            core.pose_rows_dev(F, R, traj.data_ptr(), bodies, max_rms, *[out[k].data_ptr() for k in core.POSE_OUT])
            core.smooth_tracks_dev(F, B, t.data_ptr(), out["t_pose"].data_ptr(), *par, out["pos"].data_ptr(), out["vel"].data_ptr(),
                                   out["acc"].data_ptr(), ws["res"].data_ptr(), ws["n_tr"].data_ptr(), ws["flag_tr"].data_ptr())
            core.smooth_rotations_dev(F, B, t.data_ptr(), out["quat"].data_ptr(), *par, out["quat_s"].data_ptr(),
                                      out["omega"].data_ptr(), out["res_rot"].data_ptr(), ws["n_rot"].data_ptr(), out["flag_s"].data_ptr())
            if fill:
                core.fill_rows_dev(F, R, traj.data_ptr(), bodies, out["flag"].data_ptr(), out["R"].data_ptr(), out["t_pose"].data_ptr(),
                                   out["flag_s"].data_ptr(), out["quat_s"].data_ptr(), out["pos"].data_ptr(), out["filled"].data_ptr(),
                                   out["src"].data_ptr())
            core.synchronize()
    return out


def session_joints(poses, min_common=30, tol_rank=1e-4, max_sep=float("inf")):
    """The joints of a session's bodies ("joints", include/mocap_core.h): mocap_find_joints over poses["flag"], poses["R"] and
    poses["t_pose"].  poses = what session_body_poses returns, NumPy or resident (resident poses are read in place; only the [B][B]
    and [B] outputs come to the host).  Two bodies are joined when they share min_common frames, their relative rotation spans
    more than one axis (BALL) or exactly one (HINGE) by tol_rank, and the two images of the joint's centre stay within max_sep (rms,
    metres); the skeleton is the minimum spanning forest over those pairs by that distance.  Returns {"joints": a list of {"a", "b",
    "kind" (capi.JT_HINGE or capi.JT_BALL), "centre_a", "centre_b" [3]: the joint in a's and in b's coordinates, "axis_a", "axis_b"
    [3] (HINGE; else NaN), "sep", "frames"} for the tree edges, a < b, ordered by (a, b); "parent" int32 [B]: each body's neighbour
    towards the root of its tree (-1 = a root or a body of no joint); "pairs": mocap_find_joints' tables}."""
    flag = poses["flag"]
    resident = getattr(flag, "is_cuda", False)
    with _state["lock"]:
        core = get_core()
        if not resident:
            res = core.find_joints(flag, poses["R"], poses["t_pose"], min_common=min_common, tol_rank=tol_rank, max_sep=max_sep)
        else:
            import torch
            B, F = flag.shape
            Rm, t_pose = poses["R"], poses["t_pose"]
            assert flag.dtype == torch.int32 and flag.is_contiguous()
            for a, n in ((Rm, 9), (t_pose, 3)):
                assert a.dtype == torch.float64 and a.is_contiguous() and a.is_cuda and a.numel() == B * F * n
            if flag.device.index != core.device_id:
                raise ValueError(f"the session lives on {flag.device}, the core on GPU {core.device_id}: a resident session is read in place")
            dev = flag.device
            d = {k: torch.empty((B, B), dtype=torch.int32, device=dev) for k in ("cnt", "kind", "accepted")}
            d.update({k: torch.empty((B, B, 3), dtype=torch.float64, device=dev) for k in ("lam", "centre", "axis")})
            d.update(sep=torch.empty((B, B), dtype=torch.float64, device=dev), parent=torch.empty(B, dtype=torch.int32, device=dev),
                     n_joints=torch.empty(1, dtype=torch.int32, device=dev))
            torch.cuda.current_stream(dev).synchronize()      # whatever torch itself still has queued on these buffers
            core.find_joints_dev(F, B, flag.data_ptr(), Rm.data_ptr(), t_pose.data_ptr(), min_common, tol_rank, max_sep,
                                 *[d[k].data_ptr() for k in core.JOINTS_OUT])
            core.synchronize()
            res = {k: v.cpu().numpy() for k, v in d.items()}
            res["n_joints"] = int(res["n_joints"][0])
    parent = res["parent"]
    joints = []
    for child in range(parent.size):
        if parent[child] >= 0:
            a, b = sorted((int(child), int(parent[child])))
            joints.append({"a": a, "b": b, "kind": int(res["kind"][a, b]), "centre_a": res["centre"][a, b].copy(),
                           "centre_b": res["centre"][b, a].copy(), "axis_a": res["axis"][a, b].copy(), "axis_b": res["axis"][b, a].copy(),
                           "sep": float(res["sep"][a, b]), "frames": int(res["cnt"][a, b])})
    joints.sort(key=lambda j: (j["a"], j["b"]))
    return {"joints": joints, "parent": parent, "pairs": res}


def _unwrapped_angle(twist, present, xp):
    """2 atan2(twist_s, twist_c) along the last axis of twist [J][F][2], unwrapped over the present frames of each joint (a jump of
    more than pi between consecutive present frames is a turn of 2 pi the other way); NaN elsewhere.  xp = numpy or torch."""
    raw = 2.0 * xp.arctan2(twist[..., 1], twist[..., 0])
    out = xp.full_like(raw, float("nan"))
    for j in range(raw.shape[0]):
        at = xp.nonzero((present[j] != 0) & ~xp.isnan(raw[j]))
        at = at[0] if isinstance(at, tuple) else at[:, 0]
        if at.shape[0] == 0:
            continue
        v = raw[j][at]
        step = v[1:] - v[:-1]
        turns = xp.cumsum(xp.round(step / (2.0 * np.pi)), 0)
        out[j][at[1:]] = v[1:] - 2.0 * np.pi * turns
        out[j][at[:1]] = v[:1]
    return out


def session_joint_motion(t, poses, joints, degree=2, W=8, span=float("inf"), n_min=None, max_gap=0):
    """The motion of a session's joints ("joints", include/mocap_core.h): mocap_joint_series, then mocap_smooth_tracks over the
    joints' centres and mocap_smooth_rotations over the relative quaternions.  t [F], poses = session_body_poses' dict, joints =
    session_joints' list (or its dict), NumPy or resident (then every result stays a torch tensor on that GPU).  A joint without
    "q_ref" gets b's orientation in a at the joint's first present frame, so its angles start at zero.  Returns {"present" [J][F],
    "centre" [J][F][3], "gap" [J][F], "quat_rel" [J][F][4], "twist" [J][F][2]: the series; "pos", "vel", "acc" [J][F][3]: the centre
    smoothed; "quat_s" [J][F][4], "omega" [J][F][3], "flag_s" [J][F]: the relative orientation smoothed; "angle" [J][F]: the hinge
    angle against q_ref in radians, unwrapped along the present frames (NaN for other kinds); "q_ref" [J][4]}."""
    joints = joints["joints"] if isinstance(joints, dict) else list(joints)
    if not joints:
        raise ValueError("session_joint_motion: no joints")
    flag = poses["flag"]
    resident = getattr(flag, "is_cuda", False)
    n_min = min(int(degree) + 2, 2 * int(W) + 1) if n_min is None else int(n_min)
    par = (int(degree), int(W), float(span), n_min, int(max_gap))
    J = len(joints)
    B, F = flag.shape
    # the reference orientations: conj(q_a) (x) q_b at each joint's first frame with both bodies POSED (two quaternions per joint)
    joints = [dict(j) for j in joints]
    for j in joints:
        if j.get("q_ref") is None:
            both = (flag[j["a"]] == capi.BP_POSED) & (flag[j["b"]] == capi.BP_POSED)
            at = both.nonzero()
            at = at[0] if isinstance(at, tuple) else at[:, 0]
            j["q_ref"] = (1.0, 0.0, 0.0, 0.0)
            if at.shape[0]:
                f0 = int(at[0])
                qa, qb = (np.asarray(poses["quat"][k][f0].cpu() if resident else poses["quat"][k][f0], dtype=np.float64) for k in (j["a"], j["b"]))
                p = (qa[0], -qa[1], -qa[2], -qa[3])
                ref = np.array([((p[0] * qb[0] - p[1] * qb[1]) - p[2] * qb[2]) - p[3] * qb[3],
                                ((p[0] * qb[1] + p[1] * qb[0]) + p[2] * qb[3]) - p[3] * qb[2],
                                ((p[0] * qb[2] - p[1] * qb[3]) + p[2] * qb[0]) + p[3] * qb[1],
                                ((p[0] * qb[3] + p[1] * qb[2]) - p[2] * qb[1]) + p[3] * qb[0]])
                j["q_ref"] = ref / np.sqrt(ref @ ref)
    with _state["lock"]:
        core = get_core()
        if not resident:
            out = core.joint_series(flag, poses["quat"], poses["R"], poses["t_pose"], joints)
            tr = core.smooth_tracks(t, out["centre"], *par)
            rot = core.smooth_rotations(t, out["quat_rel"], *par)
            out.update(pos=tr["pos"], vel=tr["vel"], acc=tr["acc"], quat_s=rot["quat_s"], omega=rot["omega"], flag_s=rot["flag"])
            out["angle"] = _unwrapped_angle(out["twist"], out["present"], np)
        else:
            import torch
            dev = flag.device
            if dev.index != core.device_id:
                raise ValueError(f"the session lives on {dev}, the core on GPU {core.device_id}: a resident session is read in place")
            t = t if getattr(t, "is_cuda", False) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(dev)
            assert t.dtype == torch.float64 and t.is_contiguous() and t.numel() == F

            def f64(*shape):
                return torch.empty(shape, dtype=torch.float64, device=dev)

            def i32(*shape):
                return torch.empty(shape, dtype=torch.int32, device=dev)

            out = {"present": i32(J, F), "centre": f64(J, F, 3), "gap": f64(J, F), "quat_rel": f64(J, F, 4), "twist": f64(J, F, 2),
                   "pos": f64(J, F, 3), "vel": f64(J, F, 3), "acc": f64(J, F, 3), "quat_s": f64(J, F, 4), "omega": f64(J, F, 3),
                   "flag_s": i32(J, F)}
            ws = {"res": f64(J, F), "n_tr": i32(J, F), "flag_tr": i32(J, F), "res_rot": f64(J, F), "n_rot": i32(J, F)}
            torch.cuda.current_stream(dev).synchronize()      # whatever torch itself still has queued on these buffers
            core.joint_series_dev(F, B, flag.data_ptr(), poses["quat"].data_ptr(), poses["R"].data_ptr(), poses["t_pose"].data_ptr(), joints,
                                  *[out[k].data_ptr() for k in core.SERIES_OUT])
            core.smooth_tracks_dev(F, J, t.data_ptr(), out["centre"].data_ptr(), *par, out["pos"].data_ptr(), out["vel"].data_ptr(),
                                   out["acc"].data_ptr(), ws["res"].data_ptr(), ws["n_tr"].data_ptr(), ws["flag_tr"].data_ptr())
            core.smooth_rotations_dev(F, J, t.data_ptr(), out["quat_rel"].data_ptr(), *par, out["quat_s"].data_ptr(),
                                      out["omega"].data_ptr(), ws["res_rot"].data_ptr(), ws["n_rot"].data_ptr(), out["flag_s"].data_ptr())
            core.synchronize()
            out["angle"] = _unwrapped_angle(out["twist"], out["present"], torch)
    out["q_ref"] = np.array([j["q_ref"] for j in joints], dtype=np.float64)
    return out


def session_joint_poses(t, session, bodies, poses, joints, axis_len=0.1, max_rms=float("inf"), max_rounds=4, degree=2, W=8,
                        span=float("inf"), n_min=None, max_gap=0, fill=True):
    """The bodies session_body_poses could not pose, posed through the skeleton ("joint poses", include/mocap_core.h):
    mocap_pose_joints over session["traj"], the bodies, poses (session_body_poses' dict) and joints (session_joints' dict or its
    list), then the two smoothers over the new tables and, with fill, mocap_fill_rows.  NumPy or resident: resident arrays are read
    in place and every result stays a torch tensor on that GPU.  A frame whose flag is BP_FEW or BP_DEGENERATE gets a pose from a
    neighbour at most max_rounds joints away from a POSED body: two markers and a ball joint's centre, or one marker off a hinge's
    axis (axis_len metres along it lies the hinge's second point), fitted like any other pose and kept when its rms is within
    max_rms.  Returns a dict shaped like poses: {"flag" [B][F] (capi.BP_*, BP_JOINTED among them), "quat", "R", "t_pose": the poses;
    "hops" [B][F]: joints between the body and the POSED body its pose came from (0 = POSED, -1 = none), "via" [B][F]: the joint,
    "rms_j" [B][F]; "rms", "n_used", "present": poses' own; "flag_posed" [B][F]: flag with JOINTED read as POSED -- what
    mocap_fill_rows is given here, and with it in the place of "flag" session_joint_motion sees a joint in those frames too;
    "pos", "vel", "acc", "quat_s", "omega", "res_rot", "flag_s": the smoothers' results as session_body_poses names them; with fill
    "filled" [R][F][3], "src" [R][F] and "from_joint" [R][F] bool: the rows filled from a JOINTED pose}."""
    joints = joints["joints"] if isinstance(joints, dict) else list(joints)
    if not joints:
        raise ValueError("session_joint_poses: no joints")
    for b, body in enumerate(bodies):
        if not isinstance(body, dict) or "rows" not in body or "markers" not in body:
            raise ValueError(f"session_joint_poses: body {b} has no 'rows': pass learn_session_bodies' list")
    traj = session["traj"]
    resident = getattr(traj, "is_cuda", False)
    n_min = min(int(degree) + 2, 2 * int(W) + 1) if n_min is None else int(n_min)
    par = (int(degree), int(W), float(span), n_min, int(max_gap))
    B = len(bodies)
    row_body = np.full(traj.shape[0], -1, dtype=np.int64)
    for b, body in enumerate(bodies):
        row_body[np.asarray(body["rows"], dtype=np.int64)] = b
    owned = np.flatnonzero(row_body >= 0)
    with _state["lock"]:
        core = get_core()
        if not resident:
            o = core.pose_joints(traj, bodies, poses["flag"], poses["quat"], poses["R"], poses["t_pose"], joints, axis_len=axis_len,
                                 max_rms=max_rms, max_rounds=max_rounds)
            posed = np.where(o["flag"] == capi.BP_JOINTED, capi.BP_POSED, o["flag"]).astype(np.int32)
            tr = core.smooth_tracks(t, o["t_pose"], *par)
            rot = core.smooth_rotations(t, o["quat"], *par)
            out = {**o, "rms": poses["rms"], "n_used": poses["n_used"], "present": poses["present"], "flag_posed": posed, "pos": tr["pos"],
                   "vel": tr["vel"], "acc": tr["acc"], "quat_s": rot["quat_s"], "omega": rot["omega"], "res_rot": rot["res"],
                   "flag_s": rot["flag"]}
            if fill:
                out.update(core.fill_rows(traj, bodies, posed, o["R"], o["t_pose"], rot["flag"], rot["quat_s"], tr["pos"]))
                out["from_joint"] = np.zeros(out["src"].shape, dtype=bool)
                out["from_joint"][owned] = (out["src"][owned] == capi.BP_SRC_RIGID) & (o["flag"][row_body[owned]] == capi.BP_JOINTED)
        else:
            import torch
            R, F = traj.shape[0], traj.shape[1]
            assert traj.dtype == torch.float64 and traj.is_contiguous() and traj.dim() == 3 and traj.shape[2] == 3
            if traj.device.index != core.device_id:
                raise ValueError(f"the session lives on {traj.device}, the core on GPU {core.device_id}: a resident session is read in place")
            dev = traj.device
            t = t if getattr(t, "is_cuda", False) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(dev)
            assert t.dtype == torch.float64 and t.is_contiguous() and t.numel() == F
            for k, n, dt in (("flag", 1, torch.int32), ("quat", 4, torch.float64), ("R", 9, torch.float64), ("t_pose", 3, torch.float64)):
                a = poses[k]
                assert a.is_cuda and a.device == dev and a.dtype == dt and a.is_contiguous() and a.numel() == B * F * n, k

            def f64(*shape):
                return torch.empty(shape, dtype=torch.float64, device=dev)

            def i32(*shape):
                return torch.empty(shape, dtype=torch.int32, device=dev)

            out = {"flag": i32(B, F), "hops": i32(B, F), "via": i32(B, F), "quat": f64(B, F, 4), "R": f64(B, F, 3, 3), "t_pose": f64(B, F, 3),
                   "rms_j": f64(B, F), "rms": poses["rms"], "n_used": poses["n_used"], "present": poses["present"], "pos": f64(B, F, 3),
                   "vel": f64(B, F, 3), "acc": f64(B, F, 3), "quat_s": f64(B, F, 4), "omega": f64(B, F, 3), "res_rot": f64(B, F),
                   "flag_s": i32(B, F)}
            ws = {"res": f64(B, F), "n_tr": i32(B, F), "flag_tr": i32(B, F), "n_rot": i32(B, F)}
            if fill:
                out.update(filled=f64(R, F, 3), src=i32(R, F))
            torch.cuda.current_stream(dev).synchronize()      # whatever torch itself still has queued on these buffers
            core.pose_joints_dev(F, R, traj.data_ptr(), bodies, poses["flag"].data_ptr(), poses["quat"].data_ptr(), poses["R"].data_ptr(),
                                 poses["t_pose"].data_ptr(), joints, axis_len, max_rms, max_rounds,
                                 *[out[k].data_ptr() for k in core.JOINT_POSE_OUT])
            core.smooth_tracks_dev(F, B, t.data_ptr(), out["t_pose"].data_ptr(), *par, out["pos"].data_ptr(), out["vel"].data_ptr(),
                                   out["acc"].data_ptr(), ws["res"].data_ptr(), ws["n_tr"].data_ptr(), ws["flag_tr"].data_ptr())
            core.smooth_rotations_dev(F, B, t.data_ptr(), out["quat"].data_ptr(), *par, out["quat_s"].data_ptr(),
                                      out["omega"].data_ptr(), out["res_rot"].data_ptr(), ws["n_rot"].data_ptr(), out["flag_s"].data_ptr())
            core.synchronize()                                # the mapped flag is torch's own arithmetic, on torch's stream
            jointed = out["flag"] == capi.BP_JOINTED
            out["flag_posed"] = torch.where(jointed, torch.full_like(out["flag"], capi.BP_POSED), out["flag"]).contiguous()
            if fill:
                torch.cuda.current_stream(dev).synchronize()
                core.fill_rows_dev(F, R, traj.data_ptr(), bodies, out["flag_posed"].data_ptr(), out["R"].data_ptr(), out["t_pose"].data_ptr(),
                                   out["flag_s"].data_ptr(), out["quat_s"].data_ptr(), out["pos"].data_ptr(), out["filled"].data_ptr(),
                                   out["src"].data_ptr())
                core.synchronize()
                at, of = torch.from_numpy(owned).to(dev), torch.from_numpy(row_body[owned]).to(dev)
                out["from_joint"] = torch.zeros((R, F), dtype=torch.bool, device=dev)
                out["from_joint"][at] = (out["src"][at] == capi.BP_SRC_RIGID) & jointed[of]
    return out


def session_skeleton_fit(t, session, bodies, poses_j, joints, axis_len=0.1, w_joint=1.0, iters=8, degree=2, W=8, span=float("inf"),
                         n_min=None, max_gap=0, fill=True):
    """All joints of a frame closed at once ("skeleton fit", include/mocap_core.h): mocap_fit_skeleton over session["traj"], the
    bodies, poses_j (session_joint_poses' dict, or session_body_poses') and joints (session_joints' dict or its list), then the
    two smoothers over the fitted tables and, with fill, mocap_fill_rows.  NumPy or resident: resident arrays are read in place and
    every result stays a torch tensor on that GPU.  Every body of a frame whose flag is BP_POSED or BP_JOINTED is fitted together
    with the others: the markers' residuals and, per joint between two such bodies, w_joint times the squared distance between the
    joint's two images (a hinge has a second point axis_len metres along its axis), by `iters` Levenberg-Marquardt passes.
    Returns a dict shaped like session_joint_poses': {"flag": poses_j's own; "quat", "R", "t_pose": the fitted poses (NaN where the
    body had none); "rms_s" [B][F]: each body's marker rms under them; "cost0", "cost" [F]: the frame's cost before and after;
    "steps" [F]: accepted passes; "n_act" [F]: joints with both bodies posed; "hops", "via", "rms_j", "rms", "n_used", "present":
    poses_j's own where it has them; "flag_posed" [B][F]: flag with JOINTED read as POSED; "pos", "vel", "acc", "quat_s", "omega",
    "res_rot", "flag_s": the smoothers' results; with fill "filled" [R][F][3] and "src" [R][F]}.  session_joint_motion reads the
    result directly."""
    joints = joints["joints"] if isinstance(joints, dict) else list(joints)
    if not joints:
        raise ValueError("session_skeleton_fit: no joints")
    for b, body in enumerate(bodies):
        if not isinstance(body, dict) or "rows" not in body or "markers" not in body:
            raise ValueError(f"session_skeleton_fit: body {b} has no 'rows': pass learn_session_bodies' list")
    traj = session["traj"]
    resident = getattr(traj, "is_cuda", False)
    n_min = min(int(degree) + 2, 2 * int(W) + 1) if n_min is None else int(n_min)
    par = (int(degree), int(W), float(span), n_min, int(max_gap))
    B = len(bodies)
    carried = {k: poses_j[k] for k in ("hops", "via", "rms_j", "rms", "n_used", "present") if k in poses_j}
    with _state["lock"]:
        core = get_core()
        if not resident:
            o = core.fit_skeleton(traj, bodies, poses_j["flag"], poses_j["quat"], poses_j["t_pose"], joints, axis_len=axis_len,
                                  w_joint=w_joint, iters=iters)
            flag = np.ascontiguousarray(poses_j["flag"], dtype=np.int32)
            posed = np.where(flag == capi.BP_JOINTED, capi.BP_POSED, flag).astype(np.int32)
            tr = core.smooth_tracks(t, o["t_pose"], *par)
            rot = core.smooth_rotations(t, o["quat"], *par)
            out = {**carried, **o, "flag": flag, "flag_posed": posed, "pos": tr["pos"], "vel": tr["vel"], "acc": tr["acc"],
                   "quat_s": rot["quat_s"], "omega": rot["omega"], "res_rot": rot["res"], "flag_s": rot["flag"]}
            if fill:
                out.update(core.fill_rows(traj, bodies, posed, o["R"], o["t_pose"], rot["flag"], rot["quat_s"], tr["pos"]))
        else:
            import torch
            R, F = traj.shape[0], traj.shape[1]
            assert traj.dtype == torch.float64 and traj.is_contiguous() and traj.dim() == 3 and traj.shape[2] == 3
            if traj.device.index != core.device_id:
                raise ValueError(f"the session lives on {traj.device}, the core on GPU {core.device_id}: a resident session is read in place")
            dev = traj.device
            t = t if getattr(t, "is_cuda", False) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(dev)
            assert t.dtype == torch.float64 and t.is_contiguous() and t.numel() == F
            for k, n, dt in (("flag", 1, torch.int32), ("quat", 4, torch.float64), ("t_pose", 3, torch.float64)):
                a = poses_j[k]
                assert a.is_cuda and a.device == dev and a.dtype == dt and a.is_contiguous() and a.numel() == B * F * n, k

            def f64(*shape):
                return torch.empty(shape, dtype=torch.float64, device=dev)

            def i32(*shape):
                return torch.empty(shape, dtype=torch.int32, device=dev)

            flag = poses_j["flag"]
            out = {**carried, "flag": flag, "quat": f64(B, F, 4), "R": f64(B, F, 3, 3), "t_pose": f64(B, F, 3), "rms_s": f64(B, F),
                   "cost0": f64(F), "cost": f64(F), "steps": i32(F), "n_act": i32(F), "pos": f64(B, F, 3), "vel": f64(B, F, 3),
                   "acc": f64(B, F, 3), "quat_s": f64(B, F, 4), "omega": f64(B, F, 3), "res_rot": f64(B, F), "flag_s": i32(B, F)}
            ws = {"res": f64(B, F), "n_tr": i32(B, F), "flag_tr": i32(B, F), "n_rot": i32(B, F)}
            if fill:
                out.update(filled=f64(R, F, 3), src=i32(R, F))
            out["flag_posed"] = torch.where(flag == capi.BP_JOINTED, torch.full_like(flag, capi.BP_POSED), flag).contiguous()
            torch.cuda.current_stream(dev).synchronize()      # whatever torch itself still has queued on these buffers
            core.fit_skeleton_dev(F, R, traj.data_ptr(), bodies, flag.data_ptr(), poses_j["quat"].data_ptr(), poses_j["t_pose"].data_ptr(),
                                  joints, axis_len, w_joint, iters, *[out[k].data_ptr() for k in core.SKELETON_FIT_OUT])
            core.smooth_tracks_dev(F, B, t.data_ptr(), out["t_pose"].data_ptr(), *par, out["pos"].data_ptr(), out["vel"].data_ptr(),
                                   out["acc"].data_ptr(), ws["res"].data_ptr(), ws["n_tr"].data_ptr(), ws["flag_tr"].data_ptr())
            core.smooth_rotations_dev(F, B, t.data_ptr(), out["quat"].data_ptr(), *par, out["quat_s"].data_ptr(),
                                      out["omega"].data_ptr(), out["res_rot"].data_ptr(), ws["n_rot"].data_ptr(), out["flag_s"].data_ptr())
            if fill:
                core.fill_rows_dev(F, R, traj.data_ptr(), bodies, out["flag_posed"].data_ptr(), out["R"].data_ptr(), out["t_pose"].data_ptr(),
                                   out["flag_s"].data_ptr(), out["quat_s"].data_ptr(), out["pos"].data_ptr(), out["filled"].data_ptr(),
                                   out["src"].data_ptr())
            core.synchronize()
    return out


def _bodies_core():
    """The registration lives in the context: a core handed over by set_core gets it on first use (callers hold the lock)."""
    core = get_core()
    reg = _state["bodies"]
    if reg is not None and getattr(core, "rigid_bodies_n", 0) != len(reg[0]):
        core.set_rigid_bodies(reg[1], tol=reg[2], max_rms=reg[3], work_cap=reg[4])
    return core


def _bodies_list(res, f=0):
    """One frame's found bodies: {"name", "R" 3x3, "t" [3], "rms", "markers": point index per marker, -1 = not seen}."""
    reg = _state["bodies"]
    if reg is None:
        return []
    return [{"name": reg[0][b], "R": res["R"][f, b].copy(), "t": res["t"][f, b].copy(), "rms": float(res["rms"][f, b]),
             "markers": res["assign"][f, b, :reg[1][b].shape[0]].astype(int).tolist()}
            for b in range(len(reg[0])) if res["found"][f, b]]


def locate_rigid_bodies(object_points):
    """The registered bodies among one frame's object points (at most 64): list of {"name", "R", "t", "rms", "markers"},
    world = R body + t, bodies that are not found left out."""
    P = np.asarray(object_points, dtype=np.float64).reshape(-1, 3)
    if P.shape[0] == 0 or _state["bodies"] is None:
        return []
    with _state["lock"]:
        res = _bodies_core().locate_rigid_bodies(P[None], [P.shape[0]])
    return _bodies_list(res)


def track_frame_bodies(image_points, camera_poses, is_locating_objects=True, O_max=8):
    """track_frame with the rigid-body stage in the same core call.  Returns (errors, object_points, objects, bodies):
    track_frame's three values and the list locate_rigid_bodies returns for the frame's object points; hand `bodies` to
    object_points_payload(..., bodies=bodies)."""
    for image_points_i in image_points:
        try:
            image_points_i.remove([None, None])
        except Exception:
            pass
    with _state["lock"]:
        core = _upload_cameras(camera_poses)
        _bodies_core()
        blobs, counts, _ = pack_frame(image_points)
        res = core.track_frame_bodies(blobs, counts, gate_px=5.0, O_max=O_max if is_locating_objects else 0)
    if int(res["status"][0]) != 0:
        raise capi.MocapError(_status_message(int(res["status"][0])))
    k = int(res["n_pts"][0])
    if k == 0:
        return np.array([]), np.array([]), [], []
    return (res["err"][0, :k].copy(), res["xyz"][0, :k].copy(), (_objects_list(res) if is_locating_objects else []),
            _bodies_list(res))


def set_body_tracker(gate=0.03, max_missed=10, vel_alpha=0.5, on=True):
    """Switches the body tracker on (mocap_set_body_tracker, include/mocap_core.h) and clears its slots: from now on
    track_bodies() / track_frame_bodies_tracked() follow every registered body from frame to frame -- a symmetric body keeps its
    labelling, a body with fewer than three visible markers coasts for up to max_missed frames, identical bodies keep their
    points.  gate = how far (in the unit of the object points) a marker may be from where the predicted pose puts it; vel_alpha
    in [0, 1] = weight of the newest velocity; on=False switches the tracker off.  Settings the core refuses raise
    capi.MocapError and change nothing."""
    with _state["lock"]:
        get_core().set_body_tracker(gate=gate, max_missed=max_missed, vel_alpha=vel_alpha, on=on)
        _state["body_tracker"] = (float(gate), int(max_missed), float(vel_alpha)) if on else None


def _tracked_core():
    """Registration and tracker live in the context: a core handed over by set_core gets both on first use (callers hold the lock)."""
    core = _bodies_core()
    reg = _state["body_tracker"]
    if reg is not None and getattr(core, "body_tracker", None) != reg:
        core.set_body_tracker(gate=reg[0], max_missed=reg[1], vel_alpha=reg[2])
    return core


_BT_SOURCE = {capi.BT_SRC_GUIDED: "guided", capi.BT_SRC_SEARCH: "search", capi.BT_SRC_COAST: "coast"}


def _tracked_list(res, f=0):
    """One frame's tracked bodies: {"name", "R" 3x3, "t" [3], "rms", "markers": point index per marker, -1 = not seen, "source":
    "guided" | "search" | "coast", "hits", "missed"}; a coasting body carries its predicted pose and no markers."""
    reg = _state["bodies"]
    if reg is None:
        return []
    return [{"name": reg[0][b], "R": res["bt_R"][f, b].copy(), "t": res["bt_t"][f, b].copy(), "rms": float(res["bt_rms"][f, b]),
             "markers": res["bt_assign"][f, b, :reg[1][b].shape[0]].astype(int).tolist(),
             "source": _BT_SOURCE[int(res["source"][f, b])], "hits": int(res["bt_hits"][f, b]), "missed": int(res["bt_missed"][f, b])}
            for b in range(len(reg[0])) if res["tracked"][f, b]]


def track_bodies(object_points, now=None):
    """The registered bodies among one frame's object points (at most 64), followed over time: list of {"name", "R", "t", "rms",
    "markers", "source", "hits", "missed"}, world = R body + t, bodies without a pose left out.  Frames are handed over in time
    order; `now` defaults to time.time().  Needs set_rigid_bodies() and set_body_tracker()."""
    now = time.time() if now is None else float(now)
    P = np.asarray(object_points, dtype=np.float64).reshape(-1, 3)
    n = P.shape[0]
    with _state["lock"]:
        res = _tracked_core().track_bodies([now], P[None] if n else np.zeros((1, 1, 3)), [n])
    return _tracked_list(res)


def track_frame_bodies_tracked(image_points, camera_poses, now=None, is_locating_objects=True, O_max=8):
    """track_frame_bodies with the body tracker in the same core call.  Returns (errors, object_points, objects, bodies):
    track_frame's three values and the list track_bodies returns for the frame's object points; hand `bodies` to
    object_points_payload(..., bodies=bodies).  `now` defaults to time.time()."""
    now = time.time() if now is None else float(now)
    for image_points_i in image_points:
        try:
            image_points_i.remove([None, None])
        except Exception:
            pass
    with _state["lock"]:
        core = _upload_cameras(camera_poses)
        _tracked_core()
        blobs, counts, _ = pack_frame(image_points)
        res = core.track_frame_bodies_tracked(blobs, counts, [now], gate_px=5.0, O_max=O_max if is_locating_objects else 0)
    if int(res["status"][0]) != 0:
        raise capi.MocapError(_status_message(int(res["status"][0])))
    k = int(res["n_pts"][0])
    if k == 0:   # (a body may coast through a frame without points)
        return np.array([]), np.array([]), [], _tracked_list(res)
    return (res["err"][0, :k].copy(), res["xyz"][0, :k].copy(), (_objects_list(res) if is_locating_objects else []),
            _tracked_list(res))


def set_marker_tracker(gate=0.05, max_missed=5, vel_alpha=0.5, T_max=64):
    """Switches the marker tracker on (mocap_set_marker_tracker, include/mocap_core.h) and clears its tracks: from now on
    track_markers() / track_frame_ids() give every object point an id that it keeps from frame to frame.  gate = how far (in the
    unit of the object points) a marker may be from its constant-velocity prediction; max_missed = frames it may go unseen;
    vel_alpha in [0, 1] = weight of the newest velocity; T_max = track slots (1 .. 64), 0 switches the tracker off.  Settings
    the core refuses raise capi.MocapError and change nothing."""
    with _state["lock"]:
        get_core().set_marker_tracker(gate=gate, max_missed=max_missed, vel_alpha=vel_alpha, T_max=T_max)
        _state["markers"] = (float(gate), int(max_missed), float(vel_alpha), int(T_max)) if int(T_max) else None


def _markers_core():
    """The tracker lives in the context: a core handed over by set_core gets the settings on first use (callers hold the lock)."""
    core = get_core()
    reg = _state["markers"]
    if reg is not None and getattr(core, "marker_tracker", None) != reg:
        core.set_marker_tracker(gate=reg[0], max_missed=reg[1], vel_alpha=reg[2], T_max=reg[3])
    return core


def track_markers(object_points, now=None):
    """The ids of one frame's object points (at most 64), in their order: list of int, -1 = the point has no track (not finite,
    or every track slot taken).  Frames are handed over in time order; `now` defaults to time.time().  Needs
    set_marker_tracker()."""
    now = time.time() if now is None else float(now)
    P = np.asarray(object_points, dtype=np.float64).reshape(-1, 3)
    n = P.shape[0]
    with _state["lock"]:
        res = _markers_core().track_markers([now], P[None] if n else np.zeros((1, 1, 3)), [n])
    return res["id"][0, :n].astype(int).tolist()


def track_frame_ids(image_points, camera_poses, now=None, is_locating_objects=True, O_max=8):
    """track_frame with the marker tracker in the same core call.  Returns (errors, object_points, objects, ids): track_frame's
    three values and the list track_markers returns for the frame's object points.  `now` defaults to time.time()."""
    now = time.time() if now is None else float(now)
    for image_points_i in image_points:
        try:
            image_points_i.remove([None, None])
        except Exception:
            pass
    with _state["lock"]:
        core = _upload_cameras(camera_poses)
        _markers_core()
        blobs, counts, _ = pack_frame(image_points)
        res = core.track_frame_ids(blobs, counts, [now], gate_px=5.0, O_max=O_max if is_locating_objects else 0)
    if int(res["status"][0]) != 0:
        raise capi.MocapError(_status_message(int(res["status"][0])))
    k = int(res["n_pts"][0])
    if k == 0:
        return np.array([]), np.array([]), [], []
    return (res["err"][0, :k].copy(), res["xyz"][0, :k].copy(), (_objects_list(res) if is_locating_objects else []),
            res["id"][0, :k].astype(int).tolist())


def _filtered_list(res, f=0):
    """One frame's `filtered_objects` as the reference builds it (KalmanFilter.py:93-98): drones in ascending index, absent ones left out."""
    return [{"pos": res["fpos"][f, d].copy(), "vel": res["fvel"][f, d].copy(), "heading": float(res["fheading"][f, d]),
             "droneIndex": int(d)}
            for d in range(res["chosen"].shape[1]) if res["chosen"][f, d] >= 0]


class KalmanFilter:
    """The reference's KalmanFilter (computer_code/api/KalmanFilter.py) with its state on the device: same constructor, same
    predict_location(objects) / reset() seam, so it drops into Cameras.kalman_filter (helpers.py:175).  The filter lives in the
    core's context (one per context: constructing another one re-initialises it); `now` defaults to time.time() like the
    reference, pass it for a reproducible run.  Constructor defaults as there: 5th-order Butterworth, 20 Hz cut-off at 60 Hz,
    buffers of 300."""

    def __init__(self, num_objects, cutoff_frequency=20, sampling_frequency=60.0, order=5, buffer_size=300):
        from scipy.signal import butter
        self.num_objects = int(num_objects)
        b, a = butter(order, cutoff_frequency / (sampling_frequency / 2), btype="low")
        with _state["lock"]:
            get_core().set_object_filter(self.num_objects, b, a, buffer_size=buffer_size)

    def predict_location(self, objects, now=None):
        """objects: locate_objects' list for one frame -> [{"pos" float32[3], "vel" float32[3], "heading" float, "droneIndex" int}]."""
        now = time.time() if now is None else float(now)
        O = max(1, len(objects))
        pos = np.zeros((1, O, 3))
        heading = np.zeros((1, O))
        drone = np.full((1, O), -1, dtype=np.int32)
        for j, obj in enumerate(objects):
            pos[0, j] = np.asarray(obj["pos"], dtype=np.float64).reshape(3)
            heading[0, j] = float(obj["heading"])
            drone[0, j] = int(obj["droneIndex"])
        with _state["lock"]:
            res = get_core().filter_objects([now], pos, heading, drone, [len(objects)])
        return _filtered_list(res)

    def reset(self, now=None):
        with _state["lock"]:
            get_core().reset_object_filter(time.time() if now is None else float(now))


def track_frame_filtered(image_points, camera_poses, now=None, O_max=8):
    """track_frame() plus helpers.py:109 in the same core call: returns (errors, object_points, objects, filtered_objects), the
    four values object_points_payload() takes.  Needs a KalmanFilter(num_objects) to have been constructed (Cameras.
    start_trangulating_points does, helpers.py:175); `now` defaults to time.time()."""
    now = time.time() if now is None else float(now)
    for image_points_i in image_points:
        try:
            image_points_i.remove([None, None])
        except Exception:
            pass
    with _state["lock"]:
        core = _upload_cameras(camera_poses)
        blobs, counts, _ = pack_frame(image_points)
        res = core.track_frame_filtered(blobs, counts, [now], gate_px=5.0, O_max=O_max)
    if int(res["status"][0]) != 0:
        raise capi.MocapError(_status_message(int(res["status"][0])))
    k = int(res["n_pts"][0])
    return res["err"][0, :k].copy(), res["xyz"][0, :k].copy(), _objects_list(res), _filtered_list(res)


def camera_read_track(raw_frames, camera_poses, M_max=16, is_locating_objects=True, O_max=8, want_jpeg=False, quality=95):
    """Raw camera frames -> (image_points, errors, object_points, objects): Cameras._camera_read's preprocessing,
    _find_dot, the frame path, the world transform and locate_objects (helpers.py:68-108) in one core call; nothing but the
    payload crosses PCIe on the way back.  image_points is what _find_dot returns per camera ([[None, None]] when a
    camera saw nothing).  want_jpeg=True appends the preview stream's frame (get_frames_jpeg's bytes, same call, same wait)
    as a fifth element."""
    raw = np.ascontiguousarray(np.asarray(raw_frames, dtype=np.uint8))
    C, rows, cols = raw.shape[0], raw.shape[1], raw.shape[2]
    params = _state["camera_params"]
    if params is None or len(params) < C:
        raise RuntimeError("set_camera_params() has not been called with one entry per camera")
    K = np.array([np.array(params[i]["intrinsic_matrix"], dtype=np.float64) for i in range(C)])
    dist = np.array([np.array(params[i]["distortion_coef"], dtype=np.float64).ravel()[:5] for i in range(C)])
    rot = np.array([int(params[i].get("rotation", 0)) for i in range(C)], dtype=np.int32)
    with _state["lock"]:
        core = _apply_overlay(_upload_cameras(camera_poses))
        key = (rows, cols, K.tobytes(), dist.tobytes(), rot.tobytes())
        if _state["img_key"] != key:
            core.set_image_params(rows, cols, K, dist, rot)
            _state["img_key"] = key
        while True:
            if want_jpeg:
                res = core.track_frame_images_jpeg(raw[None], M_max=M_max, O_max=O_max if is_locating_objects else 0, quality=quality)
            else:
                res = core.track_frame_images(raw[None], M_max=M_max, O_max=O_max if is_locating_objects else 0)
            if (res["blob_status"] & capi.BLOB_ST_POINT_OVERFLOW).any() and M_max < 256:   # more dots than slots: ask again
                M_max = min(256, 4 * M_max)
                continue
            break
    if (res["blob_status"] & capi.BLOB_ST_CAP_OVERFLOW).any():
        raise capi.MocapError("more contours than the blob stage's largest tables hold (BLOB_ST_CAP_OVERFLOW)")
    if int(res["status"][0]) != 0:
        raise capi.MocapError(f"frame exceeds the core's limits (status {int(res['status'][0])})")
    image_points = []
    for c in range(C):
        image_points.append(_points_list(core, res["blobs"][0, c], int(res["counts"][0, c])))
    tail = (res["jpeg"][0],) if want_jpeg else ()
    k = int(res["n_pts"][0])
    if k == 0:
        return (image_points, np.array([]), np.array([]), []) + tail
    return (image_points, res["err"][0, :k].copy(), res["xyz"][0, :k].copy(),
            _objects_list(res) if is_locating_objects else []) + tail


def object_points_payload(errors, object_points, objects, filtered_objects=(), bodies=None):
    """The dict the reference emits as the `object-points` socket event (helpers.py:128-133), built from what
    track_frame() / camera_read_track() / track_frame_filtered() return.  `filtered_objects` is KalmanFilter.predict_location's
    list (or track_frame_filtered's fourth value); its "pos" and "vel" arrays are .tolist()-ed like helpers.py:124-126 does,
    entries a caller has already converted pass through.  `bodies` (track_frame_bodies' fourth value; the reference has no such
    field) adds a "bodies" list of {"name", "R", "t", "rms", "markers"}; without it the dict is the reference's."""
    as_json = lambda d: {k: (v.tolist() if isinstance(v, np.ndarray) else v) for (k, v) in d.items()}   # noqa: E731
    payload = {
        "object_points": np.asarray(object_points).tolist(),
        "errors": np.asarray(errors).tolist(),
        "objects": [as_json(obj) for obj in objects],
        "filtered_objects": [as_json(obj) for obj in filtered_objects],
    }
    if bodies is not None:
        payload["bodies"] = [as_json(body) for body in bodies]
    return payload


def _status_message(st):
    """What a frame's status word says once the core's worst-case re-submit has run (include/mocap_core.h MOCAP_ST_*)."""
    if st & capi.ST_INTRACTABLE:
        lg = (st >> capi.ST_LOG2_GROUPS_SHIFT) & capi.ST_LOG2_GROUPS_MASK
        return (f"frame has a root with about 2^{lg} candidate groups (status {st}): the reference would enumerate all of them "
                "(helpers.py:394-400) and never return; no enumeration reaches it and the exact search could not bound it")
    return (f"frame exceeds the core's limits (status {st}): candidate groups / roots over the caps of include/mocap_core.h")


# ----------------------------------------------------------------------------- initial poses (caller of BA)
def initial_camera_poses(image_points):
    """The pose-chaining loop of the `calculate-camera-pose` handler (index.py:234-270): `image_points` is
    the handler's np.array(data["cameraPoints"]) -- (N, C, 2) with None for unseen -- and the result the
    list of {"R": 3x3, "t": (3, 1)} it hands to bundle_adjustment (camera 0 = identity)."""
    arr = np.asarray(image_points, dtype=object)
    C = arr.shape[1]
    obs = _obs_array(arr, C)
    K = _intrinsics(C)
    with _state["lock"]:
        R, t, _ = get_core().initial_poses(obs, K)
    return [{"R": R[i], "t": t[i].reshape(3, 1)} for i in range(C)]


def calculate_camera_pose(data, socketio):
    """index.py:229-281 end to end: initial poses, bundle_adjustment, final error, the `camera-pose` event."""
    image_points = np.array(data["cameraPoints"], dtype=object)
    camera_poses = initial_camera_poses(image_points)
    camera_poses = bundle_adjustment(image_points, camera_poses, socketio)
    object_points = triangulate_points(image_points, camera_poses)
    error = float(np.mean(calculate_reprojection_errors(image_points, object_points, camera_poses)))
    socketio.emit("camera-pose", {"camera_poses": camera_pose_to_serializable(camera_poses)})
    return camera_poses, error


# ----------------------------------------------------------------------------- camera resection (one camera re-seated)
def _resection_inputs(image_points, camera_poses, camera):
    """One camera against the rig's own points: the capture's points triangulated and refined WITHOUT that camera (its column
    blanked: every point needs two other cameras), and where the camera saw them -> (core, X [N][3] NaN for no point, obs [N][2],
    K [3][3], prior (R, t) or None).  Caller holds the lock."""
    C = len(camera_poses)
    if C < 3:
        raise ValueError("camera resection needs at least 3 cameras: the points must come from two others")
    if not 0 <= int(camera) < C:
        raise IndexError("camera index out of range")
    camera = int(camera)
    has_pose = camera_poses[camera] is not None
    poses = list(camera_poses)
    if not has_pose:
        poses[camera] = {"R": np.eye(3), "t": np.zeros(3)}    # its column is blanked: the placeholder is never used
    obs = _obs_array(image_points, C)
    if obs.shape[0] == 0:
        raise ValueError("camera resection needs a capture: image_points is empty")
    blanked = obs.copy()
    blanked[:, camera] = np.nan
    core = _upload_cameras(poses)
    X, _, _ = core.triangulate_refined(blanked, iters=_state["refine"] or 4)
    R, t = _pose_arrays(poses)
    return core, X, obs[:, camera].copy(), _intrinsics(C)[camera], ((R[camera], t[camera]) if has_pose else None)


def reseat_camera(image_points, camera_poses, camera, threshold_px=2.0, n_hyp=256, seed=0, min_inliers=6, max_iter=20):
    """Re-seat ONE camera of a calibrated rig -- it was knocked, or it is new -- from a capture (`capture-points` payload,
    [N][C][2] with None for unseen), keeping the rig's scale, frame and world transform (mocap_resect_camera, include/mocap_core.h
    "camera resection"): the 3-D points are the capture's points built WITHOUT that camera (triangulate_points_refined with its
    column blanked, so C >= 3), its pose in camera_poses -- None for a new camera -- is the prior, its intrinsic matrix the one from
    set_camera_params.

    Returns (camera_poses, report): the pose list with that camera replaced, and the solver's info fields by name plus "camera" and
    "R", "t" (the resected pose in the frame the poses came in).
    When the status is not capi.RESECT_OK the poses come back as they were.  Camera 0 defines the rig's frame: the result is
    re-gauged so that it stays (I, 0) -- with (R0, t0) its resected pose in the old frame every camera becomes R_c R0^T,
    t_c - R_c R0^T t0 -- and report["to_world_right"] is the 4 x 4 matrix to right-multiply onto to_world_coords_matrix so that
    world coordinates do not move (D R0^T D | -D R0^T t0 with D = diag(-1, -1, 1) of set_to_world_coords_matrix's convention)."""
    with _state["lock"]:
        core, X, obs, K, prior = _resection_inputs(image_points, camera_poses, camera)
        R, t, _, info = core.resect_camera(X, obs, K, prior=prior, threshold_px=threshold_px, n_hyp=n_hyp, seed=seed,
                                           min_inliers=min_inliers, max_iter=max_iter)
    camera = int(camera)
    report = dict(info, camera=camera, R=R, t=t)        # the resected pose in the frame the poses came in
    poses =[None if p is None else {"R": np.array(p["R"], dtype=np.float64).reshape(3, 3), "t": np.array(p["t"], dtype=np.float64).reshape(3)}
             for p in camera_poses]
    if info["status"] != capi.RESECT_OK:
        return poses, report
    if camera != 0:
        poses[camera] = {"R": R, "t": t}
        return poses, report
    for c in range(1, len(poses)):
        Rc = poses[c]["R"] @ R.T
        poses[c] = {"R": Rc, "t": poses[c]["t"] - Rc @ t}
    poses[0] = {"R": np.eye(3), "t": np.zeros(3)}
    D = np.diag([-1.0, -1.0, 1.0])
    M = np.eye(4)
    M[:3, :3] = D @ R.T @ D
    M[:3, 3] = -D @ R.T @ t
    report["to_world_right"] = M
    return poses, report


def camera_health(image_points, camera_poses, threshold_px=2.0):
    """Which camera was knocked?  Every camera's reprojection error against points built WITHOUT it (the evaluate-only mode of
    mocap_resect_camera: nothing is searched or refined).  Returns one dict per camera: "rms" (pixels, over all its views of such
    points that lie in front of it), "inlier_share" (views within threshold_px) and "views".  The camera with the largest rms is
    the one to hand to reseat_camera."""
    out = []
    with _state["lock"]:
        for c in range(len(camera_poses)):
            core, X, obs, K, prior = _resection_inputs(image_points, camera_poses, c)
            if prior is None:
                raise ValueError("camera_health needs a pose for every camera")
            _, _, _, near = core.resect_camera(X, obs, K, prior=prior, threshold_px=threshold_px, n_hyp=0, min_inliers=4, max_iter=0)
            _, _, _, wide = core.resect_camera(X, obs, K, prior=prior, threshold_px=1e9, n_hyp=0, min_inliers=4, max_iter=0)
            out.append({"rms": wide["rms_final"], "inlier_share": near["inliers"] / near["valid"] if near["valid"] else 0.0,
                        "views": near["valid"]})
    return out


# ----------------------------------------------------------------------------- calibration tail (scale, floor, origin)
def _pack_object_points(object_points):
    """The UI's ragged objectPoints (per frame a list of [x, y, z]) -> (xyz [F][K_max][3] NaN-padded, n_pts [F])."""
    F = len(object_points)
    K_max = max([1] + [len(frame) for frame in object_points])
    xyz = np.full((F, K_max, 3), np.nan)
    n_pts = np.zeros(F, dtype=np.int32)
    for f, frame in enumerate(object_points):
        if len(frame):
            xyz[f, :len(frame)] = np.asarray(frame, dtype=np.float64).reshape(-1, 3)
        n_pts[f] = len(frame)
    return xyz, n_pts


def _capture_call(object_points, host_fn, dev_fn, n_result):
    """Runs one of the calibration-tail reductions over a capture and returns its `n_result` doubles (host_fn and dev_fn both
    produce exactly that many).  object_points: the UI's
    ragged list, or a dict {"xyz" [F][K_max][3], "n_out" | "n_pts" [F], "status" [F] (optional)} as
    find_point_correspondance_and_object_points_batch returns it (NumPy arrays), or the same dict of torch tensors on the GPU
    (the buffers track_frame_dev wrote): those are read in place, only the result crosses PCIe."""
    if not isinstance(object_points, dict):
        xyz, n_pts = _pack_object_points(object_points)
        return host_fn(xyz, n_pts, None)
    xyz = object_points["xyz"]
    n_pts = object_points["n_pts"] if "n_pts" in object_points else object_points["n_out"]
    status = object_points.get("status")
    if not getattr(xyz, "is_cuda", False):
        return host_fn(np.asarray(xyz), np.asarray(n_pts), None if status is None else np.asarray(status))
    import torch
    assert xyz.dtype == torch.float64 and xyz.is_contiguous() and xyz.dim() == 3 and xyz.shape[2] == 3
    assert n_pts.dtype == torch.int32 and n_pts.is_contiguous() and n_pts.is_cuda and n_pts.numel() == xyz.shape[0]
    assert status is None or (status.dtype == torch.int32 and status.is_contiguous() and status.is_cuda and status.numel() == xyz.shape[0])
    core = get_core()
    if xyz.device.index != core.device_id or n_pts.device != xyz.device or (status is not None and status.device != xyz.device):
        raise ValueError(f"the capture lives on {xyz.device}, the core on GPU {core.device_id}: a resident capture is read in place")
    torch.cuda.current_stream(xyz.device).synchronize()      # whatever torch itself still has queued on these buffers
    result = torch.empty(n_result, dtype=torch.float64, device=xyz.device)
    dev_fn(core, xyz.shape[0], xyz.shape[1], xyz.data_ptr(), n_pts.data_ptr(), 0 if status is None else status.data_ptr(),
           result.data_ptr())
    core.synchronize()
    return result.cpu().numpy()


def _scale_result(res):
    """MocapCore.determine_scale's dict -> the 4 doubles of mocap_determine_scale's `result`."""
    return np.array([res["scale_factor"], res["mean_distance"], res["pairs"], res["skipped"]], dtype=np.float64)


def determine_scale(data, socketio, actual_distance=0.15):
    """index.py:290-309, the `determine-scale` handler: data = {"objectPoints", "cameraPoses"}; emits `camera-pose` with
    {"error": None, "camera_poses": ...}, every t multiplied by actual_distance / mean(pair distance).  Returns
    (camera_poses, scale_factor).  No two-point frame at all: the factor is NaN, as in the reference."""
    camera_poses = data["cameraPoses"]
    with _state["lock"]:
        res = _capture_call(
            data["objectPoints"],
            lambda xyz, n, st: _scale_result(get_core().determine_scale(xyz, n, st, actual_distance)),
            lambda core, F, K, d_xyz, d_n, d_st, d_res: core.determine_scale_dev(F, K, d_xyz, d_n, d_st, actual_distance, 0, d_res), 4)
    scale_factor = float(res[0])
    for i in range(0, len(camera_poses)):
        camera_poses[i]["t"] = (np.array(camera_poses[i]["t"]) * scale_factor).tolist()     # index.py:307
    if socketio is not None:
        socketio.emit("camera-pose", {"error": None, "camera_poses": camera_poses})
    return camera_poses, scale_factor


def acquire_floor(data, socketio):
    """index.py:158-194, the `acquire-floor` handler: data = {"objectPoints"}; the plane through every captured point, the
    rotation that lays it flat -> set_to_world_coords_matrix + the `to-world-coords-matrix` event.  Returns (matrix, info) with
    info = {"a", "b", "c", "points", "rms_residual", "tilt", "degenerate"}; "degenerate" is True when the floor is parallel to
    the xy-plane (the reference's rotation is then noise-determined; the matrix is emitted as the arithmetic gives it).  Fewer
    than 3 points or collinear points raise MocapError (include/mocap_core.h, mocap_floor_from_factor)."""
    with _state["lock"]:
        factor = _capture_call(data["objectPoints"], lambda xyz, n, st: get_core().floor_factor(xyz, n, st),
                               lambda core, F, K, d_xyz, d_n, d_st, d_res: core.floor_factor_dev(F, K, d_xyz, d_n, d_st, d_res), 17)
        to_world, info, rc = get_core().floor_from_factor(factor)
    info["degenerate"] = rc != capi.MOCAP_OK
    set_to_world_coords_matrix(to_world)
    if socketio is not None:
        socketio.emit("to-world-coords-matrix", {"to_world_coords_matrix": to_world.tolist()})
    return to_world, info


def set_origin(data, socketio):
    """index.py:197-210, the `set-origin` handler: data = {"objectPoint", "toWorldCoordsMatrix"}; the matrix translated by the
    point (y and z swapped) -> set_to_world_coords_matrix + the `to-world-coords-matrix` event.  Returns the matrix."""
    to_world = capi.world_set_origin(data["toWorldCoordsMatrix"], data["objectPoint"])
    set_to_world_coords_matrix(to_world)
    if socketio is not None:
        socketio.emit("to-world-coords-matrix", {"to_world_coords_matrix": to_world.tolist()})
    return to_world


# ----------------------------------------------------------------------------- bundle adjustment
def _ba_x0(camera_poses):
    """helpers.py:278-285 (including its focal-length indexing: entry i+1 takes camera i's focal)."""
    from scipy.spatial.transform import Rotation
    K = _intrinsics(len(camera_poses))
    x0 = [K[0][0, 0]]
    for i, pose in enumerate(camera_poses[1:]):
        rot_vec = Rotation.from_matrix(np.asarray(pose["R"], dtype=np.float64)).as_rotvec().flatten()
        x0 += [K[i][0, 0]] + rot_vec.tolist() + np.asarray(pose["t"], dtype=np.float64).flatten().tolist()
    return np.array(x0, dtype=np.float64)


def _params_to_camera_poses(params):
    """helpers.py:247-262."""
    from scipy.spatial.transform import Rotation
    C = int((params.size - 1) / 7) + 1
    poses = [{"R": np.eye(3), "t": np.array([0, 0, 0], dtype=np.float32)}]
    for i in range(C - 1):
        poses.append({"R": Rotation.from_rotvec(params[i * 7 + 2:i * 7 + 5]).as_matrix(),
                      "t": params[i * 7 + 5:i * 7 + 8]})
    return poses


def camera_pose_to_serializable(camera_poses):
    """helpers.py:526-530."""
    return [{k: np.asarray(v).tolist() for k, v in p.items()} for p in camera_poses]


def bundle_adjustment(image_points, camera_poses, socketio, return_info=False):
    """helpers.py:244-290: least_squares(residual_function, x0, loss="cauchy", ftol=1e-2).

    mode "scipy" (default): the reference's optimizer call verbatim, only the residual evaluations are GPU -- poses
    bit-identical to the reference's on the solver goldens.
    mode "resident": the whole trust-region loop runs in the core (mocap_ba_solve), milliseconds instead of seconds;
    inside the reference's own reproducibility, see DEFAULT_BA_MODE above.
    `socketio.emit("camera-pose", ...)`: the reference streams one per residual evaluation (helpers.py:274; the UI
    animates the cameras while calibrating, App.tsx:255).  Mode "scipy" does exactly that; mode "resident" has no
    per-evaluation host round trip and emits once per accepted step (1 / (n + 2) as often), then the final poses."""
    C = len(camera_poses)
    x0 = _ba_x0(camera_poses)
    obs = _obs_array(image_points, C)
    R, t = _pose_arrays(camera_poses)
    K = _intrinsics(C)

    def emit(params):
        if socketio is not None:
            socketio.emit("camera-pose", {"camera_poses": camera_pose_to_serializable(_params_to_camera_poses(params))})

    # The solve runs on bundle adjustment's OWN context: the module lock -- the one every frame call takes -- is held only to
    # fetch that context, never across a residual evaluation, let alone the whole solve.
    with _state["lock"]:
        core = _ba_core()
        mode = _state["ba_mode"]
        f32_rounding = get_core().f32_rounding      # options live in a context: the calibration's follows the frame path's
    with _state["ba_lock"]:
        if core.f32_rounding != f32_rounding:
            core.set_options(f32_rounding=f32_rounding)
        core.set_cameras(K, R, t)
        if mode == "resident":
            core.set_ba_progress(emit if socketio is not None else None)
            try:
                x, info = core.ba_solve(x0, obs, ftol=1e-2, f32_residuals=True, use_cauchy=True)
            finally:
                core.set_ba_progress(None)
        else:
            from scipy import optimize
            # SciPy's own step rule for jac='2-point' (a PRIVATE helper: its 4-argument form exists in SciPy 1.5 .. 1.15; checked
            # here, not assumed).  Anything else -- import error, another signature, a step that is not what approx_derivative
            # would take -- falls back to jac='2-point' (the reference's call verbatim: n + 1 separate residual evaluations)
            _compute_absolute_step = None
            try:
                import inspect
                from scipy.optimize._numdiff import _compute_absolute_step as _cas
                if list(inspect.signature(_cas).parameters)[:4] == ["rel_step", "x0", "f0", "method"]:
                    probe = _cas(None, np.array([1.0, -2.0, 0.0]), np.zeros(2, dtype=np.float32), "2-point")
                    eps32 = float(np.finfo(np.float32).eps) ** 0.5
                    if np.allclose(probe, [eps32, -2.0 * eps32, eps32], rtol=1e-12, atol=0.0):
                        _compute_absolute_step = _cas
            except Exception:
                _compute_absolute_step = None

            last = {"x": None, "r": None}
            spent = {"core_s": 0.0}                             # wall time inside the core's calls (the rest is SciPy's own)

            def residual_function(params):
                t0 = time.perf_counter()
                r = core.ba_residuals(params, obs)[0]
                spent["core_s"] += time.perf_counter() - t0
                emit(params)                                    # helpers.py:274
                r = r[~np.isnan(r)].astype(np.float32)          # helpers.py:273
                last["x"], last["r"] = np.array(params, dtype=np.float64), r
                return r

            def jacobian(params):
                """The Jacobian least_squares would difference itself (jac='2-point': scipy _numdiff.approx_derivative ->
                _dense_difference), with its n residual evaluations made by ONE call of the core: the n perturbed parameter
                vectors x + h_i e_i go through mocap_ba_residuals as a batch.  Same step vector (SciPy's own
                _compute_absolute_step: float32 residuals -> sqrt(eps_float32) relative step), same residual bits (the batch
                is the single call's kernel per parameter vector), same NumPy expressions for `df / dx` (float32
                difference, float64 quotient) => the same J bit for bit, hence the same iterates, nfev, njev and poses as
                the reference's call on the solver goldens (tests/test_gpu_ba.py).  The reference's residual_function
                emits the poses at every one of those evaluations (helpers.py:274): so does this."""
                x0_ = np.array(params, dtype=np.float64)
                if last["x"] is not None and np.array_equal(last["x"], x0_):
                    f0 = last["r"]                              # trf hands approx_derivative the f it just evaluated at x
                    X = np.repeat(x0_[None, :], x0_.size, axis=0)
                    first = 0
                else:                                           # (not reached from trf: f0 rides along in the batch)
                    X = np.repeat(x0_[None, :], x0_.size + 1, axis=0)
                    first = 1
                    f0 = None
                h = _compute_absolute_step(None, x0_, last["r"] if f0 is None else f0, "2-point")
                idx = np.arange(x0_.size)
                X[first + idx, idx] = x0_ + h                   # x1[i] += h[i]
                dx = X[first + idx, idx] - x0_                  # "recompute dx as exactly representable number"
                t0 = time.perf_counter()
                R = core.ba_residuals(X, obs)
                spent["core_s"] += time.perf_counter() - t0
                if f0 is None:
                    f0 = R[0][~np.isnan(R[0])].astype(np.float32)
                J_T = np.empty((x0_.size, f0.size))
                for i in range(x0_.size):
                    emit(X[first + i])
                    ri = R[first + i]
                    df = ri[~np.isnan(ri)].astype(np.float32) - f0   # (a mask that moved raises here, as it would in the reference)
                    J_T[i] = df / dx[i]
                return J_T.T

            use_batched = os.environ.get("MOCAP_BA_BATCHED_JAC", "1") != "0" and _compute_absolute_step is not None
            import contextlib
            blas = contextlib.nullcontext()
            if _state["ba_blas_threads"] is not None:
                try:
                    from threadpoolctl import threadpool_limits
                    blas = threadpool_limits(limits=_state["ba_blas_threads"])
                except Exception:
                    pass
            with blas:
                res = optimize.least_squares(residual_function, x0, jac=jacobian if use_batched else "2-point", verbose=0,
                                             loss="cauchy", ftol=1e-2)
            x, info = res.x, {"iterations": res.njev, "njev": res.njev, "nfev": res.nfev, "status": res.status,
                       "cost": res.cost, "optimality": res.optimality, "core_s": spent["core_s"]}
    poses = _params_to_camera_poses(x)
    if socketio is not None:
        socketio.emit("camera-pose", {"camera_poses": camera_pose_to_serializable(poses)})
    return (poses, info) if return_info else poses


def bundle_adjustment_joint(image_points, camera_poses, socketio=None, refine_focal=False, huber_px=0.0, max_iter=50, ftol=1e-10,
                            return_info=False):
    """The core's own calibration refinement (mocap_ba_joint_solve, include/mocap_core.h "joint bundle adjustment"): the poses of
    cameras 1 .. C-1 and every 3-D point as unknowns -- with refine_focal also one focal scale per camera, which needs three
    cameras -- the true reprojection error with each camera's own K, analytic Jacobians, a Huber cost at huber_px (0 = off).
    Opt-in, beside bundle_adjustment: that function, its two modes and DEFAULT_BA_MODE are what they were.

    Returns camera_poses in the reference's dict shape ({"R": 3x3, "t": 3}; camera 0 as it came, |t_1| as it came: the scale
    determine_scale set survives); with refine_focal (poses, scales); with return_info the solver's info dict last.  Runs on bundle
    adjustment's own context under its lock, like bundle_adjustment; `socketio.emit("camera-pose", ...)` once per accepted step, then
    the final poses."""
    C = len(camera_poses)
    if refine_focal and C < 3:
        raise ValueError("refine_focal needs at least 3 cameras: with two, the scale of the focal lengths is not observable")
    if not (np.isfinite(huber_px) and huber_px >= 0 and np.isfinite(ftol) and ftol >= 0 and int(max_iter) >= 1):
        raise ValueError("huber_px and ftol must be finite and >= 0, max_iter at least 1")
    obs = _obs_array(image_points, C)
    R, t = _pose_arrays(camera_poses)
    K = _intrinsics(C)

    def emit(params):
        socketio.emit("camera-pose", {"camera_poses": camera_pose_to_serializable(_params_to_camera_poses(params))})

    with _state["lock"]:
        core = _ba_core()
    with _state["ba_lock"]:
        core.set_cameras(K, R, t)
        core.set_ba_progress(emit if socketio is not None else None)
        try:
            R1, t1, scales, _, info = core.ba_joint_solve(obs, R, t, refine_focal=refine_focal, huber_px=huber_px, ftol=ftol,
                                                          max_iter=max_iter)
        finally:
            core.set_ba_progress(None)
    poses = [{"R": R1[c].copy(), "t": t1[c].copy()} for c in range(C)]
    if socketio is not None:
        socketio.emit("camera-pose", {"camera_poses": camera_pose_to_serializable(poses)})
    out = (poses,) + ((scales,) if refine_focal else ()) + ((info,) if return_info else ())
    return out[0] if len(out) == 1 else out


def _lens_arrays(C):
    """K [C][3][3] and dist [C][5] of the camera params; a camera without "distortion_coef" has zeros."""
    K = _intrinsics(C)
    params = _state["camera_params"]
    dist = np.zeros((C, 5))
    for c in range(C):
        d = np.asarray(params[c].get("distortion_coef", [0.0] * 5), dtype=np.float64).ravel()
        dist[c, :min(5, d.size)] = d[:5]
    return K, dist


def calibrate_lenses(image_points, camera_poses, refine=("focal", "centre", "radial"), huber_px=0.0, max_iter=100, ftol=1e-10,
                     return_info=False):
    """Lens calibration from a wand capture (mocap_ba_lens_solve, include/mocap_core.h "lens calibration"): the poses of cameras
    1 .. C-1, every 3-D point and, per camera, the intrinsics named in `refine` -- "focal" (fx, fy), "centre" (cx, cy), "radial"
    (k1, k2), "tangential" (p1, p2), or an integer of capi.BAL_* bits -- as unknowns of one bundle adjustment.  Needs three cameras.  The start is the camera params
    as set_camera_params has them (nominal values do: the data sheet's focal length, the picture's centre, zero distortion).

    THE CAPTURE: image_points are `capture-points` rows taken RAW, i.e. with distortion_coef = 0 in the camera params while
    capturing, so that the blob stage does not undistort with a lens nobody knows yet; and the wand must FILL THE IMAGES, out to
    the corners of every camera's picture.  Points that cover only the middle of the pictures do not determine a lens: the solver
    still returns, with intrinsics that are worth nothing (DESIGN 3.7r has the figures).

    Returns (camera_poses, camera_params): poses in the reference's dict shape (camera 0 and |t_1| as they came), and a list of
    {"intrinsic_matrix": 3x3 list, "distortion_coef": [k1, k2, p1, p2, k3]} in camera-params.json's convention, ready for
    set_camera_params (other keys of the current params, like "rotation", are kept); with return_info the solver's info dict
    last.  undistort_image_points(image_points, camera_params) then turns the same raw capture into what determine_scale,
    acquire_floor, bundle_adjustment_joint and reseat_camera take."""
    C = len(camera_poses)
    try:
        flags = capi.MocapCore.bal_flags(refine)
    except capi.MocapError as e:
        raise ValueError(str(e))
    if flags & ~15:
        raise ValueError(f"unknown bits in refine: {flags:#x}")
    if flags and C < 3:
        raise ValueError("lens calibration needs at least 3 cameras: with two, the intrinsics are not observable")
    if not (np.isfinite(huber_px) and huber_px >= 0 and np.isfinite(ftol) and ftol >= 0 and int(max_iter) >= 1):
        raise ValueError("huber_px and ftol must be finite and >= 0, max_iter at least 1")
    obs = _obs_array(image_points, C)
    R, t = _pose_arrays(camera_poses)
    K, dist = _lens_arrays(C)
    with _state["lock"]:
        core = _ba_core()
    with _state["ba_lock"]:
        R1, t1, K1, d1, _, info = core.ba_lens_solve(obs, R, t, K, dist, refine=flags, huber_px=huber_px, ftol=ftol, max_iter=max_iter)
    poses = [{"R": R1[c].copy(), "t": t1[c].copy()} for c in range(C)]
    params = []
    for c in range(C):
        p = dict(_state["camera_params"][c])
        p["intrinsic_matrix"] = K1[c].tolist()
        p["distortion_coef"] = d1[c].tolist()
        params.append(p)
    return (poses, params, info) if return_info else (poses, params)


def undistort_image_points(image_points, camera_params=None):
    """Raw capture rows -> the ideal pinhole pixels under each camera's intrinsic_matrix and distortion_coef
    (mocap_undistort_points): [N][C][2] float64, NaN where a camera did not see the point.  camera_params: the list
    calibrate_lenses returns; None = the params of set_camera_params."""
    params = _state["camera_params"] if camera_params is None else camera_params
    if params is None:
        raise RuntimeError("set_camera_params() has not been called and no camera_params were given")
    C = len(params)
    K = np.array([np.array(p["intrinsic_matrix"], dtype=np.float64) for p in params])
    dist = np.zeros((C, 5))
    for c in range(C):
        d = np.asarray(params[c].get("distortion_coef", [0.0] * 5), dtype=np.float64).ravel()
        dist[c, :min(5, d.size)] = d[:5]
    obs = _obs_array(image_points, C)
    with _state["lock"]:
        core = _ba_core()
    with _state["ba_lock"]:
        return core.undistort_points(obs, K, dist)


# ----------------------------------------------------------------------------- predicted precision
def precision_frame(to_world=None):
    """The `frame` of "predicted precision" (include/mocap_core.h) for coordinates as the frame path returns them: None without a
    world transform; with one -- x_w = swap_yz(dehom(T [diag(-1, -1, 1) X; 1])) -- the 3 x 4 matrix [A | a] with X = A x_w + a.  The
    inverse is taken here, once per call, never in the core.  ValueError for a T whose last row is not (0, 0, 0, k), k != 0, or whose
    linear part is singular."""
    T = _state["to_world"] if to_world is None else to_world
    if T is None:
        return None
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    if not np.all(np.isfinite(T)) or T[3, 0] != 0.0 or T[3, 1] != 0.0 or T[3, 2] != 0.0 or T[3, 3] == 0.0:
        raise ValueError("predicted precision needs an affine to-world matrix: last row (0, 0, 0, k) with k != 0")
    swap = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    M = swap @ (T[:3, :3] / T[3, 3]) @ np.diag([-1.0, -1.0, 1.0])
    m = swap @ (T[:3, 3] / T[3, 3])
    if not np.linalg.matrix_rank(M) == 3:
        raise ValueError("the to-world matrix's linear part is singular")
    A = np.linalg.inv(M)
    return np.concatenate([A, (-A @ m)[:, None]], axis=1)


def _precision_out(core, like, shape):
    """The five outputs of a precision call as tensors beside `like`."""
    import torch
    f64 = dict(dtype=torch.float64, device=like.device)
    i32 = dict(dtype=torch.int32, device=like.device)
    return {"cov": torch.empty(shape + (6,), **f64), "sig": torch.empty(shape + (3,), **f64), "axis": torch.empty(shape + (3,), **f64),
            "n_views": torch.empty(shape, **i32), "info": torch.empty(shape, **i32)}


def _resident_check(core, *tensors):
    for a in tensors:
        if a is not None and (not a.is_cuda or not a.is_contiguous() or a.device.index != core.device_id):
            raise ValueError(f"a resident array must be contiguous and live on GPU {core.device_id}: it is read in place")


def point_precision(object_points, seen=None, sigma_px=1.0, image_size=None, near=0.0, far=float("inf")):
    """How well the rig can know each of object_points [N][3] (world coordinates when a world transform is set, camera 0's otherwise):
    {"cov" [N][6] packed 00 01 02 11 12 22, "sig" [N][3] principal standard deviations ascending, "axis" [N][3] the worst direction,
    "n_views", "info" (capi.PM_*)} for pixel noise sigma_px, in the points' own length unit.  seen: per point the bit mask of the
    cameras that see it, or None = every camera that has it inside image_size = (width, height) between near and far.  NumPy in,
    NumPy out; torch tensors on the core's GPU are read in place and answered with tensors."""
    core = get_core()
    frame = precision_frame()
    if seen is None and image_size is None:
        raise ValueError("point_precision needs seen or image_size")
    if not getattr(object_points, "is_cuda", False):
        with _state["lock"]:
            return core.point_precision(object_points, seen, sigma_px, image_size, near, far, frame)
    import torch
    xyz = object_points
    assert xyz.dtype == torch.float64 and xyz.dim() == 2 and xyz.shape[1] == 3
    if seen is not None and not getattr(seen, "is_cuda", False):
        seen = torch.from_numpy(np.ascontiguousarray(seen, dtype=np.uint64).view(np.int64)).to(xyz.device)
    _resident_check(core, xyz, seen)
    torch.cuda.current_stream(xyz.device).synchronize()      # whatever torch itself still has queued on these buffers
    N = xyz.shape[0]
    out = _precision_out(core, xyz, (N,))
    with _state["lock"]:
        core.point_precision_dev(N, xyz.data_ptr(), 0 if seen is None else seen.data_ptr(), image_size, near, far, sigma_px, frame,
                                 *[out[k].data_ptr() for k in core.PRECISION_OUT])
        core.synchronize()
    return out


def frame_precision(result, sigma_px=1.0):
    """Predicted precision of every point of a frame batch: `result` is the dict the batch frame call returns ({"xyz" [F][K_max][3],
    "corr" [F][K_max][C], "n_out" | "n_pts" [F], "status" [F] optional}), NumPy arrays or torch tensors on the core's GPU (read in
    place) -> the outputs of point_precision per slot [F][K_max]; a slot without a point has info 0, n_views 0 and NaN."""
    core = get_core()
    frame = precision_frame()
    xyz, corr = result["xyz"], result["corr"]
    n_pts = result["n_pts"] if "n_pts" in result else result["n_out"]
    status = result.get("status")
    if not getattr(xyz, "is_cuda", False):
        with _state["lock"]:
            return core.frame_precision(np.asarray(xyz), np.asarray(corr), np.asarray(n_pts), None if status is None else np.asarray(status),
                                        sigma_px, frame)
    import torch
    assert xyz.dtype == torch.float64 and xyz.dim() == 3 and xyz.shape[2] == 3
    F, K_max = xyz.shape[:2]
    assert corr.dtype == torch.int16 and tuple(corr.shape) == (F, K_max, core.C)
    assert n_pts.dtype == torch.int32 and n_pts.numel() == F and (status is None or (status.dtype == torch.int32 and status.numel() == F))
    _resident_check(core, xyz, corr, n_pts, status)
    torch.cuda.current_stream(xyz.device).synchronize()
    out = _precision_out(core, xyz, (F, K_max))
    with _state["lock"]:
        core.frame_precision_dev(F, K_max, xyz.data_ptr(), corr.data_ptr(), n_pts.data_ptr(), 0 if status is None else status.data_ptr(),
                                 sigma_px, frame, *[out[k].data_ptr() for k in core.PRECISION_OUT])
        core.synchronize()
    return out


def capture_volume(lo, hi, step, image_size, sigma_px=1.0, near=0.0, far=float("inf"), min_views=2, max_sigma=float("inf"),
                   resident=False, want_seen=False):
    """Where in the room the rig can track, and how precisely: the box lo .. hi (world coordinates when a world transform is set,
    camera 0's otherwise) sampled every `step` (a number, or one per axis), n = floor((hi - lo) / step) + 1 voxels per axis from lo.
    Returns {"n_views" [nz][ny][nx] u8, "sig_max" [nz][ny][nx] f32 (the worst principal standard deviation, NaN where the point has
    none), "seen" (want_seen), "summary" [capi.PM_SUMMARY], "shape" (nx, ny, nz), "origin", "step",
    "good_voxels", "good_volume" (good voxels x the voxel's volume, in the caller's cubic unit), "histogram" [65] (voxels seen by
    exactly v cameras), "bbox" ((lo, hi) of the good voxels in coordinates, or None)}.  A voxel is GOOD when it has a covariance,
    at least min_views views and sig_max <= max_sigma.  resident=True leaves the arrays on the GPU as torch tensors."""
    core = get_core()
    frame = precision_frame()
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    step = np.broadcast_to(np.asarray(step, dtype=np.float64), (3,)).copy()
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(np.isfinite(step)) and np.all(step > 0) and np.all(hi >= lo)):
        raise ValueError("capture_volume needs finite lo <= hi and step > 0")
    shape = tuple(int(v) for v in np.floor((hi - lo) / step + 1e-9) + 1)
    e = np.diag(step)
    if not resident:
        with _state["lock"]:
            out = core.coverage_map(shape, lo, e[0], e[1], e[2], image_size, near, far, sigma_px, frame, min_views, max_sigma, want_seen)
        summary = out["summary"]
    else:
        import torch
        dev = torch.device("cuda", core.device_id)
        n = shape[::-1]
        out = {"n_views": torch.empty(n, dtype=torch.uint8, device=dev), "sig_max": torch.empty(n, dtype=torch.float32, device=dev),
               "seen": torch.empty(n, dtype=torch.int64, device=dev) if want_seen else None,
               "summary": torch.empty(capi.PM_SUMMARY, dtype=torch.int64, device=dev)}
        with _state["lock"]:
            core.coverage_map_dev(shape, lo, e[0], e[1], e[2], image_size, near, far, sigma_px, frame, min_views, max_sigma,
                                  out["n_views"].data_ptr(), out["sig_max"].data_ptr(), out["seen"].data_ptr() if want_seen else 0,
                                  out["summary"].data_ptr())
            core.synchronize()
        summary = out["summary"].cpu().numpy()
    good = int(summary[65])
    box = summary[66:72].reshape(3, 2)
    out.update(shape=shape, origin=lo, step=step, good_voxels=good, good_volume=good * float(np.prod(step)),
               histogram=np.array(summary[:65]), bbox=None if not good else (lo + box[:, 0] * step, lo + box[:, 1] * step))
    return out
