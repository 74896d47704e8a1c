"""ctypes binding of the C ABI in include/mocap_core.h (lib/libmocap_core.so).

Load order: PyTorch ships its own libamdhip64 under the same SONAME as the system one this library
links to; the first one loaded serves the whole process.  When PyTorch is used alongside (device
buffers, torch.distributed), import torch BEFORE the first MocapCore() so both share PyTorch's copy.

This is the host side of the drop-in boundary.  There is NO CPU fallback: if the shared
library is missing or no MI355X is visible, construction raises.  Marshalling only --
every number comes from the HIP kernels.
"""
import ctypes
import os

import numpy as np

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# MOCAP_CORE_LIB points at another build of the same C ABI (A/B measurements of kernel variants)
LIB_PATH = os.environ.get("MOCAP_CORE_LIB") or os.path.join(_PKG_ROOT, "lib", "libmocap_core.so")

MOCAP_OK = 0
MOCAP_E_ARG = -1
MOCAP_E_LIMIT = -4
MOCAP_E_NOCONV = -5
ST_ROOT_OVERFLOW = 1
ST_CAND_OVERFLOW = 2
ST_HIT_OVERFLOW = 4
ST_INTRACTABLE = 16      # with ST_CAND_OVERFLOW: a root of more than 2^24 groups the exact search could not bound
ST_FINAL = 32            # the re-submit pass has seen the frame: its status is final
ST_LOG2_GROUPS_SHIFT, ST_LOG2_GROUPS_MASK = 20, 0x1FF
ST_ROUNDED = 8          # informational (mocap_match_triangulate_f64): a coordinate was rounded to float32
BLOB_ST_POINT_OVERFLOW = 1
BLOB_ST_CAP_OVERFLOW = 2
JPEG_ST_OVERFLOW = 1      # mocap_encode_jpeg*: the image needs more than `capacity` bytes
OVERLAY_CONTOURS = 1      # mocap_set_preview_overlay: every contour pixel green (cv.drawContours, helpers.py:148)
OVERLAY_CENTRES = 2       # ... a filled radius-1 circle on every stored centroid (cv.circle, helpers.py:157)
OVERLAY_EPILINES = 4      # ... one epipolar line per point and later camera (drawlines, helpers.py:365)
CENTROID_REFERENCE = 0    # mocap_set_centroid_mode: the reference's int(m10 / m00) (helpers.py:152-155), the default
CENTROID_WEIGHTED = 1     # ... grey-weighted sub-pixel centroid over the contour's bounding box (include/mocap_core.h)
RB_MAX_BODIES, RB_MAX_MARKERS, RB_MAX_POINTS = 8, 8, 64   # mocap_set_rigid_bodies: bodies, markers per body, points per frame
RB_DEFAULT_WORK_CAP = 65536   # ... extensions one (frame, body) search may make when work_cap = 0
RB_ST_RMS = 1             # per (frame, body): the best assignment's fit has rms > max_rms (not found)
RB_ST_WORK_CAP = 2        # ... the search needed more than work_cap extensions (not found)
OPT_F32_ROUNDING = 1
MT_MAX_TRACKS, MT_MAX_POINTS = 64, 64   # mocap_set_marker_tracker: track slots, points per frame
MT_ST_FULL = 1            # per frame: a finite point found no free track slot (its id is -1)
MT_ST_BAD_TIME = 2        # ... the frame's time stamp is not finite: no output, the state untouched
BT_SRC_NONE, BT_SRC_GUIDED, BT_SRC_SEARCH, BT_SRC_COAST = 0, 1, 2, 3   # mocap_track_bodies: where a body's pose of a frame comes from
BT_ST_BAD_TIME = 1        # per frame: the time stamp is not finite: no output, the state untouched
CONSOLIDATE_OFF = 0       # mocap_set_point_consolidation: the frame path's points as the reference's algorithm gives them, the default
CONSOLIDATE_BLOBS = 1     # ... compacted so that no two points of a frame share a blob (include/mocap_core.h)
PC_MAX_POINTS = 256       # ... point slots per frame the consolidation takes
REFINE_MAX_ITERS = 16     # mocap_set_point_refinement: Levenberg-Marquardt steps at most (0 = off, the default)
RF_REFINED, RF_FEW_VIEWS, RF_BAD_INDEX, RF_BAD_OBS, RF_BAD_START = 1, 2, 4, 8, 16   # ... a point's info word: refined, or why not
RF_STEPS_SHIFT = 8        # ... and the accepted steps, info >> 8
LB_RESULT = 129           # mocap_learn_rigid_body: doubles of its `result`
LB_ST_NO_REF = 1          # ... status flags: no valid frame shows every selected marker (or the given ref_frame does not)
LB_ST_MARKER_UNSEEN = 2   # ... a marker had no used frame in some round and kept its previous position
TS_MAX_ROWS, TS_MAX_HALF_WINDOW = 1024, 32   # mocap_gather_tracks / mocap_smooth_tracks: rows, half window in frames
TS_SMOOTHED, TS_FILLED, TS_FEW, TS_SINGULAR, TS_BAD_TIME = 1, 2, 4, 8, 16   # ... a sample's flag (include/mocap_core.h)
ST_MAX_FIT = 64           # mocap_stitch_tracks: frames of an end model's window at most
RG_MAX_ROWS, RG_MAX_FRAMES = 256, 1 << 22    # mocap_rigid_groups: rows and frames at most
BP_MAX_BODIES = 64        # mocap_pose_rows / mocap_smooth_rotations / mocap_fill_rows: bodies of a call at most
BP_POSED, BP_FEW, BP_DEGENERATE, BP_RMS = 1, 2, 4, 8   # ... a (body, frame)'s flag (include/mocap_core.h)
BP_SRC_NONE, BP_SRC_MEASURED, BP_SRC_RIGID, BP_SRC_RIGID_FILLED = 0, 1, 2, 3   # ... where a filled sample comes from
JT_MAX_JOINTS = 64        # mocap_joint_series: joints of a call at most
JT_UNSEEN, JT_SINGULAR, JT_FIXED, JT_HINGE, JT_BALL = 0, 1, 2, 3, 4   # mocap_find_joints: a pair's kind (include/mocap_core.h)
BP_JOINTED = 16           # mocap_pose_joints: a (body, frame) posed through a joint, beside the BP_* flags above
JP_MAX_ROUNDS = 16        # ... rounds (joints away from a POSED body) at most
SK_MAX_ITERS = 16         # mocap_fit_skeleton: passes of the loop at most
BAJ_MAX_CAMERAS = 16      # mocap_ba_joint_*: cameras at most
BAJ_MAX_POINTS = 131072   # ... points at most
BAJ_INFO = 12             # ... doubles of `info`
BAJ_FOCAL = 1             # ... flag: one focal scale per camera is an unknown (needs 3 cameras)
BAJ_ST_CAMERA_UNSEEN = 1  # ... status: a camera has no observation on a participating point, nothing was changed
BAJ_ST_NO_POINTS = 2      # ... no point takes part, nothing was changed
BAJ_ST_SINGULAR = 4       # ... the reduced system had no Cholesky factor in some pass
BAJ_ST_POINT_SINGULAR = 8 # ... some point's 3 x 3 block had no Cholesky factor in some linearisation
BAJ_ST_LAMBDA = 16        # ... stopped because the damping passed 1e12
BAJ_ST_MAX_ITER = 32      # ... stopped after max_iter passes
BAJ_ST_BAD_DEPTH = 64     # ... ba_joint_normal_eq: a view was not used (depth not finite or <= 0)
BAL_MAX_CAMERAS = 16      # mocap_ba_lens_*: cameras at most
BAL_MAX_POINTS = 65536    # ... points at most
BAL_INFO = 12             # ... doubles of `info` (the layout of mocap_ba_joint_solve)
BAL_FOCAL, BAL_CENTRE, BAL_RADIAL, BAL_TANGENTIAL = 1, 2, 4, 8   # ... flags: (fx, fy) / (cx, cy) / (k1, k2) / (p1, p2) of every camera are unknowns
BAL_REFINE = {"focal": BAL_FOCAL, "centre": BAL_CENTRE, "radial": BAL_RADIAL, "tangential": BAL_TANGENTIAL}
BAL_ST_CAMERA_UNSEEN, BAL_ST_NO_POINTS, BAL_ST_SINGULAR, BAL_ST_POINT_SINGULAR = 1, 2, 4, 8   # ... status: the values of BAJ_ST_*
BAL_ST_LAMBDA, BAL_ST_MAX_ITER, BAL_ST_BAD_DEPTH = 16, 32, 64
UNDISTORT_MAX_POINTS = 1 << 20   # mocap_undistort_points: rows at most
UNDISTORT_NEWTON = 8      # ... Newton steps per observation
RESECT_MAX_POINTS = 131072  # mocap_resect_*: rows at most
RESECT_MAX_HYP = 4096     # ... hypotheses at most
RESECT_INFO = 12          # ... doubles of `info`
RESECT_OK, RESECT_TOO_FEW, RESECT_NO_MODEL = 0, 1, 2   # ... status: fewer than 4 valid rows / no candidate reaches min_inliers
PM_MAX_POINTS, PM_MAX_VOXELS, PM_MAX_DIM = 1 << 24, 1 << 27, 1024   # mocap_point_precision / mocap_coverage_map: points, voxels, nx ny nz at most
PM_SUMMARY = 72           # ... int64 entries of the map's summary: histogram [0..64], GOOD [65], imin imax jmin jmax kmin kmax [66..71]
PM_SWEEPS = 16            # ... Jacobi sweeps at most
PM_OK, PM_BAD_POINT, PM_BAD_VIEW, PM_FEW_VIEWS, PM_DEGENERATE = 1, 2, 4, 8, 16   # ... a point's info word (include/mocap_core.h)
OPT_EXHAUSTIVE_WALK = 2
OPT_BOUNDED_RESUBMIT = 4

_vp, _i32, _i64, _dbl, _u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_uint32
_u64 = ctypes.c_uint64

# name -> (restype, argtypes); must list every symbol include/mocap_core.h declares
SIGNATURES = {
    "mocap_create": (_i32, [_i32, ctypes.POINTER(_vp)]),
    "mocap_destroy": (None, [_vp]),
    "mocap_last_error": (ctypes.c_char_p, [_vp]),
    "mocap_version": (ctypes.c_char_p, []),
    "mocap_set_stream": (_i32, [_vp, _vp]),
    "mocap_synchronize": (_i32, [_vp]),
    "mocap_last_frame_kernel": (ctypes.c_char_p, [_vp]),
    "mocap_set_options": (_i32, [_vp, _u32]),
    "mocap_set_tuning": (_i32, [_vp, _i32, _i32, _i32]),
    "mocap_set_frame_limits": (_i32, [_vp, _i32, _i32]),
    "mocap_limits": (None, [ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "mocap_set_cameras": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "mocap_get_fundamental": (_i32, [_vp, _vp]),
    "mocap_triangulate": (_i32, [_vp, _i64, _vp, _vp, _vp]),
    "mocap_triangulate_dev": (_i32, [_vp, _i64, _vp, _vp, _vp]),
    "mocap_match_triangulate": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_match_triangulate_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_match_triangulate_dev_auto": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_resubmit_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_match_triangulate_auto": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_match_triangulate_f64": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_frame": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_frame_images": (_i32, [_vp, _i64, _vp, _i32, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp,
                                        _vp, _vp, _vp]),
    "mocap_track_frame_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mocap_set_rigid_bodies": (_i32, [_vp, _i32, _vp, _vp, _dbl, _dbl, _i64]),
    "mocap_locate_rigid_bodies": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_locate_rigid_bodies_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_frame_bodies": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp,
                                        _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_frame_bodies_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                            _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_set_marker_tracker": (_i32, [_vp, _i32, _dbl, _i32, _dbl]),
    "mocap_reset_marker_tracker": (_i32, [_vp]),
    "mocap_track_markers": (_i32, [_vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_markers_dev": (_i32, [_vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_get_marker_tracks": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_frame_ids": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_frame_ids_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_set_body_tracker": (_i32, [_vp, _i32, _dbl, _i32, _dbl]),
    "mocap_reset_body_tracker": (_i32, [_vp]),
    "mocap_track_bodies": (_i32, [_vp, _i64, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_bodies_dev": (_i32, [_vp, _i64, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_get_body_tracks": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_frame_bodies_tracked": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                                _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_frame_bodies_tracked_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp,
                                                    _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                    _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_learn_rigid_body": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _dbl, _vp]),
    "mocap_learn_rigid_body_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _dbl, _vp]),
    "mocap_gather_tracks": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    "mocap_gather_tracks_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    "mocap_smooth_tracks": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _i32, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_smooth_tracks_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _i32, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_stitch_tracks": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_stitch_tracks_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_rigid_groups": (_i32, [_vp, _i64, _i32, _vp, _i32, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_rigid_groups_dev": (_i32, [_vp, _i64, _i32, _vp, _i32, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_pose_rows": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_pose_rows_dev": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_smooth_rotations": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _i32, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mocap_smooth_rotations_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _i32, _dbl, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mocap_find_joints": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _i32, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_find_joints_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _i32, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_joint_series": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_joint_series_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_pose_joints": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dbl,
                                 _dbl, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_pose_joints_dev": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _dbl, _dbl, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_fit_skeleton": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dbl,
                                  _dbl, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_fit_skeleton_dev": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _dbl, _dbl, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_fill_rows": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_fill_rows_dev": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_set_point_consolidation": (_i32, [_vp, _i32]),
    "mocap_consolidate_points": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_consolidate_points_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_set_point_refinement": (_i32, [_vp, _i32]),
    "mocap_refine_points": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_refine_points_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_triangulate_refined": (_i32, [_vp, _i64, _vp, _i32, _vp, _vp, _vp]),
    "mocap_triangulate_refined_dev": (_i32, [_vp, _i64, _vp, _i32, _vp, _vp, _vp]),
    "mocap_set_object_filter": (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _dbl, _dbl]),
    "mocap_reset_object_filter": (_i32, [_vp, _dbl]),
    "mocap_filter_objects": (_i32, [_vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_filter_objects_dev": (_i32, [_vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_frame_filtered": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_track_frame_filtered_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_determine_scale": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _dbl, _vp, _vp]),
    "mocap_determine_scale_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _dbl, _vp, _vp]),
    "mocap_floor_factor": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "mocap_floor_factor_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "mocap_floor_from_factor": (_i32, [_vp, _vp, _vp, _vp]),
    "mocap_world_set_origin": (_i32, [_vp, _vp, _vp, _vp]),
    "mocap_set_image_params": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mocap_set_blob_options": (_i32, [_vp, _i32]),
    "mocap_set_centroid_mode": (_i32, [_vp, _i32]),
    "mocap_get_undistort_map": (_i32, [_vp, _i32, _vp]),
    "mocap_find_blobs": (_i32, [_vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mocap_find_blobs_dev": (_i32, [_vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "mocap_jpeg_bound": (_i64, [_i32, _i32]),
    "mocap_encode_jpeg": (_i32, [_vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _i64, _vp, _vp]),
    "mocap_encode_jpeg_dev": (_i32, [_vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _i64, _vp, _vp]),
    "mocap_find_blobs_jpeg": (_i32, [_vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp]),
    "mocap_track_frame_images_jpeg": (_i32, [_vp, _i64, _vp, _i32, _dbl, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp,
                                             _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp]),
    "mocap_set_preview_overlay": (_i32, [_vp, _u32]),
    "mocap_draw_epilines": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "mocap_draw_epilines_dev": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "mocap_set_world_transform": (_i32, [_vp, _vp]),
    "mocap_locate_objects": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_locate_objects_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_initial_poses": (_i32, [_vp, _i32, _i64, _vp, _vp, _dbl, _dbl, _i32, _vp, _vp, _vp]),
    "mocap_find_fundamental": (_i32, [_vp, _i64, _vp, _vp, _dbl, _dbl, _i32, _vp, _vp, _vp]),
    "mocap_ba_residuals": (_i32, [_vp, _i32, _vp, _i64, _vp, _vp]),
    "mocap_ba_normal_eq": (_i32, [_vp, _vp, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mocap_ba_trust_region_step": (_i32, [_vp, _i32, _i64, _vp, _vp, _dbl, _vp, _i32, _vp, _vp]),
    "mocap_track_record_bytes": (_i32, [_i32]),
    "mocap_compact_tracks_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mocap_reproject": (_i32, [_vp, _i64, _vp, _vp, _vp]),
    "mocap_set_ba_progress": (_i32, [_vp, _vp, _vp]),
    "mocap_ba_profile": (_i32, [_vp, _vp, _i64, _vp, _i32, _i32, _i32, _vp]),
    "mocap_ba_solve": (_i32, [_vp, _vp, _i64, _vp, _dbl, _dbl, _dbl, _i32, _i32, _i32, _vp]),
    "mocap_ba_solve_ex": (_i32, [_vp, _vp, _i64, _vp, _dbl, _dbl, _dbl, _i32, _i32, _i32, _vp, _i32]),
    "mocap_ba_joint_normal_eq": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _u32, _dbl, _dbl, _vp, _vp, _vp, _vp]),
    "mocap_ba_joint_solve": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _u32, _dbl, _dbl, _i32, _vp]),
    "mocap_resect_camera": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _dbl, _i32, _u64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mocap_resect_camera_dev": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _dbl, _i32, _u64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mocap_resect_hypotheses": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _dbl, _i32, _u64, _vp, _vp, _vp, _vp]),
    "mocap_ba_lens_normal_eq": (_i32, [_vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _dbl, _dbl, _vp, _vp, _vp, _vp]),
    "mocap_ba_lens_solve": (_i32, [_vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _dbl, _dbl, _i32, _vp]),
    "mocap_undistort_points": (_i32, [_vp, _i32, _i64, _vp, _vp, _vp, _vp]),
    "mocap_undistort_points_dev": (_i32, [_vp, _i32, _i64, _vp, _vp, _vp, _vp]),
    "mocap_precision_limits": (None, [ctypes.POINTER(_i32), ctypes.POINTER(_i64), ctypes.POINTER(_i32)]),
    "mocap_point_precision": (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_point_precision_dev": (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_frame_precision": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_frame_precision_dev": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mocap_coverage_map": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _dbl, _dbl, _dbl, _vp, _i32, _dbl, _vp, _vp, _vp,
                                  _vp]),
    "mocap_coverage_map_dev": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _dbl, _dbl, _dbl, _vp, _i32, _dbl, _vp, _vp,
                                      _vp, _vp]),
}

_lib = None


class MocapError(RuntimeError):
    code = None   # the MOCAP_E_* value, when the core returned one


def load_library(path=None):
    """dlopen the core.  Raises (never falls back) when the library is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise MocapError(f"{p} not found: build it with `make -C {_PKG_ROOT}` (hipcc, gfx950); "
                         "there is no CPU fallback")
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError = the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def floor_from_factor(factor, ctx=None, lib=None):
    """mocap_floor_from_factor (host-only arithmetic, no GPU): factor [17] -> (to_world 4x4, info dict, rc).  rc is MOCAP_OK or
    MOCAP_E_NOCONV (floor parallel to the xy-plane: the matrix is written as the arithmetic gives it); MOCAP_E_ARG raises."""
    lib = lib or load_library()
    factor = np.ascontiguousarray(factor, dtype=np.float64).reshape(17)
    W = np.zeros((4, 4))
    info = np.zeros(6)
    rc = lib.mocap_floor_from_factor(ctx, _p(factor), _p(W), _p(info))
    if rc not in (MOCAP_OK, MOCAP_E_NOCONV):
        e = MocapError(f"mocap_floor_from_factor: error {rc} (fewer than 3 points, or points that do not span a plane over x, y)")
        e.code = rc
        raise e
    return W, dict(zip(("a", "b", "c", "points", "rms_residual", "tilt"), info.tolist())), rc


def world_set_origin(to_world, point, ctx=None, lib=None):
    """mocap_world_set_origin (host-only arithmetic, no GPU): `set-origin`, index.py:200-207."""
    lib = lib or load_library()
    W = np.ascontiguousarray(to_world, dtype=np.float64).reshape(16)
    p = np.ascontiguousarray(point, dtype=np.float64).reshape(3)
    out = np.zeros((4, 4))
    rc = lib.mocap_world_set_origin(ctx, _p(W), _p(p), _p(out))
    if rc != MOCAP_OK:
        raise MocapError(f"mocap_world_set_origin: error {rc}")
    return out


class MocapCore:
    """One context = one GPU (include/mocap_core.h).  Methods mirror the C entry points."""

    def __init__(self, device_id=0):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.mocap_create(int(device_id), ctypes.byref(h))
        if rc != MOCAP_OK:
            raise MocapError(f"mocap_create(device {device_id}) failed with {rc}: no MI355X visible? "
                             "(there is no CPU fallback)")
        self._h = h
        self.device_id = int(device_id)
        self.C = 0
        self._hit_cap, self._force_wide = 32, False
        self.f32_rounding = True     # MOCAP_OPT_F32_ROUNDING, the library's default
        self.filter_objects_n = 0    # drone indices of the object filter (set_object_filter), 0 = off
        self.preview_overlay = 0     # OVERLAY_* bits (set_preview_overlay), the library's default
        self.centroid_mode = CENTROID_REFERENCE   # CENTROID_* (set_centroid_mode), the library's default
        self.rigid_bodies_n = 0      # bodies registered by set_rigid_bodies, 0 = none
        self.marker_tracker = None   # (gate, max_missed, vel_alpha, T_max) of set_marker_tracker, None = off
        self.body_tracker = None     # (gate, max_missed, vel_alpha) of set_body_tracker, None = off
        self.point_consolidation = CONSOLIDATE_OFF   # CONSOLIDATE_* (set_point_consolidation), the library's default
        self.point_refinement = 0    # Levenberg-Marquardt steps of set_point_refinement, 0 = off, the library's default

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mocap_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, allow=()):
        if rc != MOCAP_OK and rc not in allow:
            e = MocapError(f"mocap_core error {rc}: {self.lib.mocap_last_error(self._h).decode()}")
            e.code = rc
            raise e
        return rc

    def last_frame_kernel(self):
        """Name of the kernel the last frame batch went to (diagnostic; results never depend on it)."""
        return self.lib.mocap_last_frame_kernel(self._h).decode()

    # ------------------------------------------------------------------ configuration
    def set_cameras(self, K, R, t):
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 9)
        C = K.shape[0]
        R = np.ascontiguousarray(R, dtype=np.float64).reshape(C, 9)
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(C, 3)
        self._check(self.lib.mocap_set_cameras(self._h, C, _p(K), _p(R), _p(t)))
        self.C = C

    def set_options(self, f32_rounding=True, exhaustive_walk=False, bounded_resubmit=False):
        """exhaustive_walk: MOCAP_OPT_EXHAUSTIVE_WALK, the verification mode (every candidate group evaluated in full).
        bounded_resubmit: MOCAP_OPT_BOUNDED_RESUBMIT (no whole-GPU enumeration of roots the exact search gives up on)."""
        self._check(self.lib.mocap_set_options(self._h, (OPT_F32_ROUNDING if f32_rounding else 0) |
                                               (OPT_EXHAUSTIVE_WALK if exhaustive_walk else 0) |
                                               (OPT_BOUNDED_RESUBMIT if bounded_resubmit else 0)))
        self.f32_rounding = bool(f32_rounding)

    def set_tuning(self, frame_threads=0, heavy_threshold=-1, slice_size=0):
        self._check(self.lib.mocap_set_tuning(self._h, int(frame_threads), int(heavy_threshold), int(slice_size)))

    def set_frame_limits(self, hit_cap=0, force_wide=False):
        """hit_cap: gated hits kept per (root, camera) by the wide-frame variant (0 = keep the current
        value); force_wide: run every batch through that variant (tests)."""
        self._apply_frame_limits(hit_cap, force_wide)
        if hit_cap:
            self._hit_cap = int(hit_cap)
        self._force_wide = bool(force_wide)

    def _apply_frame_limits(self, hit_cap, force_wide):
        self._check(self.lib.mocap_set_frame_limits(self._h, int(hit_cap), int(bool(force_wide))))

    def set_stream(self, hip_stream_handle):
        self._check(self.lib.mocap_set_stream(self._h, ctypes.c_void_p(hip_stream_handle or 0)))

    def synchronize(self):
        self._check(self.lib.mocap_synchronize(self._h))

    def fundamental(self):
        F = np.zeros((self.C, self.C, 3, 3))
        self._check(self.lib.mocap_get_fundamental(self._h, _p(F)))
        return F

    # ------------------------------------------------------------------ host-buffer entry points
    def triangulate(self, obs):
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, self.C, 2)
        N = obs.shape[0]
        xyz = np.empty((N, 3))
        err = np.empty(N)
        self._check(self.lib.mocap_triangulate(self._h, N, _p(obs), _p(xyz), _p(err)))
        return xyz, err

    def reproject(self, obs, xyz):
        """Reprojection error of given points (calculate_reprojection_errors, helpers.py:203-241); NaN = < 2 views."""
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, self.C, 2)
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        assert xyz.shape[0] == obs.shape[0]
        err = np.empty(obs.shape[0])
        self._check(self.lib.mocap_reproject(self._h, obs.shape[0], _p(obs), _p(xyz), _p(err)))
        return err

    def match_triangulate(self, blobs, counts, gate_px=5.0, K_max=None, G_cap=1 << 20):
        blobs = np.ascontiguousarray(blobs, dtype=np.float32)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        F, C, M, _ = blobs.shape
        assert C == self.C and counts.shape == (F, C)
        K_max = min(C * M, 64) if K_max is None else int(K_max)
        xyz = np.full((F, K_max, 3), np.nan)
        err = np.full((F, K_max), np.nan)
        corr = np.full((F, K_max, C), -1, dtype=np.int16)
        n_out = np.zeros(F, dtype=np.int32)
        status = np.zeros(F, dtype=np.int32)
        n_cand = np.zeros(F, dtype=np.int32)
        self._check(self.lib.mocap_match_triangulate(self._h, F, M, _p(blobs), _p(counts), float(gate_px), K_max,
                                                     int(G_cap), _p(xyz), _p(err), _p(corr), _p(n_out),
                                                     _p(status), _p(n_cand)))
        return {"xyz": xyz, "err": err, "corr": corr, "n_out": n_out, "status": status, "n_cand": n_cand}

    def match_triangulate_auto(self, blobs, counts, gate_px=5.0, K_max=None, G_cap=1 << 20):
        """mocap_match_triangulate_auto: frames whose caps overflowed are re-submitted ON THE GPU by the core itself with the
        worst-case root capacity (C*M), the largest candidate cap and (wide frames) an uncapped hit list -- any caller of
        the C ABI gets this, not only Python.  What is left to do here is grow the output arrays when a re-submitted frame
        needs more than K_max slots (the C entry reports how many in n_out)."""
        blobs = np.ascontiguousarray(blobs, dtype=np.float32)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        F, C, M, _ = blobs.shape
        assert C == self.C and counts.shape == (F, C)
        K_max = min(C * M, 64) if K_max is None else int(K_max)

        def call(b, c, k):
            f = b.shape[0]
            out = {"xyz": np.full((f, k, 3), np.nan), "err": np.full((f, k), np.nan), "corr": np.full((f, k, C), -1, dtype=np.int16),
                   "n_out": np.zeros(f, dtype=np.int32), "status": np.zeros(f, dtype=np.int32), "n_cand": np.zeros(f, dtype=np.int32)}
            nres = ctypes.c_int32()
            self._check(self.lib.mocap_match_triangulate_auto(self._h, f, M, _p(b), _p(c), float(gate_px), k, int(G_cap),
                                                              _p(out["xyz"]), _p(out["err"]), _p(out["corr"]), _p(out["n_out"]),
                                                              _p(out["status"]), _p(out["n_cand"]), ctypes.addressof(nres)))
            out["resubmitted"] = nres.value
            return out

        res = call(blobs, counts, K_max)
        need = np.nonzero((res["status"] == ST_ROOT_OVERFLOW) & (res["n_out"] > K_max))[0]
        if need.size:
            grow = int(res["n_out"][need].max())
            big = call(blobs[need], counts[need], grow)
            for key, fill in (("xyz", np.nan), ("err", np.nan), ("corr", -1)):
                shape = list(res[key].shape)
                shape[1] = grow
                new = np.full(shape, fill, dtype=res[key].dtype)
                new[:, :K_max] = res[key]
                new[need] = big[key]
                res[key] = new
            for key in ("n_out", "status", "n_cand"):
                res[key][need] = big[key]
        return res

    def match_triangulate_f64(self, blobs, counts, gate_px=5.0, K_max=None, G_cap=1 << 20):
        """mocap_match_triangulate_f64: double centroids.  float32-representable coordinates are used exactly; others are
        rounded to the nearest float32 and the frame's status carries ST_ROUNDED (informational)."""
        blobs = np.ascontiguousarray(blobs, dtype=np.float64)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        F, C, M, _ = blobs.shape
        assert C == self.C and counts.shape == (F, C)
        K_max = min(C * M, 64) if K_max is None else int(K_max)
        while True:
            out = {"xyz": np.full((F, K_max, 3), np.nan), "err": np.full((F, K_max), np.nan), "corr": np.full((F, K_max, C), -1, dtype=np.int16),
                   "n_out": np.zeros(F, dtype=np.int32), "status": np.zeros(F, dtype=np.int32), "n_cand": np.zeros(F, dtype=np.int32)}
            self._check(self.lib.mocap_match_triangulate_f64(self._h, F, M, _p(blobs), _p(counts), float(gate_px), K_max, int(G_cap),
                                                             _p(out["xyz"]), _p(out["err"]), _p(out["corr"]), _p(out["n_out"]),
                                                             _p(out["status"]), _p(out["n_cand"]), None))
            need = ((out["status"] & ~ST_ROUNDED) == ST_ROOT_OVERFLOW) & (out["n_out"] > K_max)
            if need.any():
                K_max = int(out["n_out"][need].max())
                continue
            return out

    # ------------------------------------------------------------------ the live loop in one call
    def _track_outputs(self, F, K_max, O_max):
        O = max(1, int(O_max))
        return {"xyz": np.full((F, K_max, 3), np.nan), "err": np.full((F, K_max), np.nan),
                "corr": np.full((F, K_max, self.C), -1, dtype=np.int16), "n_pts": np.zeros(F, dtype=np.int32),
                "status": np.zeros(F, dtype=np.int32), "pos": np.full((F, O, 3), np.nan), "heading": np.full((F, O), np.nan),
                "error": np.full((F, O), np.nan), "droneIndex": np.full((F, O), -1, dtype=np.int32),
                "n_obj": np.zeros(F, dtype=np.int32)}

    @staticmethod
    def _track_ptrs(o, O_max):
        """The argument run every host mocap_track_frame* shares behind G_cap: frame outputs, O_max, object outputs."""
        return [_p(o[k]) for k in ("xyz", "err", "corr", "n_pts", "status")] + [int(O_max)] + \
               [_p(o[k]) for k in ("pos", "heading", "error", "droneIndex", "n_obj")]

    def _track_blobs(self, blobs, counts, K_max):
        """The blob inputs of a host mocap_track_frame* -> (blobs, counts, F, M, K_max), K_max defaulted."""
        blobs = np.ascontiguousarray(blobs, dtype=np.float32)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        F, C, M, _ = blobs.shape
        assert C == self.C and counts.shape == (F, C)
        return blobs, counts, F, M, min(C * M, 64) if K_max is None else int(K_max)

    @staticmethod
    def _track_retry(call, K_max, K_all, O_max):
        """call(K_max) -> the outputs of one mocap_track_frame*; again with more slots while a frame has more roots than K_max:
        the core re-ran those frames itself and says how many slots they need (n_pts).  K_all: a frame's blobs over all cameras."""
        limit = 256 if O_max else 1024
        while True:
            o = call(K_max)
            need = (o["status"] & ST_ROOT_OVERFLOW).astype(bool) & (o["n_pts"] > K_max)
            if not (need.any() and K_max < min(K_all, limit)):
                return o
            K_max = min(int(o["n_pts"][need].max()), limit)

    def track_frame(self, blobs, counts, gate_px=5.0, K_max=None, G_cap=1 << 20, O_max=8):
        """mocap_track_frame: match -> world coordinates -> locate_objects for one or a few frames in one call
        (helpers.py:94-133).  O_max = 0 switches the object search off (Cameras.is_locating_objects)."""
        blobs, counts, F, M, K_max = self._track_blobs(blobs, counts, K_max)

        def call(K_max):
            o = self._track_outputs(F, K_max, O_max)
            self._check(self.lib.mocap_track_frame(self._h, F, M, _p(blobs), _p(counts), float(gate_px), K_max, int(G_cap),
                                                   *self._track_ptrs(o, O_max)))
            return o
        return self._track_retry(call, K_max, self.C * M, O_max)

    def _track_images(self, entry, images, M_max, gate_px, K_max, G_cap, O_max, *stream):
        """mocap_track_frame_images / _images_jpeg (`stream`: the latter's trailing arguments), with the root-overflow retry."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        F, C = images.shape[:2]
        assert images.shape == (F, C, self.img_rows, self.img_cols, 3) and C == self.img_C == self.C
        K_max = min(C * M_max, 64) if K_max is None else int(K_max)

        def call(K_max):
            o = self._track_outputs(F, K_max, O_max)
            o.update(blobs=np.zeros((F, C, M_max, 2), dtype=np.float32), counts=np.zeros((F, C), dtype=np.int32),
                     blob_status=np.zeros((F, C), dtype=np.int32))
            self._check(entry(self._h, F, _p(images), int(M_max), float(gate_px), K_max, int(G_cap), _p(o["blobs"]), _p(o["counts"]),
                              _p(o["blob_status"]), *self._track_ptrs(o, O_max), *stream))
            return o
        return self._track_retry(call, K_max, C * M_max, O_max)

    def track_frame_images(self, images, M_max=16, gate_px=5.0, K_max=None, G_cap=1 << 20, O_max=8):
        """mocap_track_frame_images: raw camera frames [F][C][rows][cols][3] -> image points, object points, objects."""
        return self._track_images(self.lib.mocap_track_frame_images, images, M_max, gate_px, K_max, G_cap, O_max)

    def track_frame_images_jpeg(self, images, M_max=16, gate_px=5.0, K_max=None, G_cap=1 << 20, O_max=8, quality=95, capacity=None):
        """mocap_track_frame_images_jpeg: track_frame_images plus the preview stream: "jpeg" = one bytes object per frame set
        (its C processed frames side by side, the file cv.imencode('.jpg') writes), "jpeg_size" the bytes each needed."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        F, C = images.shape[:2]
        S = self.img_cols
        cap = self.jpeg_default_capacity(S, S * C) if capacity is None else int(capacity)
        while True:
            buf, size = np.zeros((F, cap), dtype=np.uint8), np.zeros(F, dtype=np.int64)
            o = self._track_images(self.lib.mocap_track_frame_images_jpeg, images, M_max, gate_px, K_max, G_cap, O_max,
                                   int(quality), _p(buf), cap, _p(size))
            K_max = o["xyz"].shape[1]                     # (the slots a root-overflow retry settled on)
            if capacity is None and (size > cap).any():   # a frame set that does not compress: once more with room for it
                cap = int(size.max())
                continue
            o["jpeg"] = [buf[f, :min(int(size[f]), cap)].tobytes() for f in range(F)]
            o["jpeg_size"] = size
            return o

    def track_frame_dev(self, n_frames, M_max, d_blobs, d_counts, gate_px, K_max, G_cap, d_xyz, d_err, d_corr, d_n_pts, d_status,
                        O_max=0, d_pos=0, d_heading=0, d_oerr=0, d_drone=0, d_n_obj=0):
        self._check(self.lib.mocap_track_frame_dev(
            self._h, int(n_frames), int(M_max), _vp(d_blobs), _vp(d_counts), float(gate_px), int(K_max), int(G_cap), _vp(d_xyz),
            _vp(d_err), _vp(d_corr), _vp(d_n_pts), _vp(d_status), int(O_max), _vp(d_pos or 0), _vp(d_heading or 0), _vp(d_oerr or 0),
            _vp(d_drone or 0), _vp(d_n_obj or 0)))

    # ------------------------------------------------------------------ before the path
    def set_image_params(self, rows, cols, K, dist, rotation=None):
        """Frame geometry + lens model of every camera (camera-params.json: intrinsic_matrix,
        distortion_coef, rotation) -> the undistortion maps of the blob-extraction stage."""
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 9)
        C = K.shape[0]
        dist = np.ascontiguousarray(dist, dtype=np.float64).reshape(C, 5)
        rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.int32).reshape(C)
        self._check(self.lib.mocap_set_image_params(self._h, C, int(rows), int(cols), _p(K), _p(dist), _p(rot)))
        self.img_C, self.img_rows, self.img_cols = C, int(rows), int(cols)

    def set_blob_options(self, skip_dark_tiles=True):
        """True / 1: activity pre-pass + early-out; False / 0: every tile filtered; 2: early-out decided inside the mask pass."""
        self._check(self.lib.mocap_set_blob_options(self._h, 2 if skip_dark_tiles == 2 and skip_dark_tiles is not True else int(bool(skip_dark_tiles))))

    def set_centroid_mode(self, mode):
        """mocap_set_centroid_mode: CENTROID_REFERENCE (default, the reference's integer centroids) or CENTROID_WEIGHTED
        (grey-weighted sub-pixel centroids; only the values in `blobs` change).  Honoured by find_blobs, find_blobs_dev,
        find_blobs_jpeg, track_frame_images and track_frame_images_jpeg."""
        self._check(self.lib.mocap_set_centroid_mode(self._h, int(mode)))
        self.centroid_mode = int(mode)

    def undistort_map(self, camera=0):
        m = np.zeros((self.img_cols, self.img_cols), dtype=np.uint32)
        self._check(self.lib.mocap_get_undistort_map(self._h, int(camera), _p(m)))
        return m

    def find_blobs(self, images, M_max=16, want_processed=False):
        """images [F][C][rows][cols][3] uint8 RGB -> blobs f32 [F][C][M_max][2], counts, status
        (the frame path's input layout), optionally the processed BGR frames."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        F, C = images.shape[:2]
        assert images.shape == (F, C, self.img_rows, self.img_cols, 3) and C == self.img_C
        blobs = np.zeros((F, C, M_max, 2), dtype=np.float32)
        counts = np.zeros((F, C), dtype=np.int32)
        status = np.zeros((F, C), dtype=np.int32)
        ncont = np.zeros((F, C), dtype=np.int32)
        proc = np.zeros((F, C, self.img_cols, self.img_cols, 3), dtype=np.uint8) if want_processed else None
        self._check(self.lib.mocap_find_blobs(self._h, F, _p(images), int(M_max), _p(blobs), _p(counts), _p(status),
                                              _p(proc), _p(ncont)))
        out = {"blobs": blobs, "counts": counts, "status": status, "n_contours": ncont}
        if want_processed:
            out["processed"] = proc
        return out

    def find_blobs_dev(self, n_frames, d_images, M_max, d_blobs, d_counts, d_status, d_processed=0):
        self._check(self.lib.mocap_find_blobs_dev(self._h, int(n_frames), _vp(d_images), int(M_max), _vp(d_blobs),
                                                  _vp(d_counts), _vp(d_status), _vp(d_processed or 0)))

    # ------------------------------------------------------------------ preview stream
    def jpeg_bound(self, H, W_total):
        """mocap_jpeg_bound: upper bound on the bytes of one H x W_total image (-1: not a size the encoder takes)."""
        return int(self.lib.mocap_jpeg_bound(int(H), int(W_total)))

    def jpeg_default_capacity(self, H, W_total):
        """Slot size the Python layer starts with: a quarter of the raw frame (camera frames compress to a few per cent of
        it), never more than the bound; a call that overflows it is repeated with the size the core reported."""
        return min(self.jpeg_bound(H, W_total), 1024 + H * W_total * 3 // 4)

    def encode_jpeg(self, bgr, quality=95, capacity=None):
        """mocap_encode_jpeg: bgr [F][T][H][W][3] uint8 (the blob stage's `processed`) -> per image the JPEG of its T tiles
        side by side.  Returns {"jpeg": [bytes per image], "sizes", "status"}; with an explicit `capacity` an image that
        needs more keeps its first `capacity` bytes and JPEG_ST_OVERFLOW in status."""
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        assert bgr.ndim == 5 and bgr.shape[4] == 3
        F, T, H, W = bgr.shape[:4]
        cap = max(1, self.jpeg_default_capacity(H, T * W)) if capacity is None else int(capacity)
        while True:
            buf = np.zeros((F, max(cap, 1)), dtype=np.uint8)
            sizes, status = np.zeros(F, dtype=np.int64), np.zeros(F, dtype=np.int32)
            self._check(self.lib.mocap_encode_jpeg(self._h, F, T, H, W, _p(bgr), int(quality), _p(buf), cap, _p(sizes), _p(status)))
            if capacity is None and (status & JPEG_ST_OVERFLOW).any():
                cap = int(sizes.max())
                continue
            return {"jpeg": [buf[f, :min(int(sizes[f]), cap)].tobytes() for f in range(F)], "sizes": sizes, "status": status}

    def encode_jpeg_dev(self, n_images, T, H, W, d_bgr, quality, d_jpeg, capacity, d_sizes, d_status):
        self._check(self.lib.mocap_encode_jpeg_dev(self._h, int(n_images), int(T), int(H), int(W), _vp(d_bgr), int(quality),
                                                   _vp(d_jpeg), int(capacity), _vp(d_sizes), _vp(d_status)))

    def find_blobs_jpeg(self, images, M_max=16, quality=95, capacity=None):
        """mocap_find_blobs_jpeg: find_blobs with the preview stream ("jpeg": bytes per frame set, "jpeg_size") in place of
        the processed frames, which stay on the device."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        F, C = images.shape[:2]
        assert images.shape == (F, C, self.img_rows, self.img_cols, 3) and C == self.img_C
        S = self.img_cols
        cap = self.jpeg_default_capacity(S, S * C) if capacity is None else int(capacity)
        while True:
            blobs = np.zeros((F, C, M_max, 2), dtype=np.float32)
            counts, status, ncont = (np.zeros((F, C), dtype=np.int32) for _ in range(3))
            buf, size = np.zeros((F, max(cap, 1)), dtype=np.uint8), np.zeros(F, dtype=np.int64)
            self._check(self.lib.mocap_find_blobs_jpeg(self._h, F, _p(images), int(M_max), _p(blobs), _p(counts), _p(status),
                                                       _p(ncont), int(quality), _p(buf), cap, _p(size)))
            if capacity is None and (size > cap).any():
                cap = int(size.max())
                continue
            return {"blobs": blobs, "counts": counts, "status": status, "n_contours": ncont,
                    "jpeg": [buf[f, :min(int(size[f]), cap)].tobytes() for f in range(F)], "jpeg_size": size}

    # ------------------------------------------------------------------ preview overlays
    def set_preview_overlay(self, flags):
        """mocap_set_preview_overlay: OVERLAY_* bits.  Contours and centre marks are painted into every picture the blob
        stage hands out (find_blobs(want_processed=True), find_blobs_dev with d_processed, find_blobs_jpeg,
        track_frame_images_jpeg), epipolar lines into the stream of track_frame_images_jpeg.  0 (default) = bare frames."""
        self._check(self.lib.mocap_set_preview_overlay(self._h, int(flags)))
        self.preview_overlay = int(flags)

    def draw_epilines(self, bgr, blobs, counts, corr, n_pts, status):
        """mocap_draw_epilines: bgr [F][C][S][S][3] uint8 (copied, the drawn copy is returned), blobs [F][C][M][2], counts
        [F][C] = the frame path's inputs, corr [F][K][C], n_pts [F], status [F] = its outputs, cameras of set_cameras."""
        bgr = np.array(bgr, dtype=np.uint8, order="C")
        F, C, S = bgr.shape[:3]
        assert bgr.shape == (F, C, S, S, 3) and C == self.C
        blobs = np.ascontiguousarray(blobs, dtype=np.float32)
        M = blobs.shape[2]
        assert blobs.shape == (F, C, M, 2)
        counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(F, C)
        corr = np.ascontiguousarray(corr, dtype=np.int16)
        K = corr.shape[1]
        assert corr.shape == (F, K, C)
        n_pts = np.ascontiguousarray(n_pts, dtype=np.int32).reshape(F)
        status = np.ascontiguousarray(status, dtype=np.int32).reshape(F)
        self._check(self.lib.mocap_draw_epilines(self._h, F, S, _p(bgr), M, _p(blobs), _p(counts), K, _p(corr), _p(n_pts), _p(status)))
        return bgr

    def draw_epilines_dev(self, n_frames, S, d_bgr, M_max, d_blobs, d_counts, K_max, d_corr, d_n_pts, d_status):
        self._check(self.lib.mocap_draw_epilines_dev(self._h, int(n_frames), int(S), _vp(d_bgr), int(M_max), _vp(d_blobs),
                                                     _vp(d_counts), int(K_max), _vp(d_corr), _vp(d_n_pts), _vp(d_status)))

    # ------------------------------------------------------------------ after the path
    def set_world_transform(self, to_world):
        """4x4 to-world matrix (Cameras.to_world_coords_matrix) -> frame-path points leave the kernel in
        world coordinates (helpers.py:96-103); None switches the epilogue off."""
        if to_world is None:
            self._check(self.lib.mocap_set_world_transform(self._h, None))
        else:
            W = np.ascontiguousarray(to_world, dtype=np.float64).reshape(16)
            self._check(self.lib.mocap_set_world_transform(self._h, _p(W)))

    def locate_objects(self, xyz, err, n_pts, O_max=8):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        F, K_max, _ = xyz.shape
        err = np.ascontiguousarray(err, dtype=np.float64).reshape(F, K_max)
        n_pts = np.ascontiguousarray(n_pts, dtype=np.int32).reshape(F)
        out = {"pos": np.full((F, O_max, 3), np.nan), "heading": np.full((F, O_max), np.nan),
               "error": np.full((F, O_max), np.nan), "droneIndex": np.full((F, O_max), -1, dtype=np.int32),
               "lead": np.full((F, O_max), -1, dtype=np.int32), "n_obj": np.zeros(F, dtype=np.int32)}
        self._check(self.lib.mocap_locate_objects(self._h, F, K_max, _p(xyz), _p(err), _p(n_pts), int(O_max),
                                                  _p(out["pos"]), _p(out["heading"]), _p(out["error"]),
                                                  _p(out["droneIndex"]), _p(out["lead"]), _p(out["n_obj"])))
        return out

    # ------------------------------------------------------------------ calibration tail (scale, floor plane, origin)
    @staticmethod
    def _capture(xyz, n_pts, status):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        F, K_max, _ = xyz.shape
        n_pts = np.ascontiguousarray(n_pts, dtype=np.int32).reshape(F)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(F)
        return xyz, n_pts, status, F, K_max

    def determine_scale(self, xyz, n_pts, status=None, actual_distance=0.15, want_pair_dist=False):
        """mocap_determine_scale over host arrays xyz [F][K_max][3], n_pts [F], status [F] or None ->
        {"scale_factor", "mean_distance", "pairs", "skipped"[, "pair_dist" [F]]}."""
        xyz, n_pts, status, F, K_max = self._capture(xyz, n_pts, status)
        res = np.zeros(4)
        pd = np.full(F, np.nan) if want_pair_dist else None
        self._check(self.lib.mocap_determine_scale(self._h, F, K_max, _p(xyz), _p(n_pts), _p(status), float(actual_distance),
                                                   _p(pd), _p(res)))
        out = {"scale_factor": float(res[0]), "mean_distance": float(res[1]), "pairs": int(res[2]), "skipped": int(res[3])}
        if want_pair_dist:
            out["pair_dist"] = pd
        return out

    def determine_scale_dev(self, n_frames, K_max, d_xyz, d_n_pts, d_status, actual_distance, d_pair_dist, d_result):
        """Device pointers (ints; d_status, d_pair_dist may be 0); d_result: device-accessible double[4]."""
        self._check(self.lib.mocap_determine_scale_dev(self._h, int(n_frames), int(K_max), _vp(d_xyz), _vp(d_n_pts),
                                                       _vp(d_status or 0), float(actual_distance), _vp(d_pair_dist or 0),
                                                       _vp(d_result)))

    def floor_factor(self, xyz, n_pts, status=None):
        """mocap_floor_factor over host arrays -> factor [17] (R of [x y 1 | z] row-major, then the point count)."""
        xyz, n_pts, status, F, K_max = self._capture(xyz, n_pts, status)
        factor = np.zeros(17)
        self._check(self.lib.mocap_floor_factor(self._h, F, K_max, _p(xyz), _p(n_pts), _p(status), _p(factor)))
        return factor

    def floor_factor_dev(self, n_frames, K_max, d_xyz, d_n_pts, d_status, d_factor):
        """Device pointers (ints; d_status may be 0); d_factor: device-accessible double[17]."""
        self._check(self.lib.mocap_floor_factor_dev(self._h, int(n_frames), int(K_max), _vp(d_xyz), _vp(d_n_pts),
                                                    _vp(d_status or 0), _vp(d_factor)))

    def floor_from_factor(self, factor):
        """-> (to_world 4x4, info dict, rc); see the module-level floor_from_factor."""
        return floor_from_factor(factor, ctx=self._h, lib=self.lib)

    def world_set_origin(self, to_world, point):
        return world_set_origin(to_world, point, ctx=self._h, lib=self.lib)

    # ------------------------------------------------------------------ rigid bodies (6-DoF poses of registered marker sets)
    def set_rigid_bodies(self, markers, tol=0.01, max_rms=0.005, work_cap=0):
        """mocap_set_rigid_bodies: `markers` = one [N][3] array of body coordinates per body (3 <= N <= 8, at most 8 bodies;
        an empty list clears the registration).  tol, max_rms in metres; work_cap 0 = RB_DEFAULT_WORK_CAP.  A registration the
        core refuses (MOCAP_E_ARG) raises and leaves the previous one in force."""
        B = len(markers)
        n = np.zeros(max(B, 1), dtype=np.int32)
        q = np.zeros((max(B, 1), RB_MAX_MARKERS, 3))
        for b, m in enumerate(markers[:RB_MAX_BODIES]):
            m = np.asarray(m, dtype=np.float64).reshape(-1, 3)
            n[b] = m.shape[0]
            q[b, :min(m.shape[0], RB_MAX_MARKERS)] = m[:RB_MAX_MARKERS]
        self._check(self.lib.mocap_set_rigid_bodies(self._h, B, _p(n), _p(q), float(tol), float(max_rms), int(work_cap)))
        self.rigid_bodies_n = B

    @staticmethod
    def _body_outputs(F, B_max):
        return {"found": np.zeros((F, B_max), dtype=np.int32), "n_used": np.zeros((F, B_max), dtype=np.int32),
                "assign": np.zeros((F, B_max, RB_MAX_MARKERS), dtype=np.int8), "R": np.zeros((F, B_max, 3, 3)),
                "t": np.zeros((F, B_max, 3)), "rms": np.zeros((F, B_max)), "score": np.zeros((F, B_max)),
                "rb_status": np.zeros((F, B_max), dtype=np.int32)}

    @staticmethod
    def _body_ptrs(o):
        return [_p(o[k]) for k in ("found", "n_used", "assign", "R", "t", "rms", "score", "rb_status")]

    def locate_rigid_bodies(self, xyz, n_pts, B_max=None):
        """mocap_locate_rigid_bodies over host arrays xyz [F][K_max][3] (K_max <= 64), n_pts [F] -> {"found", "n_used" [F][B],
        "assign" int8 [F][B][8], "R" [F][B][3][3], "t" [F][B][3], "rms", "score" [F][B], "rb_status" [F][B]}; the entries of a
        body that was not found are zero.  B_max: body slots per frame, default = the registered bodies."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        F, K_max, _ = xyz.shape
        n_pts = np.ascontiguousarray(n_pts, dtype=np.int32).reshape(F)
        B_max = self.rigid_bodies_n if B_max is None else int(B_max)
        o = self._body_outputs(F, B_max)
        self._check(self.lib.mocap_locate_rigid_bodies(self._h, F, K_max, _p(xyz), _p(n_pts), B_max, *self._body_ptrs(o)))
        return o

    def locate_rigid_bodies_dev(self, n_frames, K_max, d_xyz, d_n_pts, B_max, d_found, d_n_used, d_assign, d_R, d_t, d_rms,
                                d_score, d_status):
        self._check(self.lib.mocap_locate_rigid_bodies_dev(self._h, int(n_frames), int(K_max), _vp(d_xyz), _vp(d_n_pts), int(B_max),
                                                           _vp(d_found), _vp(d_n_used), _vp(d_assign), _vp(d_R), _vp(d_t),
                                                           _vp(d_rms), _vp(d_score), _vp(d_status)))

    def track_frame_bodies(self, blobs, counts, gate_px=5.0, K_max=None, G_cap=1 << 20, O_max=8, B_max=None):
        """mocap_track_frame_bodies: track_frame with the rigid-body stage behind the object search; the same dict plus the
        keys of locate_rigid_bodies.  With bodies registered a frame holds at most 64 points (K_max <= 64)."""
        blobs, counts, F, M, K_max = self._track_blobs(blobs, counts, K_max)
        B_max = self.rigid_bodies_n if B_max is None else int(B_max)
        o = self._track_outputs(F, K_max, O_max)
        o.update(self._body_outputs(F, B_max))
        self._check(self.lib.mocap_track_frame_bodies(self._h, F, M, _p(blobs), _p(counts), float(gate_px), K_max, int(G_cap),
                                                      *self._track_ptrs(o, O_max), B_max, *self._body_ptrs(o)))
        return o

    def track_frame_bodies_dev(self, n_frames, M_max, d_blobs, d_counts, gate_px, K_max, G_cap, d_xyz, d_err, d_corr, d_n_pts,
                               d_status, O_max, d_pos, d_heading, d_oerr, d_drone, d_n_obj, B_max, d_found, d_n_used, d_assign,
                               d_R, d_t, d_rms, d_score, d_rb_status):
        self._check(self.lib.mocap_track_frame_bodies_dev(
            self._h, int(n_frames), int(M_max), _vp(d_blobs), _vp(d_counts), float(gate_px), int(K_max), int(G_cap), _vp(d_xyz),
            _vp(d_err), _vp(d_corr), _vp(d_n_pts), _vp(d_status), int(O_max), _vp(d_pos or 0), _vp(d_heading or 0), _vp(d_oerr or 0),
            _vp(d_drone or 0), _vp(d_n_obj or 0), int(B_max), _vp(d_found), _vp(d_n_used), _vp(d_assign), _vp(d_R), _vp(d_t),
            _vp(d_rms), _vp(d_score), _vp(d_rb_status)))

    # ------------------------------------------------------------------ rigid-body learning (a body's markers from a capture)
    @staticmethod
    def learned_body(result, N):
        """The `result` doubles of mocap_learn_rigid_body -> the dict learn_rigid_body returns."""
        r = np.asarray(result, dtype=np.float64).reshape(LB_RESULT)
        N = int(N)
        pair = {k: np.zeros((N, N)) for k in ("pair_mean", "pair_std", "pair_frames")}
        p = 0
        for i in range(RB_MAX_MARKERS):
            for j in range(i + 1, RB_MAX_MARKERS):
                if j < N:
                    for k, base in (("pair_mean", 40), ("pair_std", 68), ("pair_frames", 96)):
                        pair[k][i, j] = pair[k][j, i] = r[base + p]
                p += 1
        seen = pair["pair_mean"][np.triu_indices(N, 1)][pair["pair_frames"][np.triu_indices(N, 1)] > 0]
        return {"markers": r[:24].reshape(RB_MAX_MARKERS, 3)[:N].copy(), "marker_rms": r[24:24 + N].copy(),
                "marker_frames": r[32:32 + N].astype(np.int64), "pair_mean": pair["pair_mean"], "pair_std": pair["pair_std"],
                "pair_frames": pair["pair_frames"].astype(np.int64), "frames_used": int(r[124]), "frames_valid": int(r[125]),
                "ref_frame": int(r[126]), "rms": float(r[127]), "status": int(r[128]),
                "min_pair_distance": float(seen.min()) if seen.size else 0.0}

    def learn_rigid_body(self, xyz, n_pts, ids, sel, status=None, ref_frame=-1, iters=4, max_rms=float("inf")):
        """mocap_learn_rigid_body over host arrays xyz [F][K_max][3] (K_max <= 64), n_pts [F], ids [F][K_max] (the marker tracker's),
        status [F] or None; sel = the 3 .. 8 track ids of the body's markers -> {"markers" [N][3] body coordinates (what
        set_rigid_bodies takes), "marker_rms", "marker_frames" [N], "pair_mean", "pair_std", "pair_frames" [N][N] symmetric,
        "frames_used", "frames_valid", "ref_frame", "rms", "status" (LB_ST_* flags), "min_pair_distance"}."""
        xyz, n_pts, status, F, K_max = self._capture(xyz, n_pts, status)
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(F, K_max)
        sel = np.ascontiguousarray(sel, dtype=np.int32).reshape(-1)
        res = np.zeros(LB_RESULT)
        self._check(self.lib.mocap_learn_rigid_body(self._h, F, K_max, _p(xyz), _p(n_pts), _p(ids), _p(status), sel.size, _p(sel),
                                                    int(ref_frame), int(iters), float(max_rms), _p(res)))
        return self.learned_body(res, sel.size)

    def learn_rigid_body_dev(self, n_frames, K_max, d_xyz, d_n_pts, d_id, d_status, sel, ref_frame, iters, max_rms, d_result):
        """Device pointers (ints; d_status may be 0); sel: host ids; d_result: device-accessible double[LB_RESULT]."""
        sel = np.ascontiguousarray(sel, dtype=np.int32).reshape(-1)
        self._check(self.lib.mocap_learn_rigid_body_dev(self._h, int(n_frames), int(K_max), _vp(d_xyz), _vp(d_n_pts), _vp(d_id),
                                                        _vp(d_status or 0), sel.size, _p(sel), int(ref_frame), int(iters),
                                                        float(max_rms), _vp(d_result)))

    # ------------------------------------------------------------------ trajectories (a session as one time series per marker)
    def gather_tracks(self, xyz, n_pts, ids, relabel, R, hits=None, min_hits=0):
        """mocap_gather_tracks over host arrays xyz [F][K_max][3] (K_max <= 64), n_pts [F], ids [F][K_max] (the marker tracker's),
        hits [F][K_max] or None; relabel [n_ids]: the row of each id, -1 = none -> traj [R][F][3], NaN where a row has no point."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        F, K_max, _ = xyz.shape
        n_pts = np.ascontiguousarray(n_pts, dtype=np.int32).reshape(F)
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(F, K_max)
        hits = None if hits is None else np.ascontiguousarray(hits, dtype=np.int32).reshape(F, K_max)
        relabel = np.ascontiguousarray(relabel, dtype=np.int32).reshape(-1)
        traj = np.zeros((max(int(R), 0), F, 3))
        self._check(self.lib.mocap_gather_tracks(self._h, F, K_max, _p(xyz), _p(n_pts), _p(ids), _p(hits), int(min_hits), relabel.size,
                                                 _p(relabel), int(R), _p(traj)))
        return traj

    def gather_tracks_dev(self, n_frames, K_max, d_xyz, d_n_pts, d_id, d_hits, min_hits, n_ids, d_relabel, R, d_traj):
        """Device pointers (ints; d_hits may be 0); d_relabel: device-accessible int32[n_ids]; d_traj: double[R][F][3]."""
        self._check(self.lib.mocap_gather_tracks_dev(self._h, int(n_frames), int(K_max), _vp(d_xyz), _vp(d_n_pts), _vp(d_id),
                                                     _vp(d_hits or 0), int(min_hits), int(n_ids), _vp(d_relabel), int(R), _vp(d_traj)))

    def smooth_tracks(self, t, traj, degree=2, W=8, span=float("inf"), n_min=None, max_gap=0):
        """mocap_smooth_tracks over host arrays t [F], traj [R][F][3] -> {"pos", "vel", "acc" [R][F][3], "res" [R][F], "n_used",
        "flag" int32 [R][F] (TS_* values)}: a local polynomial of `degree` over the present samples within W frames and `span`
        seconds of each sample; gaps of at most max_gap frames are filled.  n_min: samples a fit needs, default degree + 2
        (capped at 2 W + 1)."""
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        R, F, _ = traj.shape
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(F)
        n_min = min(int(degree) + 2, 2 * int(W) + 1) if n_min is None else int(n_min)
        o = {"pos": np.zeros((R, F, 3)), "vel": np.zeros((R, F, 3)), "acc": np.zeros((R, F, 3)), "res": np.zeros((R, F)),
             "n_used": np.zeros((R, F), dtype=np.int32), "flag": np.zeros((R, F), dtype=np.int32)}
        self._check(self.lib.mocap_smooth_tracks(self._h, F, R, _p(t), _p(traj), int(degree), int(W), float(span), n_min, int(max_gap),
                                                 *[_p(o[k]) for k in ("pos", "vel", "acc", "res", "n_used", "flag")]))
        return o

    def smooth_tracks_dev(self, n_frames, R, d_t, d_traj, degree, W, span, n_min, max_gap, d_pos, d_vel, d_acc, d_res, d_n_used,
                          d_flag):
        """Device pointers (ints), shapes as smooth_tracks."""
        self._check(self.lib.mocap_smooth_tracks_dev(self._h, int(n_frames), int(R), _vp(d_t), _vp(d_traj), int(degree), int(W),
                                                     float(span), int(n_min), int(max_gap), _vp(d_pos), _vp(d_vel), _vp(d_acc),
                                                     _vp(d_res), _vp(d_n_used), _vp(d_flag)))

    # ------------------------------------------------------------------ track stitching (the rows of one marker linked into a chain)
    STITCH_OUT = ("ext", "next", "prev", "cost", "chain", "row_of", "n_chains")

    def stitch_tracks(self, t, traj, fit_frames=8, max_dt=float("inf"), gate=0.05, gate_rate=0.0):
        """mocap_stitch_tracks over host arrays t [F], traj [R][F][3] (gather_tracks') -> {"ext" int32 [R][3]: first and last present
        frame and the number present (-1, -1, 0 for an empty row), "next", "prev" int32 [R]: the linked rows, -1 = none, "cost" [R]:
        the cost of the link to next, NaN where none, "chain" int32 [R]: the head row of each row's chain, "row_of" int32 [R]: the
        number of its chain, -1 for an empty row, "n_chains" int}.  A fragment's end is a line through the present samples of its
        last (first) fit_frames + 1 frames; p -> q is linked when q starts after p ends, at most max_dt seconds later, and the two
        extrapolations miss by less than gate + gate_rate * dt (symmetric mean square), cheapest pairs first."""
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        R, F, _ = traj.shape
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(F)
        o = {"ext": np.zeros((R, 3), dtype=np.int32), "cost": np.zeros(R), "n_chains": np.zeros(1, dtype=np.int32)}
        o.update({k: np.zeros(R, dtype=np.int32) for k in ("next", "prev", "chain", "row_of")})
        self._check(self.lib.mocap_stitch_tracks(self._h, F, R, _p(t), _p(traj), int(fit_frames), float(max_dt), float(gate),
                                                 float(gate_rate), *[_p(o[k]) for k in self.STITCH_OUT]))
        o["n_chains"] = int(o["n_chains"][0])
        return o

    def stitch_tracks_dev(self, n_frames, R, d_t, d_traj, fit_frames, max_dt, gate, gate_rate, d_ext, d_next, d_prev, d_cost, d_chain,
                          d_row_of, d_n_chains):
        """Device pointers (ints), shapes as stitch_tracks; d_n_chains: int32[1]."""
        self._check(self.lib.mocap_stitch_tracks_dev(self._h, int(n_frames), int(R), _vp(d_t), _vp(d_traj), int(fit_frames),
                                                     float(max_dt), float(gate), float(gate_rate), _vp(d_ext), _vp(d_next), _vp(d_prev),
                                                     _vp(d_cost), _vp(d_chain), _vp(d_row_of), _vp(d_n_chains)))

    # ------------------------------------------------------------------ rigid groups (the rows that keep their mutual distances)
    RIGID_OUT = ("cnt", "dist", "spread", "travel", "group_of", "gsize", "ghead", "gconf", "gspread", "n_groups")

    def rigid_groups(self, traj, min_common, tol, max_dist=float("inf"), min_travel=0.0):
        """mocap_rigid_groups over the host array traj [R][F][3] (gather_tracks') -> {"cnt" int32, "dist", "spread" [R][R]: frames
        in common, mean and standard deviation of every pair's distance (NaN where cnt is 0), "travel" [R]: the diagonal of each
        row's bounding box, "group_of" int32 [R]: the row's group or -1, "gsize", "ghead", "gconf" int32 [R], "gspread" [R]: per
        group its rows, lowest row, conflicts and largest edge spread (-1, -1, -1, NaN beyond n_groups), "n_groups" int}.  Two rows
        are linked when both have min_common samples and min_travel of travel, share min_common frames, and their distance has a
        standard deviation <= tol and a mean <= max_dist; the groups are the connected components of at least two rows."""
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        R, F, _ = traj.shape
        o = {"cnt": np.zeros((R, R), dtype=np.int32), "dist": np.zeros((R, R)), "spread": np.zeros((R, R)), "travel": np.zeros(R),
             "gspread": np.zeros(R), "n_groups": np.zeros(1, dtype=np.int32)}
        o.update({k: np.zeros(R, dtype=np.int32) for k in ("group_of", "gsize", "ghead", "gconf")})
        self._check(self.lib.mocap_rigid_groups(self._h, F, R, _p(traj), int(min_common), float(tol), float(max_dist),
                                                float(min_travel), *[_p(o[k]) for k in self.RIGID_OUT]))
        o["n_groups"] = int(o["n_groups"][0])
        return o

    def rigid_groups_dev(self, n_frames, R, d_traj, min_common, tol, max_dist, min_travel, d_cnt, d_dist, d_spread, d_travel,
                         d_group_of, d_gsize, d_ghead, d_gconf, d_gspread, d_n_groups):
        """Device pointers (ints), shapes as rigid_groups; d_n_groups: int32[1]."""
        self._check(self.lib.mocap_rigid_groups_dev(self._h, int(n_frames), int(R), _vp(d_traj), int(min_common), float(tol),
                                                    float(max_dist), float(min_travel), _vp(d_cnt), _vp(d_dist), _vp(d_spread),
                                                    _vp(d_travel), _vp(d_group_of), _vp(d_gsize), _vp(d_ghead), _vp(d_gconf),
                                                    _vp(d_gspread), _vp(d_n_groups)))

    # ------------------------------------------------------------------ body trajectories (a session's bodies as 6-DoF series)
    POSE_OUT = ("n_used", "present", "quat", "R", "t_pose", "rms", "flag")
    ROT_OUT = ("quat_s", "omega", "res", "n_used", "flag")

    @staticmethod
    def _session_bodies(bodies):
        """bodies = [{"rows": [N] session rows, "markers": [N][3]}] (learn_session_bodies' list) or [(rows, markers)]
        -> (B, n_markers int32 [B], rows int32 [B][8], markers [B][8][3]): the layout of the C entry points.  A body with more than 8
        markers keeps its count (the core refuses it); the core does every other check."""
        B = len(bodies)
        n = np.zeros(max(B, 1), dtype=np.int32)
        rows = np.full((max(B, 1), RB_MAX_MARKERS), -1, dtype=np.int32)
        q = np.zeros((max(B, 1), RB_MAX_MARKERS, 3))
        for b, body in enumerate(bodies):
            r, m = (body["rows"], body["markers"]) if isinstance(body, dict) else body
            r = np.asarray(r, dtype=np.int32).reshape(-1)
            m = np.asarray(m, dtype=np.float64).reshape(-1, 3)
            if r.size != m.shape[0]:
                raise ValueError(f"body {b}: {r.size} rows for {m.shape[0]} markers")
            n[b] = r.size
            rows[b, :min(r.size, RB_MAX_MARKERS)] = r[:RB_MAX_MARKERS]
            q[b, :min(r.size, RB_MAX_MARKERS)] = m[:RB_MAX_MARKERS]
        return B, n, rows, q

    def pose_rows(self, traj, bodies, max_rms=float("inf")):
        """mocap_pose_rows over the host array traj [R][F][3] (gather_tracks') and bodies (see _session_bodies) -> {"n_used",
        "present", "flag" int32 [B][F] (BP_* values), "quat" [B][F][4] (w, x, y, z; sign-continuous along f), "R" [B][F][3][3],
        "t_pose" [B][F][3], "rms" [B][F]}: the pose of each body at each frame from the markers present in its rows."""
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        R, F, _ = traj.shape
        B, n, rows, q = self._session_bodies(bodies)
        Bz = max(B, 1)
        o = {"quat": np.zeros((Bz, F, 4)), "R": np.zeros((Bz, F, 3, 3)), "t_pose": np.zeros((Bz, F, 3)), "rms": np.zeros((Bz, F))}
        o.update({k: np.zeros((Bz, F), dtype=np.int32) for k in ("n_used", "present", "flag")})
        self._check(self.lib.mocap_pose_rows(self._h, F, R, _p(traj), B, _p(n), _p(rows), _p(q), float(max_rms),
                                             *[_p(o[k]) for k in self.POSE_OUT]))
        return o

    def pose_rows_dev(self, n_frames, R, d_traj, bodies, max_rms, d_n_used, d_present, d_quat, d_Rm, d_t_pose, d_rms, d_flag):
        """Device pointers (ints), shapes as pose_rows; bodies: host data, as there."""
        B, n, rows, q = self._session_bodies(bodies)
        self._check(self.lib.mocap_pose_rows_dev(self._h, int(n_frames), int(R), _vp(d_traj), B, _p(n), _p(rows), _p(q), float(max_rms),
                                                 _vp(d_n_used), _vp(d_present), _vp(d_quat), _vp(d_Rm), _vp(d_t_pose), _vp(d_rms),
                                                 _vp(d_flag)))

    def smooth_rotations(self, t, quat, degree=2, W=8, span=float("inf"), n_min=None, max_gap=0):
        """mocap_smooth_rotations over host arrays t [F], quat [B][F][4] (pose_rows') -> {"quat_s" [B][F][4], "omega" [B][F][3] (rad/s,
        world axes), "res" [B][F], "n_used", "flag" int32 [B][F] (TS_* values)}; the parameters are smooth_tracks'."""
        quat = np.ascontiguousarray(quat, dtype=np.float64)
        B, F, _ = quat.shape
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(F)
        n_min = min(int(degree) + 2, 2 * int(W) + 1) if n_min is None else int(n_min)
        o = {"quat_s": np.zeros((B, F, 4)), "omega": np.zeros((B, F, 3)), "res": np.zeros((B, F)),
             "n_used": np.zeros((B, F), dtype=np.int32), "flag": np.zeros((B, F), dtype=np.int32)}
        self._check(self.lib.mocap_smooth_rotations(self._h, F, B, _p(t), _p(quat), int(degree), int(W), float(span), n_min,
                                                    int(max_gap), *[_p(o[k]) for k in self.ROT_OUT]))
        return o

    def smooth_rotations_dev(self, n_frames, B, d_t, d_quat, degree, W, span, n_min, max_gap, d_quat_s, d_omega, d_res, d_n_used,
                             d_flag):
        """Device pointers (ints), shapes as smooth_rotations."""
        self._check(self.lib.mocap_smooth_rotations_dev(self._h, int(n_frames), int(B), _vp(d_t), _vp(d_quat), int(degree), int(W),
                                                        float(span), int(n_min), int(max_gap), _vp(d_quat_s), _vp(d_omega),
                                                        _vp(d_res), _vp(d_n_used), _vp(d_flag)))

    def fill_rows(self, traj, bodies, flag, Rm, t_pose, flag_s=None, quat_s=None, pos_s=None):
        """mocap_fill_rows over host arrays: traj [R][F][3], bodies, pose_rows' flag, R and t_pose, and optionally (all three or
        none) the smoothers' flag_s, quat_s and pos_s -> {"filled" [R][F][3], "src" int32 [R][F] (BP_SRC_* values)}."""
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        R, F, _ = traj.shape
        B, n, rows, q = self._session_bodies(bodies)
        Bz = max(B, 1)
        flag = np.ascontiguousarray(flag, dtype=np.int32).reshape(Bz, F)
        Rm = np.ascontiguousarray(Rm, dtype=np.float64).reshape(Bz, F, 9)
        t_pose = np.ascontiguousarray(t_pose, dtype=np.float64).reshape(Bz, F, 3)
        flag_s = None if flag_s is None else np.ascontiguousarray(flag_s, dtype=np.int32).reshape(Bz, F)
        quat_s = None if quat_s is None else np.ascontiguousarray(quat_s, dtype=np.float64).reshape(Bz, F, 4)
        pos_s = None if pos_s is None else np.ascontiguousarray(pos_s, dtype=np.float64).reshape(Bz, F, 3)
        o = {"filled": np.zeros((R, F, 3)), "src": np.zeros((R, F), dtype=np.int32)}
        self._check(self.lib.mocap_fill_rows(self._h, F, R, _p(traj), B, _p(n), _p(rows), _p(q), _p(flag), _p(Rm), _p(t_pose),
                                             _p(flag_s), _p(quat_s), _p(pos_s), _p(o["filled"]), _p(o["src"])))
        return o

    def fill_rows_dev(self, n_frames, R, d_traj, bodies, d_flag, d_Rm, d_t_pose, d_flag_s, d_quat_s, d_pos_s, d_filled, d_src):
        """Device pointers (ints; d_flag_s, d_quat_s, d_pos_s all 0 or all given); bodies: host data, as in pose_rows."""
        B, n, rows, q = self._session_bodies(bodies)
        self._check(self.lib.mocap_fill_rows_dev(self._h, int(n_frames), int(R), _vp(d_traj), B, _p(n), _p(rows), _p(q), _vp(d_flag),
                                                 _vp(d_Rm), _vp(d_t_pose), _vp(d_flag_s or 0), _vp(d_quat_s or 0), _vp(d_pos_s or 0),
                                                 _vp(d_filled), _vp(d_src)))

    # ------------------------------------------------------------------ joints (which bodies are joined, where and how)
    JOINTS_OUT = ("cnt", "kind", "accepted", "lam", "sep", "centre", "axis", "parent", "n_joints")
    SERIES_OUT = ("present", "centre", "gap", "quat_rel", "twist")

    def find_joints(self, flag, R, t_pose, min_common=30, tol_rank=1e-4, max_sep=float("inf")):
        """mocap_find_joints over host arrays flag [B][F], R [B][F][3][3], t_pose [B][F][3] (pose_rows') -> {"cnt", "kind" (JT_*),
        "accepted" int32 [B][B], "lam" [B][B][3]: the three smallest eigenvalues of the pair's 6 x 6 system, "sep" [B][B]: the rms
        distance between the two images of the centre, "centre", "axis" [B][B][3]: centre[p][q] is the joint of the pair {p, q} in
        p's coordinates (axis: HINGE only), "parent" int32 [B]: the skeleton (-1 = a root or a body of no joint), "n_joints" int}."""
        flag = np.ascontiguousarray(flag, dtype=np.int32)
        B, F = flag.shape
        R = np.ascontiguousarray(R, dtype=np.float64).reshape(B, F, 9)
        t_pose = np.ascontiguousarray(t_pose, dtype=np.float64).reshape(B, F, 3)
        o = {k: np.zeros((B, B), dtype=np.int32) for k in ("cnt", "kind", "accepted")}
        o.update({k: np.zeros((B, B, 3)) for k in ("lam", "centre", "axis")})
        o.update(sep=np.zeros((B, B)), parent=np.zeros(B, dtype=np.int32), n_joints=np.zeros(1, dtype=np.int32))
        self._check(self.lib.mocap_find_joints(self._h, F, B, _p(flag), _p(R), _p(t_pose), int(min_common), float(tol_rank),
                                               float(max_sep), *[_p(o[k]) for k in self.JOINTS_OUT]))
        o["n_joints"] = int(o["n_joints"][0])
        return o

    def find_joints_dev(self, n_frames, B, d_flag, d_Rm, d_t_pose, min_common, tol_rank, max_sep, d_cnt, d_kind, d_accepted, d_lam,
                        d_sep, d_centre, d_axis, d_parent, d_n_joints):
        """Device pointers (ints), shapes as find_joints; d_n_joints: int32[1]."""
        self._check(self.lib.mocap_find_joints_dev(self._h, int(n_frames), int(B), _vp(d_flag), _vp(d_Rm), _vp(d_t_pose),
                                                   int(min_common), float(tol_rank), float(max_sep), _vp(d_cnt), _vp(d_kind),
                                                   _vp(d_accepted), _vp(d_lam), _vp(d_sep), _vp(d_centre), _vp(d_axis),
                                                   _vp(d_parent), _vp(d_n_joints)))

    @staticmethod
    def _joint_arrays(joints):
        """joints = [{"a", "b", "kind", "centre_a" or "c_a", "centre_b" or "c_b", "axis_b", "q_ref"}] (session_joints' list; q_ref
        defaults to the identity, axis_b to zero) -> (J, body_a, body_b, kind int32 [J], c_a, c_b, axis_b [J][3], q_ref [J][4]): the
        layout of the C entry point, which does every check."""
        J = len(joints)
        Jz = max(J, 1)
        ia, ib, kind = (np.zeros(Jz, dtype=np.int32) for _ in range(3))
        c_a, c_b, axis_b, q_ref = np.zeros((Jz, 3)), np.zeros((Jz, 3)), np.zeros((Jz, 3)), np.zeros((Jz, 4))
        for j, jt in enumerate(joints):
            ia[j], ib[j], kind[j] = int(jt["a"]), int(jt["b"]), int(jt["kind"])
            c_a[j] = jt["centre_a"] if "centre_a" in jt else jt["c_a"]
            c_b[j] = jt["centre_b"] if "centre_b" in jt else jt["c_b"]
            axis = jt.get("axis_b")
            axis_b[j] = 0.0 if axis is None or kind[j] != JT_HINGE else axis
            ref = jt.get("q_ref")
            q_ref[j] = (1.0, 0.0, 0.0, 0.0) if ref is None else ref
        return J, ia, ib, kind, c_a, c_b, axis_b, q_ref

    def joint_series(self, flag, quat, R, t_pose, joints):
        """mocap_joint_series over host arrays flag [B][F], quat [B][F][4], R [B][F][3][3], t_pose [B][F][3] (pose_rows') and joints
        (see _joint_arrays) -> {"present" int32 [J][F], "centre" [J][F][3]: the joint's place in the world, "gap" [J][F]: the distance
        between its two images, "quat_rel" [J][F][4]: b's orientation in a against q_ref, "twist" [J][F][2]: cosine and sine of half
        the hinge angle (HINGE only)}; NaN where a body is not POSED."""
        flag = np.ascontiguousarray(flag, dtype=np.int32)
        B, F = flag.shape
        quat = np.ascontiguousarray(quat, dtype=np.float64).reshape(B, F, 4)
        R = np.ascontiguousarray(R, dtype=np.float64).reshape(B, F, 9)
        t_pose = np.ascontiguousarray(t_pose, dtype=np.float64).reshape(B, F, 3)
        J, *arrays = self._joint_arrays(joints)
        Jz = max(J, 1)
        o = {"present": np.zeros((Jz, F), dtype=np.int32), "centre": np.zeros((Jz, F, 3)), "gap": np.zeros((Jz, F)),
             "quat_rel": np.zeros((Jz, F, 4)), "twist": np.zeros((Jz, F, 2))}
        self._check(self.lib.mocap_joint_series(self._h, F, B, _p(flag), _p(quat), _p(R), _p(t_pose), J, *[_p(a) for a in arrays],
                                                *[_p(o[k]) for k in self.SERIES_OUT]))
        return o

    def joint_series_dev(self, n_frames, B, d_flag, d_quat, d_Rm, d_t_pose, joints, d_present, d_centre, d_gap, d_quat_rel, d_twist):
        """Device pointers (ints), shapes as joint_series; joints: host data, as there."""
        J, *arrays = self._joint_arrays(joints)
        self._check(self.lib.mocap_joint_series_dev(self._h, int(n_frames), int(B), _vp(d_flag), _vp(d_quat), _vp(d_Rm), _vp(d_t_pose),
                                                    J, *[_p(a) for a in arrays], _vp(d_present), _vp(d_centre), _vp(d_gap),
                                                    _vp(d_quat_rel), _vp(d_twist)))

    # ------------------------------------------------------------------ joint poses (hidden bodies posed through their joints)
    JOINT_POSE_OUT = ("flag", "hops", "via", "quat", "R", "t_pose", "rms_j")

    @staticmethod
    def _joint_pose_arrays(joints):
        """joints = [{"a", "b", "kind", "centre_a" or "c_a", "centre_b" or "c_b", "axis_a", "axis_b"}] (session_joints' list; the axes
        are read under JT_HINGE alone) -> (J, body_a, body_b, kind int32 [J], c_a, c_b, axis_a, axis_b [J][3]): the layout of the C
        entry point, which does every check."""
        J = len(joints)
        Jz = max(J, 1)
        ia, ib, kind = (np.zeros(Jz, dtype=np.int32) for _ in range(3))
        c_a, c_b, axis_a, axis_b = (np.zeros((Jz, 3)) for _ in range(4))
        for j, jt in enumerate(joints):
            ia[j], ib[j], kind[j] = int(jt["a"]), int(jt["b"]), int(jt["kind"])
            c_a[j] = jt["centre_a"] if "centre_a" in jt else jt["c_a"]
            c_b[j] = jt["centre_b"] if "centre_b" in jt else jt["c_b"]
            if kind[j] == JT_HINGE:
                axis_a[j], axis_b[j] = jt["axis_a"], jt["axis_b"]
        return J, ia, ib, kind, c_a, c_b, axis_a, axis_b

    def pose_joints(self, traj, bodies, flag, quat, R, t_pose, joints, axis_len=0.1, max_rms=float("inf"), max_rounds=4):
        """mocap_pose_joints over host arrays: traj [R][F][3] and bodies as pose_rows takes them, pose_rows' flag [B][F], quat
        [B][F][4], R [B][F][3][3] and t_pose [B][F][3], and joints (see _joint_pose_arrays) -> {"flag" int32 [B][F]: the input's with
        BP_JOINTED where a FEW or DEGENERATE frame got a pose through a joint, "hops" [B][F]: joints between the body and the POSED
        body the pose came from (0 = POSED itself, -1 = no pose), "via" [B][F]: the joint it came through (-1 = none), "quat",
        "R", "t_pose": the poses (quat sign-continuous over the POSED and JOINTED frames), "rms_j" [B][F]: a jointed fit's rms}."""
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        Rr, F, _ = traj.shape
        B, n, rows, q = self._session_bodies(bodies)
        Bz = max(B, 1)
        flag = np.ascontiguousarray(flag, dtype=np.int32).reshape(Bz, F)
        quat = np.ascontiguousarray(quat, dtype=np.float64).reshape(Bz, F, 4)
        R = np.ascontiguousarray(R, dtype=np.float64).reshape(Bz, F, 9)
        t_pose = np.ascontiguousarray(t_pose, dtype=np.float64).reshape(Bz, F, 3)
        J, *arrays = self._joint_pose_arrays(joints)
        o = {k: np.zeros((Bz, F), dtype=np.int32) for k in ("flag", "hops", "via")}
        o.update(quat=np.zeros((Bz, F, 4)), R=np.zeros((Bz, F, 3, 3)), t_pose=np.zeros((Bz, F, 3)), rms_j=np.zeros((Bz, F)))
        self._check(self.lib.mocap_pose_joints(self._h, F, Rr, _p(traj), B, _p(n), _p(rows), _p(q), _p(flag), _p(quat), _p(R), _p(t_pose),
                                               J, *[_p(a) for a in arrays], float(axis_len), float(max_rms), int(max_rounds),
                                               *[_p(o[k]) for k in self.JOINT_POSE_OUT]))
        return o

    def pose_joints_dev(self, n_frames, R, d_traj, bodies, d_flag, d_quat, d_Rm, d_t_pose, joints, axis_len, max_rms, max_rounds,
                        d_flag_j, d_hops, d_via, d_quat_j, d_Rm_j, d_t_j, d_rms_j):
        """Device pointers (ints), shapes as pose_joints; bodies and joints: host data, as there."""
        B, n, rows, q = self._session_bodies(bodies)
        J, *arrays = self._joint_pose_arrays(joints)
        self._check(self.lib.mocap_pose_joints_dev(self._h, int(n_frames), int(R), _vp(d_traj), B, _p(n), _p(rows), _p(q), _vp(d_flag),
                                                   _vp(d_quat), _vp(d_Rm), _vp(d_t_pose), J, *[_p(a) for a in arrays], float(axis_len),
                                                   float(max_rms), int(max_rounds), _vp(d_flag_j), _vp(d_hops), _vp(d_via),
                                                   _vp(d_quat_j), _vp(d_Rm_j), _vp(d_t_j), _vp(d_rms_j)))

    # ------------------------------------------------------------------ skeleton fit (all joints of a frame closed at once)
    SKELETON_FIT_OUT = ("quat", "R", "t_pose", "rms_s", "cost0", "cost", "steps", "n_act")

    def fit_skeleton(self, traj, bodies, flag, quat, t_pose, joints, axis_len=0.1, w_joint=1.0, iters=8):
        """mocap_fit_skeleton over host arrays: traj [R][F][3] and bodies as pose_rows takes them, flag [B][F], quat [B][F][4] and
        t_pose [B][F][3] (pose_joints' or pose_rows' tables) and joints (see _joint_pose_arrays) -> {"quat" [B][F][4] (sign-continuous
        over the POSED and JOINTED frames), "R" [B][F][3][3], "t_pose" [B][F][3], "rms_s" [B][F]: the fitted poses and each body's
        marker rms under them (NaN for a body that was not posed at the start); "cost0", "cost" [F]: the frame's cost before and
        after, "steps" [F]: accepted passes, "n_act" [F]: joints with both bodies posed}."""
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        Rr, F, _ = traj.shape
        B, n, rows, q = self._session_bodies(bodies)
        Bz = max(B, 1)
        flag = np.ascontiguousarray(flag, dtype=np.int32).reshape(Bz, F)
        quat = np.ascontiguousarray(quat, dtype=np.float64).reshape(Bz, F, 4)
        t_pose = np.ascontiguousarray(t_pose, dtype=np.float64).reshape(Bz, F, 3)
        J, *arrays = self._joint_pose_arrays(joints)
        o = {"quat": np.zeros((Bz, F, 4)), "R": np.zeros((Bz, F, 3, 3)), "t_pose": np.zeros((Bz, F, 3)), "rms_s": np.zeros((Bz, F)),
             "cost0": np.zeros(F), "cost": np.zeros(F), "steps": np.zeros(F, dtype=np.int32), "n_act": np.zeros(F, dtype=np.int32)}
        self._check(self.lib.mocap_fit_skeleton(self._h, F, Rr, _p(traj), B, _p(n), _p(rows), _p(q), _p(flag), _p(quat), _p(t_pose), J,
                                                *[_p(a) for a in arrays], float(axis_len), float(w_joint), int(iters),
                                                *[_p(o[k]) for k in self.SKELETON_FIT_OUT]))
        return o

    def fit_skeleton_dev(self, n_frames, R, d_traj, bodies, d_flag, d_quat, d_t_pose, joints, axis_len, w_joint, iters, d_quat_s, d_Rm_s,
                         d_t_s, d_rms_s, d_cost0, d_cost, d_steps, d_n_act):
        """Device pointers (ints), shapes as fit_skeleton; bodies and joints: host data, as there."""
        B, n, rows, q = self._session_bodies(bodies)
        J, *arrays = self._joint_pose_arrays(joints)
        self._check(self.lib.mocap_fit_skeleton_dev(self._h, int(n_frames), int(R), _vp(d_traj), B, _p(n), _p(rows), _p(q), _vp(d_flag),
                                                    _vp(d_quat), _vp(d_t_pose), J, *[_p(a) for a in arrays], float(axis_len),
                                                    float(w_joint), int(iters), _vp(d_quat_s), _vp(d_Rm_s), _vp(d_t_s), _vp(d_rms_s),
                                                    _vp(d_cost0), _vp(d_cost), _vp(d_steps), _vp(d_n_act)))

    # ------------------------------------------------------------------ marker tracker (identities over time)
    def set_marker_tracker(self, gate=0.05, max_missed=5, vel_alpha=0.5, T_max=64):
        """mocap_set_marker_tracker: allocates and clears the tracker's state.  gate in metres; max_missed = frames a track may go
        unseen; vel_alpha in [0, 1]; T_max = track slots (1 .. 64), 0 switches the tracker off.  Settings the core refuses
        (MOCAP_E_ARG) raise and leave the previous ones, and the state, in force."""
        self._check(self.lib.mocap_set_marker_tracker(self._h, int(T_max), float(gate), int(max_missed), float(vel_alpha)))
        self.marker_tracker = (float(gate), int(max_missed), float(vel_alpha), int(T_max)) if int(T_max) else None

    def reset_marker_tracker(self):
        self._check(self.lib.mocap_reset_marker_tracker(self._h))

    @staticmethod
    def _marker_outputs(F, K_max):
        return {"id": np.full((F, K_max), -1, dtype=np.int32), "hits": np.zeros((F, K_max), dtype=np.int32),
                "n_tracks": np.zeros(F, dtype=np.int32), "mk_status": np.zeros(F, dtype=np.int32)}

    @staticmethod
    def _marker_ptrs(o):
        return [_p(o[k]) for k in ("id", "hits", "n_tracks", "mk_status")]

    def track_markers(self, t, xyz, n_pts):
        """mocap_track_markers over host arrays t [F], xyz [F][K_max][3] (K_max <= 64), n_pts [F], consecutive frames in order ->
        {"id", "hits" [F][K_max], "n_tracks", "mk_status" [F]}; id -1 = the slot holds no tracked point."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        F, K_max, _ = xyz.shape
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(F)
        n_pts = np.ascontiguousarray(n_pts, dtype=np.int32).reshape(F)
        o = self._marker_outputs(F, K_max)
        self._check(self.lib.mocap_track_markers(self._h, F, _p(t), K_max, _p(xyz), _p(n_pts), *self._marker_ptrs(o)))
        return o

    def track_markers_dev(self, n_frames, d_t, K_max, d_xyz, d_n_pts, d_id, d_hits, d_n_tracks, d_status):
        self._check(self.lib.mocap_track_markers_dev(self._h, int(n_frames), _vp(d_t), int(K_max), _vp(d_xyz), _vp(d_n_pts),
                                                     _vp(d_id), _vp(d_hits), _vp(d_n_tracks), _vp(d_status)))

    def marker_tracks(self):
        """mocap_get_marker_tracks (synchronises): the live tracks in slot order, {"id", "missed", "hits" [n], "pos", "vel" [n][3],
        "t_seen" [n]}."""
        n = np.zeros(1, dtype=np.int32)
        o = {"id": np.zeros(MT_MAX_TRACKS, dtype=np.int32), "pos": np.zeros((MT_MAX_TRACKS, 3)), "vel": np.zeros((MT_MAX_TRACKS, 3)),
             "t_seen": np.zeros(MT_MAX_TRACKS), "missed": np.zeros(MT_MAX_TRACKS, dtype=np.int32),
             "hits": np.zeros(MT_MAX_TRACKS, dtype=np.int32)}
        self._check(self.lib.mocap_get_marker_tracks(self._h, _p(n), *[_p(o[k]) for k in ("id", "pos", "vel", "t_seen", "missed", "hits")]))
        return {k: v[:int(n[0])].copy() for k, v in o.items()}

    def track_frame_ids(self, blobs, counts, t, gate_px=5.0, K_max=None, G_cap=1 << 20, O_max=8):
        """mocap_track_frame_ids: track_frame with the marker tracker behind the object search, t [F] = the frames' time stamps;
        the same dict plus the keys of track_markers.  A frame holds at most 64 points (K_max <= 64); one that needs more is
        reported like track_frame reports it (status, n_pts) and NOT re-run here: the tracker has consumed the call's frames."""
        blobs, counts, F, M, K_max = self._track_blobs(blobs, counts, K_max)
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(F)
        o = self._track_outputs(F, K_max, O_max)
        o.update(self._marker_outputs(F, K_max))
        self._check(self.lib.mocap_track_frame_ids(self._h, F, M, _p(blobs), _p(counts), float(gate_px), K_max, int(G_cap),
                                                   *self._track_ptrs(o, O_max), _p(t), *self._marker_ptrs(o)))
        return o

    def track_frame_ids_dev(self, n_frames, M_max, d_blobs, d_counts, gate_px, K_max, G_cap, d_xyz, d_err, d_corr, d_n_pts,
                            d_status, O_max, d_pos, d_heading, d_oerr, d_drone, d_n_obj, d_t, d_id, d_hits, d_n_tracks,
                            d_mk_status):
        self._check(self.lib.mocap_track_frame_ids_dev(
            self._h, int(n_frames), int(M_max), _vp(d_blobs), _vp(d_counts), float(gate_px), int(K_max), int(G_cap), _vp(d_xyz),
            _vp(d_err), _vp(d_corr), _vp(d_n_pts), _vp(d_status), int(O_max), _vp(d_pos or 0), _vp(d_heading or 0), _vp(d_oerr or 0),
            _vp(d_drone or 0), _vp(d_n_obj or 0), _vp(d_t), _vp(d_id), _vp(d_hits), _vp(d_n_tracks), _vp(d_mk_status)))

    # ------------------------------------------------------------------ body tracker (the registered bodies over time)
    def set_body_tracker(self, gate=0.03, max_missed=10, vel_alpha=0.5, on=True):
        """mocap_set_body_tracker: allocates and clears the tracker's slots (one per registered body).  gate in metres = how far a
        marker may be from where the predicted pose puts it; max_missed = frames a body may coast; vel_alpha in [0, 1];
        on=False switches the tracker off.  Settings the core refuses (MOCAP_E_ARG) raise and change nothing."""
        self._check(self.lib.mocap_set_body_tracker(self._h, 1 if on else 0, float(gate), int(max_missed), float(vel_alpha)))
        self.body_tracker = (float(gate), int(max_missed), float(vel_alpha)) if on else None

    def reset_body_tracker(self):
        self._check(self.lib.mocap_reset_body_tracker(self._h))

    @staticmethod
    def _tracked_outputs(F, B_max):
        return {"tracked": np.zeros((F, B_max), dtype=np.int32), "source": np.zeros((F, B_max), dtype=np.int32),
                "bt_n_used": np.zeros((F, B_max), dtype=np.int32), "bt_assign": np.zeros((F, B_max, RB_MAX_MARKERS), dtype=np.int8),
                "bt_R": np.zeros((F, B_max, 3, 3)), "bt_t": np.zeros((F, B_max, 3)), "bt_rms": np.zeros((F, B_max)),
                "bt_hits": np.zeros((F, B_max), dtype=np.int32), "bt_missed": np.zeros((F, B_max), dtype=np.int32),
                "bt_status": np.zeros(F, dtype=np.int32)}

    @staticmethod
    def _tracked_ptrs(o):
        return [_p(o[k]) for k in ("tracked", "source", "bt_n_used", "bt_assign", "bt_R", "bt_t", "bt_rms", "bt_hits", "bt_missed",
                                   "bt_status")]

    def track_bodies(self, t, xyz, n_pts, B_max=None):
        """mocap_track_bodies over host arrays t [F], xyz [F][K_max][3] (K_max <= 64), n_pts [F], consecutive frames in order ->
        {"tracked", "source" (BT_SRC_*), "bt_n_used", "bt_hits", "bt_missed" [F][B], "bt_assign" int8 [F][B][8], "bt_R" [F][B][3][3],
        "bt_t" [F][B][3], "bt_rms" [F][B], "bt_status" [F]}; the entries of a body without a pose (source 0) are zero.  B_max: body
        slots per frame, default = the registered bodies."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        F, K_max, _ = xyz.shape
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(F)
        n_pts = np.ascontiguousarray(n_pts, dtype=np.int32).reshape(F)
        B_max = self.rigid_bodies_n if B_max is None else int(B_max)
        o = self._tracked_outputs(F, B_max)
        self._check(self.lib.mocap_track_bodies(self._h, F, _p(t), K_max, _p(xyz), _p(n_pts), B_max, *self._tracked_ptrs(o)))
        return o

    def track_bodies_dev(self, n_frames, d_t, K_max, d_xyz, d_n_pts, B_max, d_tracked, d_source, d_n_used, d_assign, d_R, d_t_pose,
                         d_rms, d_hits, d_missed, d_status):
        self._check(self.lib.mocap_track_bodies_dev(self._h, int(n_frames), _vp(d_t), int(K_max), _vp(d_xyz), _vp(d_n_pts), int(B_max),
                                                    _vp(d_tracked), _vp(d_source), _vp(d_n_used), _vp(d_assign), _vp(d_R),
                                                    _vp(d_t_pose), _vp(d_rms), _vp(d_hits), _vp(d_missed), _vp(d_status)))

    def get_body_tracks(self):
        """mocap_get_body_tracks (synchronises): all eight slots as they are, {"live", "missed", "hits" [8], "R" [8][3][3],
        "p", "v" [8][3], "t_seen" [8]}; slot b belongs to registered body b."""
        B = RB_MAX_BODIES
        o = {"live": np.zeros(B, dtype=np.int32), "R": np.zeros((B, 3, 3)), "p": np.zeros((B, 3)), "v": np.zeros((B, 3)),
             "t_seen": np.zeros(B), "missed": np.zeros(B, dtype=np.int32), "hits": np.zeros(B, dtype=np.int32)}
        self._check(self.lib.mocap_get_body_tracks(self._h, *[_p(o[k]) for k in ("live", "R", "p", "v", "t_seen", "missed", "hits")]))
        return o

    def track_frame_bodies_tracked(self, blobs, counts, t, gate_px=5.0, K_max=None, G_cap=1 << 20, O_max=8, B_max=None):
        """mocap_track_frame_bodies_tracked: track_frame_bodies with the body tracker behind the rigid-body stage, t [F] = the
        frames' time stamps; the same dict plus the keys of track_bodies.  A frame holds at most 64 points (K_max <= 64)."""
        blobs, counts, F, M, K_max = self._track_blobs(blobs, counts, K_max)
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(F)
        B_max = self.rigid_bodies_n if B_max is None else int(B_max)
        o = self._track_outputs(F, K_max, O_max)
        o.update(self._body_outputs(F, B_max))
        o.update(self._tracked_outputs(F, B_max))
        self._check(self.lib.mocap_track_frame_bodies_tracked(self._h, F, M, _p(blobs), _p(counts), float(gate_px), K_max, int(G_cap),
                                                              *self._track_ptrs(o, O_max), B_max, *self._body_ptrs(o), _p(t),
                                                              *self._tracked_ptrs(o)))
        return o

    def track_frame_bodies_tracked_dev(self, n_frames, M_max, d_blobs, d_counts, gate_px, K_max, G_cap, d_xyz, d_err, d_corr, d_n_pts,
                                       d_status, O_max, d_pos, d_heading, d_oerr, d_drone, d_n_obj, B_max, d_found, d_n_used,
                                       d_assign, d_R, d_t, d_rms, d_score, d_rb_status, d_time, d_bt_tracked, d_bt_source,
                                       d_bt_n_used, d_bt_assign, d_bt_R, d_bt_t, d_bt_rms, d_bt_hits, d_bt_missed, d_bt_status):
        self._check(self.lib.mocap_track_frame_bodies_tracked_dev(
            self._h, int(n_frames), int(M_max), _vp(d_blobs), _vp(d_counts), float(gate_px), int(K_max), int(G_cap), _vp(d_xyz),
            _vp(d_err), _vp(d_corr), _vp(d_n_pts), _vp(d_status), int(O_max), _vp(d_pos or 0), _vp(d_heading or 0), _vp(d_oerr or 0),
            _vp(d_drone or 0), _vp(d_n_obj or 0), int(B_max), _vp(d_found), _vp(d_n_used), _vp(d_assign), _vp(d_R), _vp(d_t),
            _vp(d_rms), _vp(d_score), _vp(d_rb_status), _vp(d_time), _vp(d_bt_tracked), _vp(d_bt_source), _vp(d_bt_n_used),
            _vp(d_bt_assign), _vp(d_bt_R), _vp(d_bt_t), _vp(d_bt_rms), _vp(d_bt_hits), _vp(d_bt_missed), _vp(d_bt_status)))

    # ------------------------------------------------------------------ point consolidation (each blob supports one point)
    def set_point_consolidation(self, mode):
        """mocap_set_point_consolidation: CONSOLIDATE_OFF (default) | CONSOLIDATE_BLOBS = every track_frame* entry point compacts a
        frame's points to a set in which no two share a blob, in front of everything that reads them.  A mode the core refuses
        (MOCAP_E_ARG) raises and changes nothing."""
        self._check(self.lib.mocap_set_point_consolidation(self._h, int(mode)))
        self.point_consolidation = int(mode)

    def consolidate_points(self, xyz, err, corr, n_pts, status=None):
        """mocap_consolidate_points over host arrays as the frame path writes them (xyz [F][K_max][3], err [F][K_max], corr
        [F][K_max][C], n_pts [F], status [F] or None = 0).  The inputs are not touched; returns {"xyz", "err", "corr", "n_pts"}
        compacted, "src" [F][K_max] = the original slot of each kept point (-1 from the kept count on) and "n_in" [F] = the
        count before, -1 = the frame was not processed."""
        xyz = np.array(xyz, dtype=np.float64, order="C")
        F, K_max, _ = xyz.shape
        err = np.array(err, dtype=np.float64, order="C").reshape(F, K_max)
        corr = np.array(corr, dtype=np.int16, order="C")
        assert corr.shape == (F, K_max, self.C) or not self.C
        n_pts = np.array(n_pts, dtype=np.int32, order="C").reshape(F)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(F)
        src = np.full((F, K_max), -1, dtype=np.int32)
        n_in = np.full(F, -1, dtype=np.int32)
        self._check(self.lib.mocap_consolidate_points(self._h, F, K_max, _p(xyz), _p(err), _p(corr), _p(n_pts), _p(status), _p(src),
                                                      _p(n_in)))
        return {"xyz": xyz, "err": err, "corr": corr, "n_pts": n_pts, "src": src, "n_in": n_in}

    def consolidate_points_dev(self, n_frames, K_max, d_xyz, d_err, d_corr, d_n_pts, d_status=0, d_src=0, d_n_in=0):
        self._check(self.lib.mocap_consolidate_points_dev(self._h, int(n_frames), int(K_max), _vp(d_xyz), _vp(d_err), _vp(d_corr),
                                                          _vp(d_n_pts), _vp(d_status or 0), _vp(d_src or 0), _vp(d_n_in or 0)))

    # ------------------------------------------------------------------ point refinement (least-squares points, each camera's own K)
    def set_point_refinement(self, iters):
        """mocap_set_point_refinement: 0 = off (default), 1 .. REFINE_MAX_ITERS = every track_frame* entry point re-triangulates
        each kept group by that many Levenberg-Marquardt steps on the true reprojection error, in front of the consolidation and
        everything that reads the points.  A value the core refuses (MOCAP_E_ARG) raises and changes nothing."""
        self._check(self.lib.mocap_set_point_refinement(self._h, int(iters)))
        self.point_refinement = int(iters)

    def refine_points(self, blobs, counts, xyz, err, corr, n_pts, status=None, iters=4):
        """mocap_refine_points over host arrays as the frame path takes and writes them (blobs [F][C][M][2] f32, counts [F][C];
        xyz [F][K_max][3], err [F][K_max], corr [F][K_max][C], n_pts [F], status [F] or None = 0).  The inputs are not touched;
        returns {"xyz", "err"} with the refined points in place and "info" [F][K_max] (RF_* bits, accepted steps from bit 8)."""
        blobs = np.ascontiguousarray(blobs, dtype=np.float32)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        F, C, M, _ = blobs.shape
        xyz = np.array(xyz, dtype=np.float64, order="C")
        K_max = xyz.shape[1]
        assert xyz.shape == (F, K_max, 3) and counts.shape == (F, C)
        err = np.array(err, dtype=np.float64, order="C").reshape(F, K_max)
        corr = np.ascontiguousarray(corr, dtype=np.int16)
        assert corr.shape == (F, K_max, C) and (C == self.C or not self.C)
        n_pts = np.ascontiguousarray(n_pts, dtype=np.int32).reshape(F)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(F)
        info = np.full((F, K_max), -1, dtype=np.int32)
        self._check(self.lib.mocap_refine_points(self._h, F, M, _p(blobs), _p(counts), K_max, int(iters), _p(xyz), _p(err), _p(corr),
                                                 _p(n_pts), _p(status), _p(info)))
        return {"xyz": xyz, "err": err, "info": info}

    def refine_points_dev(self, n_frames, M_max, d_blobs, d_counts, K_max, iters, d_xyz, d_err, d_corr, d_n_pts, d_status=0, d_info=0):
        self._check(self.lib.mocap_refine_points_dev(self._h, int(n_frames), int(M_max), _vp(d_blobs), _vp(d_counts), int(K_max),
                                                     int(iters), _vp(d_xyz), _vp(d_err), _vp(d_corr), _vp(d_n_pts), _vp(d_status or 0),
                                                     _vp(d_info or 0)))

    def triangulate_refined(self, obs, iters=4):
        """mocap_triangulate_refined: obs [N][C][2] (NaN = unseen) -> (xyz [N][3], err [N], info [N]); rows the stage does not
        refine (fewer than 2 views, an infinite observation, a start behind a camera) are NaN and say why in info."""
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, self.C, 2)
        N = obs.shape[0]
        xyz = np.empty((N, 3))
        err = np.empty(N)
        info = np.full(N, -1, dtype=np.int32)
        self._check(self.lib.mocap_triangulate_refined(self._h, N, _p(obs), int(iters), _p(xyz), _p(err), _p(info)))
        return xyz, err, info

    def triangulate_refined_dev(self, N, d_obs, iters, d_xyz, d_err=0, d_info=0):
        self._check(self.lib.mocap_triangulate_refined_dev(self._h, int(N), _vp(d_obs), int(iters), _vp(d_xyz), _vp(d_err or 0),
                                                           _vp(d_info or 0)))

    # ------------------------------------------------------------------ predicted precision (point covariances, the capture-volume map)
    @staticmethod
    def _pm_frame(frame):
        return None if frame is None else np.ascontiguousarray(frame, dtype=np.float64).reshape(12)

    @staticmethod
    def _pm_image(image_size):
        return (0, 0) if image_size is None else (int(image_size[0]), int(image_size[1]))

    def point_precision(self, xyz, seen=None, sigma_px=1.0, image_size=None, near=0.0, far=float("inf"), frame=None):
        """mocap_point_precision: xyz [N][3] in the caller's coordinates (frame [3][4] = [A | a] takes them to camera 0's, None = they
        are camera 0's); seen [N] uint64 view masks, or None = the cameras that see the point inside image_size = (width, height) and
        near .. far -> {"cov" [N][6], "sig" [N][3] ascending, "axis" [N][3], "n_views" [N], "info" [N] (PM_*)}: sigma_px^2 H^-1."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        N = xyz.shape[0]
        seen = None if seen is None else np.ascontiguousarray(seen, dtype=np.uint64).reshape(N)
        frame = self._pm_frame(frame)
        w, h = self._pm_image(image_size)
        out = {"cov": np.empty((N, 6)), "sig": np.empty((N, 3)), "axis": np.empty((N, 3)), "n_views": np.empty(N, dtype=np.int32),
               "info": np.empty(N, dtype=np.int32)}
        self._check(self.lib.mocap_point_precision(self._h, N, _p(xyz), _p(seen), w, h, float(near), float(far), float(sigma_px), _p(frame),
                                                   *[_p(out[k]) for k in self.PRECISION_OUT]))
        return out

    PRECISION_OUT = ("cov", "sig", "axis", "n_views", "info")

    def point_precision_dev(self, N, d_xyz, d_seen, image_size, near, far, sigma_px, frame, d_cov, d_sig, d_axis, d_n_views, d_info):
        """mocap_point_precision_dev: the arrays are device pointers (d_seen, d_cov, d_axis may be 0), frame a host array or None;
        enqueued on the context's stream."""
        frame = self._pm_frame(frame)
        w, h = self._pm_image(image_size)
        self._check(self.lib.mocap_point_precision_dev(self._h, int(N), _vp(d_xyz), _vp(d_seen or 0), w, h, float(near), float(far),
                                                       float(sigma_px), _p(frame), _vp(d_cov or 0), _vp(d_sig), _vp(d_axis or 0),
                                                       _vp(d_n_views), _vp(d_info)))

    def frame_precision(self, xyz, corr, n_pts, status=None, sigma_px=1.0, frame=None):
        """mocap_frame_precision over host arrays as the frame path wrote them (xyz [F][K_max][3], corr [F][K_max][C], n_pts [F],
        status [F] or None) -> the outputs of point_precision per slot [F][K_max]; slots without a point: info 0, n_views 0, NaN."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        F, K_max = xyz.shape[:2]
        corr = np.ascontiguousarray(corr, dtype=np.int16)
        assert xyz.shape == (F, K_max, 3) and corr.shape == (F, K_max, self.C)
        n_pts = np.ascontiguousarray(n_pts, dtype=np.int32).reshape(F)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(F)
        frame = self._pm_frame(frame)
        out = {"cov": np.empty((F, K_max, 6)), "sig": np.empty((F, K_max, 3)), "axis": np.empty((F, K_max, 3)),
               "n_views": np.empty((F, K_max), dtype=np.int32), "info": np.empty((F, K_max), dtype=np.int32)}
        self._check(self.lib.mocap_frame_precision(self._h, F, K_max, _p(xyz), _p(corr), _p(n_pts), _p(status), float(sigma_px), _p(frame),
                                                   *[_p(out[k]) for k in self.PRECISION_OUT]))
        return out

    def frame_precision_dev(self, n_frames, K_max, d_xyz, d_corr, d_n_pts, d_status, sigma_px, frame, d_cov, d_sig, d_axis, d_n_views,
                            d_info):
        frame = self._pm_frame(frame)
        self._check(self.lib.mocap_frame_precision_dev(self._h, int(n_frames), int(K_max), _vp(d_xyz), _vp(d_corr), _vp(d_n_pts),
                                                       _vp(d_status or 0), float(sigma_px), _p(frame), _vp(d_cov or 0), _vp(d_sig),
                                                       _vp(d_axis or 0), _vp(d_n_views), _vp(d_info)))

    @staticmethod
    def _pm_grid(origin, e0, e1, e2):
        return [np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (origin, e0, e1, e2)]

    def coverage_map(self, shape, origin, e0, e1, e2, image_size, near=0.0, far=float("inf"), sigma_px=1.0, frame=None, min_views=2,
                     max_sigma=float("inf"), want_seen=False):
        """mocap_coverage_map: shape = (nx, ny, nz); voxel (i, j, k) at origin + i e0 + j e1 + k e2 in the caller's coordinates ->
        {"n_views" [nz][ny][nx] u8, "sig_max" [nz][ny][nx] f32, "seen" u64 (want_seen), "summary" [PM_SUMMARY] i64}."""
        nx, ny, nz = (int(v) for v in shape)
        g = self._pm_grid(origin, e0, e1, e2)
        frame = self._pm_frame(frame)
        w, h = self._pm_image(image_size)
        n = (max(nz, 0), max(ny, 0), max(nx, 0))
        out = {"n_views": np.empty(n, dtype=np.uint8), "sig_max": np.empty(n, dtype=np.float32),
               "seen": np.empty(n, dtype=np.uint64) if want_seen else None, "summary": np.empty(PM_SUMMARY, dtype=np.int64)}
        self._check(self.lib.mocap_coverage_map(self._h, nx, ny, nz, *[_p(v) for v in g], w, h, float(near), float(far), float(sigma_px),
                                                _p(frame), int(min_views), float(max_sigma), _p(out["n_views"]), _p(out["sig_max"]),
                                                _p(out["seen"]), _p(out["summary"])))
        return out

    def coverage_map_dev(self, shape, origin, e0, e1, e2, image_size, near, far, sigma_px, frame, min_views, max_sigma, d_n_views,
                         d_sig_max, d_seen, d_summary):
        """mocap_coverage_map_dev: the four outputs are device pointers (d_seen may be 0); the grid and frame are host arrays."""
        nx, ny, nz = (int(v) for v in shape)
        g = self._pm_grid(origin, e0, e1, e2)
        frame = self._pm_frame(frame)
        w, h = self._pm_image(image_size)
        self._check(self.lib.mocap_coverage_map_dev(self._h, nx, ny, nz, *[_p(v) for v in g], w, h, float(near), float(far),
                                                    float(sigma_px), _p(frame), int(min_views), float(max_sigma), _vp(d_n_views),
                                                    _vp(d_sig_max), _vp(d_seen or 0), _vp(d_summary)))

    # ------------------------------------------------------------------ object filter (`filtered_objects`)
    def set_object_filter(self, num_objects, b=None, a=None, buffer_size=300, process_noise=1e-2, measurement_noise=1.0):
        """mocap_set_object_filter: the reference's KalmanFilter(num_objects) on the device (KalmanFilter.py, LowPassFilter.py).
        b, a: low-pass coefficients; default = the reference's butter(5, 20 / (60 / 2))."""
        if b is None or a is None:
            from scipy.signal import butter
            b, a = butter(5, 20 / (60.0 / 2), btype="low")
        b = np.ascontiguousarray(b, dtype=np.float64).ravel()
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        assert b.size == a.size
        self._check(self.lib.mocap_set_object_filter(self._h, int(num_objects), b.size, _p(b), _p(a), int(buffer_size),
                                                     float(process_noise), float(measurement_noise)))
        self.filter_objects_n = int(num_objects)

    def reset_object_filter(self, now):
        self._check(self.lib.mocap_reset_object_filter(self._h, float(now)))

    def _filter_outputs(self, F):
        D = self.filter_objects_n
        return {"fpos": np.full((F, D, 3), np.nan, dtype=np.float32), "fvel": np.full((F, D, 3), np.nan, dtype=np.float32),
                "fheading": np.full((F, D), np.nan), "chosen": np.full((F, D), -1, dtype=np.int32)}

    def filter_objects(self, t, pos, heading, drone, n_obj):
        """mocap_filter_objects: t [F], and locate_objects' pos [F][O][3], heading [F][O], droneIndex [F][O], n_obj [F] ->
        {"fpos", "fvel" float32 [F][D][3], "fheading" [F][D], "chosen" [F][D] (-1 = drone not in filtered_objects)}."""
        t = np.ascontiguousarray(t, dtype=np.float64).ravel()
        F = t.size
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        O = pos.shape[1]
        assert pos.shape == (F, O, 3)
        heading = np.ascontiguousarray(heading, dtype=np.float64).reshape(F, O)
        drone = np.ascontiguousarray(drone, dtype=np.int32).reshape(F, O)
        n_obj = np.ascontiguousarray(n_obj, dtype=np.int32).reshape(F)
        o = self._filter_outputs(F)
        self._check(self.lib.mocap_filter_objects(self._h, F, _p(t), O, _p(pos), _p(heading), _p(drone), _p(n_obj), _p(o["fpos"]),
                                                  _p(o["fvel"]), _p(o["fheading"]), _p(o["chosen"])))
        return o

    def filter_objects_dev(self, n_frames, d_t, O_max, d_pos, d_heading, d_drone, d_n_obj, d_fpos, d_fvel, d_fheading, d_chosen):
        self._check(self.lib.mocap_filter_objects_dev(self._h, int(n_frames), _vp(d_t), int(O_max), _vp(d_pos), _vp(d_heading),
                                                      _vp(d_drone), _vp(d_n_obj), _vp(d_fpos), _vp(d_fvel), _vp(d_fheading),
                                                      _vp(d_chosen)))

    def track_frame_filtered(self, blobs, counts, t, gate_px=5.0, K_max=None, G_cap=1 << 20, O_max=8):
        """mocap_track_frame_filtered: track_frame with the object filter behind the object search, t [F] = the frames' time
        stamps.  A frame that needs more than K_max slots is reported like track_frame reports it (status, n_pts) and NOT
        re-run here: the filter has consumed the call's time stamps."""
        blobs, counts, F, M, K_max = self._track_blobs(blobs, counts, K_max)
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(F)
        o = self._track_outputs(F, K_max, O_max)
        o.update(self._filter_outputs(F))
        self._check(self.lib.mocap_track_frame_filtered(self._h, F, M, _p(blobs), _p(counts), float(gate_px), K_max, int(G_cap),
                                                        *self._track_ptrs(o, O_max), _p(t),
                                                        *[_p(o[k]) for k in ("fpos", "fvel", "fheading", "chosen")]))
        return o

    def track_frame_filtered_dev(self, n_frames, M_max, d_blobs, d_counts, gate_px, K_max, G_cap, d_xyz, d_err, d_corr, d_n_pts,
                                 d_status, O_max, d_pos, d_heading, d_oerr, d_drone, d_n_obj, d_t, d_fpos, d_fvel, d_fheading,
                                 d_chosen):
        self._check(self.lib.mocap_track_frame_filtered_dev(
            self._h, int(n_frames), int(M_max), _vp(d_blobs), _vp(d_counts), float(gate_px), int(K_max), int(G_cap), _vp(d_xyz),
            _vp(d_err), _vp(d_corr), _vp(d_n_pts), _vp(d_status), int(O_max), _vp(d_pos), _vp(d_heading), _vp(d_oerr), _vp(d_drone),
            _vp(d_n_obj), _vp(d_t), _vp(d_fpos), _vp(d_fvel), _vp(d_fheading), _vp(d_chosen)))

    # ------------------------------------------------------------------ device-pointer entry points
    def match_triangulate_dev(self, n_frames, M_max, d_blobs, d_counts, gate_px, K_max, G_cap, d_xyz, d_err,
                              d_corr, d_n_out, d_status, d_n_cand=0):
        """Raw device pointers (ints); enqueues on the context's stream and returns."""
        self._check(self.lib.mocap_match_triangulate_dev(
            self._h, int(n_frames), int(M_max), _vp(d_blobs), _vp(d_counts), float(gate_px), int(K_max),
            int(G_cap), _vp(d_xyz), _vp(d_err), _vp(d_corr), _vp(d_n_out), _vp(d_status), _vp(d_n_cand or 0)))

    def match_triangulate_dev_auto(self, n_frames, M_max, d_blobs, d_counts, gate_px, K_max, G_cap, d_xyz, d_err,
                                   d_corr, d_n_out, d_status, d_n_cand=0, d_resubmitted=0):
        """mocap_match_triangulate_dev_auto: the same, then the frames that hit a cap are re-run ON THE DEVICE with the largest
        caps and scattered back -- three more enqueues, no host wait.  d_resubmitted: 0, or a device-accessible int32[2]
        {frames flagged, frames re-run}."""
        self._check(self.lib.mocap_match_triangulate_dev_auto(
            self._h, int(n_frames), int(M_max), _vp(d_blobs), _vp(d_counts), float(gate_px), int(K_max),
            int(G_cap), _vp(d_xyz), _vp(d_err), _vp(d_corr), _vp(d_n_out), _vp(d_status), _vp(d_n_cand or 0),
            _vp(d_resubmitted or 0)))

    def resubmit_dev(self, n_frames, M_max, d_blobs, d_counts, gate_px, K_max, d_xyz, d_err, d_corr, d_n_out, d_status,
                     d_n_cand=0, d_resubmitted=0):
        """mocap_resubmit_dev: the re-submit stage alone, for a batch whose first pass has run (continues where a scratch batch
        smaller than the flagged set stopped: d_resubmitted[0] > d_resubmitted[1])."""
        self._check(self.lib.mocap_resubmit_dev(
            self._h, int(n_frames), int(M_max), _vp(d_blobs), _vp(d_counts), float(gate_px), int(K_max), _vp(d_xyz), _vp(d_err),
            _vp(d_corr), _vp(d_n_out), _vp(d_status), _vp(d_n_cand or 0), _vp(d_resubmitted or 0)))

    def compact_tracks_dev(self, n_frames, K_max, d_n_out, d_xyz, d_err, d_corr, d_offsets, d_records, capacity, d_total=0):
        """Valid points of a frame batch -> fixed-stride records + exclusive prefix of n_out (device pointers)."""
        self._check(self.lib.mocap_compact_tracks_dev(self._h, int(n_frames), int(K_max), _vp(d_n_out), _vp(d_xyz), _vp(d_err),
                                                      _vp(d_corr), _vp(d_offsets), _vp(d_records or 0), int(capacity),
                                                      _vp(d_total or 0)))

    def locate_objects_dev(self, n_frames, K_max, d_xyz, d_err, d_n_pts, O_max, d_pos, d_heading, d_error, d_drone, d_n_obj,
                           d_lead=0):
        """mocap_locate_objects_dev: device pointers in, device pointers out, enqueued on the core's stream.  Only the first
        min(n_obj, O_max) object slots of a frame are written."""
        self._check(self.lib.mocap_locate_objects_dev(self._h, int(n_frames), int(K_max), _vp(d_xyz), _vp(d_err), _vp(d_n_pts),
                                                      int(O_max), _vp(d_pos), _vp(d_heading), _vp(d_error), _vp(d_drone),
                                                      _vp(d_lead or 0), _vp(d_n_obj)))

    def triangulate_dev(self, N, d_obs, d_xyz, d_err):
        self._check(self.lib.mocap_triangulate_dev(self._h, int(N), _vp(d_obs), _vp(d_xyz), _vp(d_err or 0)))

    # ------------------------------------------------------------------ initial poses
    def find_fundamental(self, p1, p2, threshold=1.0, confidence=0.99999, max_iters=1000):
        p1 = np.ascontiguousarray(p1, dtype=np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(p2, dtype=np.float32).reshape(-1, 2)
        n = p1.shape[0]
        F = np.zeros(9)
        mask = np.zeros(n, dtype=np.uint8)
        info = np.zeros(3, dtype=np.int32)
        self._check(self.lib.mocap_find_fundamental(self._h, n, _p(p1), _p(p2), float(threshold), float(confidence),
                                                    int(max_iters), _p(F), _p(mask), _p(info)))
        return F.reshape(3, 3), mask, {"inliers": int(info[0]), "iterations": int(info[1]), "best_iteration": int(info[2])}

    def initial_poses(self, obs, K, threshold=1.0, confidence=0.99999, max_iters=1000):
        """obs (N, C, 2) NaN = unseen, K [C][3][3] -> (R [C][3][3], t [C][3], info [C-1][4])."""
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        N, C, _ = obs.shape
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(C, 9)
        R = np.zeros((C, 3, 3))
        t = np.zeros((C, 3))
        info = np.zeros((max(C - 1, 1), 4), dtype=np.int32)
        self._check(self.lib.mocap_initial_poses(self._h, C, N, _p(obs), _p(K), float(threshold), float(confidence),
                                                 int(max_iters), _p(R), _p(t), _p(info)))
        return R, t, info

    # ------------------------------------------------------------------ bundle adjustment
    def n_params(self):
        return 1 + 7 * (self.C - 1)

    def ba_residuals(self, params, obs):
        params = np.ascontiguousarray(np.atleast_2d(params), dtype=np.float64)
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, self.C, 2)
        P, N = params.shape[0], obs.shape[0]
        assert params.shape[1] == self.n_params()
        r = np.empty((P, N))
        self._check(self.lib.mocap_ba_residuals(self._h, P, _p(params), N, _p(obs), _p(r)))
        return r

    def ba_normal_eq(self, x, obs, f32_residuals=False, use_cauchy=True, want_J=False):
        x = np.ascontiguousarray(x, dtype=np.float64)
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, self.C, 2)
        n, N = self.n_params(), obs.shape[0]
        JtJ = np.empty((n, n))
        Jtr = np.empty(n)
        cost = ctypes.c_double()
        m = ctypes.c_int64()
        J = np.zeros((N, n)) if want_J else None
        self._check(self.lib.mocap_ba_normal_eq(self._h, _p(x), N, _p(obs), int(f32_residuals), int(use_cauchy),
                                                _p(JtJ), _p(Jtr), ctypes.addressof(cost), _p(J),
                                                ctypes.addressof(m)))
        out = {"JtJ": JtJ, "Jtr": Jtr, "cost": cost.value, "m": m.value}
        if want_J:
            out["J"] = J[:m.value]
        return out

    def ba_trust_region_step(self, JtJ, Jtr, m, Delta, alpha=0.0, method=0):
        """The trust-region subproblem as mocap_ba_solve solves it -> (step, alpha, {"method", "live"})."""
        JtJ = np.ascontiguousarray(JtJ, dtype=np.float64)
        n = JtJ.shape[0]
        Jtr = np.ascontiguousarray(Jtr, dtype=np.float64).reshape(n)
        a = ctypes.c_double(float(alpha))
        step = np.zeros(n)
        info = np.zeros(2, dtype=np.int32)
        self._check(self.lib.mocap_ba_trust_region_step(self._h, n, int(m), _p(JtJ), _p(Jtr), float(Delta),
                                                        ctypes.addressof(a), int(method), _p(step), _p(info)))
        return step, a.value, {"method": int(info[0]), "live": int(info[1])}

    _BA_CB = ctypes.CFUNCTYPE(None, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_void_p)

    def set_ba_progress(self, fn):
        """fn(x: ndarray) is called once per accepted step of ba_solve (None = off)."""
        if fn is None:
            self._ba_cb = None
            self._check(self.lib.mocap_set_ba_progress(self._h, None, None))
            return
        self._ba_cb = self._BA_CB(lambda px, n, _u: fn(np.ctypeslib.as_array(px, shape=(n,)).copy()))   # keep a reference
        self._check(self.lib.mocap_set_ba_progress(self._h, ctypes.cast(self._ba_cb, ctypes.c_void_p), None))

    def ba_profile(self, x, obs, f32_residuals=True, use_cauchy=True, reps=100):
        x = np.ascontiguousarray(x, dtype=np.float64)
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, self.C, 2)
        out = np.zeros(8)
        self._check(self.lib.mocap_ba_profile(self._h, _p(x), obs.shape[0], _p(obs), int(f32_residuals), int(use_cauchy),
                                              int(reps), _p(out)))
        keys = ("gpu_us_per_linearisation", "wall_us_per_linearisation", "host_tr_us", "launches", "m", "NP", "fused", "cost")
        return dict(zip(keys, out.tolist()))

    def ba_solve(self, x0, obs, ftol=1e-2, xtol=1e-8, gtol=1e-8, max_iter=0, f32_residuals=True,
                 use_cauchy=True):
        x = np.array(x0, dtype=np.float64)
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, self.C, 2)
        info = np.zeros(12)
        rc = self._check(self.lib.mocap_ba_solve_ex(self._h, _p(x), obs.shape[0], _p(obs), float(ftol), float(xtol),
                                                    float(gtol), int(max_iter), int(f32_residuals), int(use_cauchy),
                                                    _p(info), info.size), allow=(MOCAP_E_NOCONV,))
        keys = ("iterations", "nfev", "status", "cost0", "cost", "optimality", "m", "elapsed_ms", "njev", "relaunches",
                "handovers", "fused")
        return x, dict(zip(keys, info.tolist()), converged=(rc == MOCAP_OK))

    # ------------------------------------------------------------------ joint bundle adjustment (poses and points together)
    _BAJ_INFO_KEYS = ("passes", "accepted", "cost0", "cost", "lambda", "participating", "excluded", "down_weighted", "status",
                      "elapsed_ms", "device_ms", "linearisations")

    def _baj_inputs(self, obs, R, t, fscale, refine_focal, huber_px):
        """The checks that need no device, as the library makes them (MOCAP_E_ARG), and the arrays in the C layout."""
        C = self.C
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, C, 2) if C else np.ascontiguousarray(obs, dtype=np.float64)
        R = np.array(R, dtype=np.float64, order="C").reshape(-1, 9)
        t = np.array(t, dtype=np.float64, order="C").reshape(-1, 3)
        bad = None
        if C and not (R.shape[0] == C and t.shape[0] == C):
            bad = f"R and t must hold {C} cameras"
        elif refine_focal and C == 2:
            bad = "refine_focal needs at least 3 cameras"
        elif not (np.isfinite(huber_px) and huber_px >= 0):
            bad = "huber_px must be finite and >= 0"
        if bad:
            e = MocapError(f"mocap_core error {MOCAP_E_ARG}: joint bundle adjustment: {bad}")
            e.code = MOCAP_E_ARG
            raise e
        s = None
        if refine_focal:
            s = np.ones(C) if fscale is None else np.array(fscale, dtype=np.float64, order="C").reshape(C)
        return obs, R, t, s

    def ba_joint_normal_eq(self, obs, R, t, X, fscale=None, refine_focal=False, huber_px=0.0, lam=0.0):
        """mocap_ba_joint_normal_eq: one linearisation of the joint problem at the poses (R [C][3][3], t [C][3]), the focal scales
        and the points X [N][3] (NaN rows do not take part) -> {"S" [n_c][n_c], "rhs" [n_c], "cost", "info"}: the Schur-reduced
        camera system at damping `lam`, columns (omega, t) per camera 1 .. C-1, then one focal scale per camera with refine_focal."""
        obs, R, t, s = self._baj_inputs(obs, R, t, fscale, refine_focal, huber_px)
        N = obs.shape[0]
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(N, 3)
        n_c = 6 * (self.C - 1) + (self.C if refine_focal else 0)
        S = np.zeros((max(n_c, 0), max(n_c, 0)))
        rhs = np.zeros(max(n_c, 0))
        cost = ctypes.c_double()
        info = np.zeros(BAJ_INFO)
        self._check(self.lib.mocap_ba_joint_normal_eq(self._h, N, _p(obs), _p(R), _p(t), _p(s), _p(X), BAJ_FOCAL if refine_focal else 0,
                                                      float(huber_px), float(lam), _p(S), _p(rhs), ctypes.addressof(cost), _p(info)))
        return {"S": S, "rhs": rhs, "cost": cost.value, "info": dict(zip(self._BAJ_INFO_KEYS, info.tolist()))}

    def ba_joint_solve(self, obs, R, t, fscale=None, refine_focal=False, huber_px=0.0, ftol=1e-10, max_iter=50):
        """mocap_ba_joint_solve: Levenberg-Marquardt over the poses of cameras 1 .. C-1, every point and (refine_focal) one focal
        scale per camera -> (R [C][3][3], t [C][3], fscale [C] or None, X [N][3], info).  Camera 0 comes back as it went in, |t_1|
        too (the gauge); rows of X whose point did not take part are NaN.  set_ba_progress is honoured."""
        obs, R, t, s = self._baj_inputs(obs, R, t, fscale, refine_focal, huber_px)
        if not (np.isfinite(ftol) and ftol >= 0) or int(max_iter) < 1:
            e = MocapError(f"mocap_core error {MOCAP_E_ARG}: joint bundle adjustment: ftol must be finite and >= 0, max_iter >= 1")
            e.code = MOCAP_E_ARG
            raise e
        N = obs.shape[0]
        X = np.full((N, 3), np.nan)
        info = np.zeros(BAJ_INFO)
        self._check(self.lib.mocap_ba_joint_solve(self._h, N, _p(obs), _p(R), _p(t), _p(s), _p(X), BAJ_FOCAL if refine_focal else 0,
                                                  float(huber_px), float(ftol), int(max_iter), _p(info)))
        info = dict(zip(self._BAJ_INFO_KEYS, info.tolist()))
        info["status"] = int(info["status"])
        return R.reshape(-1, 3, 3), t, s, X, info

    # ------------------------------------------------------------------ lens calibration (poses, points and intrinsics together)
    @staticmethod
    def _bal_refuse(why):
        e = MocapError(f"mocap_core error {MOCAP_E_ARG}: lens calibration: {why}")
        e.code = MOCAP_E_ARG
        raise e

    @staticmethod
    def bal_flags(refine):
        """("focal", "centre", ...) or an integer of BAL_* bits -> the bits."""
        if isinstance(refine, (int, np.integer)):
            return int(refine)
        bits = 0
        for name in refine:
            if name not in BAL_REFINE:
                MocapCore._bal_refuse(f"unknown parameter group {name!r}: {sorted(BAL_REFINE)}")
            bits |= BAL_REFINE[name]
        return bits

    def _bal_inputs(self, obs, R, t, K, dist, refine, huber_px):
        """The checks that need no device, as the library makes them (MOCAP_E_ARG), and the arrays in the C layout."""
        R = np.array(R, dtype=np.float64, order="C").reshape(-1, 9)
        C = R.shape[0]
        t = np.array(t, dtype=np.float64, order="C").reshape(-1, 3)
        K = np.array(K, dtype=np.float64, order="C").reshape(-1, 9)
        dist = np.array(dist, dtype=np.float64, order="C").reshape(-1, 5)
        flags = self.bal_flags(refine)
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if not 2 <= C <= BAL_MAX_CAMERAS:
            self._bal_refuse(f"{C} cameras, 2 .. {BAL_MAX_CAMERAS} are taken")
        if not (t.shape[0] == C and K.shape[0] == C and dist.shape[0] == C):
            self._bal_refuse(f"t, K and dist must hold {C} cameras like R")
        if obs.size % (2 * C) or not 1 <= obs.size // (2 * C) <= BAL_MAX_POINTS:
            self._bal_refuse(f"obs must be [N][{C}][2] with 1 <= N <= {BAL_MAX_POINTS}")
        if flags & ~15:
            self._bal_refuse(f"unknown flag bits {flags:#x}")
        if flags and C == 2:
            self._bal_refuse("intrinsics as unknowns need at least 3 cameras")
        if not (np.isfinite(huber_px) and huber_px >= 0):
            self._bal_refuse("huber_px must be finite and >= 0")
        plain = (K[:, [1, 3, 6, 7]] == 0).all() and (K[:, 8] == 1).all() and np.isfinite(K).all() and (K[:, [0, 4]] > 0).all()
        if not plain or not np.isfinite(dist).all():
            self._bal_refuse("every K must be [[fx,0,cx],[0,fy,cy],[0,0,1]] with fx, fy > 0, every coefficient finite")
        return obs.reshape(-1, C, 2), R, t, K, dist, flags

    def ba_lens_normal_eq(self, obs, R, t, K, dist, X, refine=(), huber_px=0.0, lam=0.0):
        """mocap_ba_lens_normal_eq: one linearisation of the lens calibration at the cameras (R [C][3][3], t [C][3], K [C][3][3],
        dist [C][5] = k1 k2 p1 p2 k3) and the points X [N][3] (NaN rows do not take part) -> {"S" [n_c][n_c], "rhs" [n_c], "cost",
        "info"}: the Schur-reduced camera system at damping `lam`; columns (omega, t) per camera 1 .. C-1, then per camera 0 .. C-1
        the pairs named in `refine` in the order focal, centre, radial, tangential.  Needs no set_cameras."""
        obs, R, t, K, dist, flags = self._bal_inputs(obs, R, t, K, dist, refine, huber_px)
        N, C = obs.shape[:2]
        if not (np.isfinite(lam) and lam >= 0):
            self._bal_refuse("lam must be finite and >= 0")
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(N, 3)
        n_c = 6 * (C - 1) + 2 * bin(flags).count("1") * C
        S = np.zeros((n_c, n_c))
        rhs = np.zeros(n_c)
        cost = ctypes.c_double()
        info = np.zeros(BAL_INFO)
        self._check(self.lib.mocap_ba_lens_normal_eq(self._h, C, N, _p(obs), _p(R), _p(t), _p(K), _p(dist), _p(X), flags, float(huber_px),
                                                     float(lam), _p(S), _p(rhs), ctypes.addressof(cost), _p(info)))
        return {"S": S, "rhs": rhs, "cost": cost.value, "info": dict(zip(self._BAJ_INFO_KEYS, info.tolist()))}

    def ba_lens_solve(self, obs, R, t, K, dist, refine=("focal", "centre", "radial"), huber_px=0.0, ftol=1e-10, max_iter=100):
        """mocap_ba_lens_solve: Levenberg-Marquardt over the poses of cameras 1 .. C-1, every point and the intrinsics named in
        `refine` of every camera -> (R [C][3][3], t [C][3], K [C][3][3], dist [C][5], X [N][3], info).  Camera 0's pose comes back
        as it went in, |t_1| too (the gauge); rows of X whose point did not take part are NaN.  The capture must be raw (taken with
        zero distortion coefficients) and must fill the images.  Needs no set_cameras."""
        obs, R, t, K, dist, flags = self._bal_inputs(obs, R, t, K, dist, refine, huber_px)
        if not (np.isfinite(ftol) and ftol >= 0) or int(max_iter) < 1:
            self._bal_refuse("ftol must be finite and >= 0, max_iter >= 1")
        N, C = obs.shape[:2]
        X = np.full((N, 3), np.nan)
        info = np.zeros(BAL_INFO)
        self._check(self.lib.mocap_ba_lens_solve(self._h, C, N, _p(obs), _p(R), _p(t), _p(K), _p(dist), _p(X), flags, float(huber_px),
                                                 float(ftol), int(max_iter), _p(info)))
        info = dict(zip(self._BAJ_INFO_KEYS, info.tolist()))
        info["status"] = int(info["status"])
        return R.reshape(-1, 3, 3), t, K.reshape(-1, 3, 3), dist, X, info

    def _undistort_inputs(self, K, dist):
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 9)
        dist = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1, 5)
        if not 1 <= K.shape[0] <= BAL_MAX_CAMERAS or dist.shape[0] != K.shape[0]:
            self._bal_refuse(f"K [C][3][3] and dist [C][5] with 1 <= C <= {BAL_MAX_CAMERAS}")
        return K, dist

    def undistort_points(self, points, K, dist):
        """mocap_undistort_points: raw pixels [N][C][2] (NaN = unseen, passed through) -> the ideal pinhole pixels under K [C][3][3]
        and dist [C][5], by UNDISTORT_NEWTON Newton steps per observation on the device.  A camera with zero coefficients is
        copied bit for bit."""
        K, dist = self._undistort_inputs(K, dist)
        C = K.shape[0]
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.size % (2 * C) or not 1 <= pts.size // (2 * C) <= UNDISTORT_MAX_POINTS:
            self._bal_refuse(f"points must be [N][{C}][2] with 1 <= N <= {UNDISTORT_MAX_POINTS}")
        pts = pts.reshape(-1, C, 2)
        out = np.empty_like(pts)
        self._check(self.lib.mocap_undistort_points(self._h, C, pts.shape[0], _p(pts), _p(K), _p(dist), _p(out)))
        return out

    def undistort_points_dev(self, d_in, d_out, n_points, K, dist):
        """mocap_undistort_points_dev: the same on device pointers (integers), enqueued on the context's stream."""
        K, dist = self._undistort_inputs(K, dist)
        self._check(self.lib.mocap_undistort_points_dev(self._h, K.shape[0], int(n_points), ctypes.c_void_p(int(d_in)), _p(K), _p(dist),
                                                        ctypes.c_void_p(int(d_out))))

    # ------------------------------------------------------------------ camera resection
    RESECT_INFO_KEYS = ("valid", "winner_inliers", "winner_hypothesis", "winner_solution", "no_solution", "inliers", "accepted",
                        "linearisations", "rms_prior", "rms_winner", "rms_final", "status")

    def _resect_inputs(self, X, obs, K, prior, threshold_px, n_hyp, n_hyp_min):
        """The checks that need no device, as the library makes them (MOCAP_E_ARG), and the arrays in the C layout."""
        def refuse(why):
            e = MocapError(f"mocap_core error {MOCAP_E_ARG}: camera resection: {why}")
            e.code = MOCAP_E_ARG
            raise e
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        if X.shape[0] != obs.shape[0] or not 1 <= X.shape[0] <= RESECT_MAX_POINTS:
            refuse(f"X [N][3] and obs [N][2] with 1 <= N <= {RESECT_MAX_POINTS}")
        if not n_hyp_min <= int(n_hyp) <= RESECT_MAX_HYP:
            refuse(f"n_hyp must be {n_hyp_min} .. {RESECT_MAX_HYP}")
        if int(n_hyp) == 0 and prior is None:
            refuse("n_hyp = 0 needs a prior pose")
        if not (np.isfinite(threshold_px) and threshold_px > 0):
            refuse("threshold_px must be finite and > 0")
        if (K[[1, 3, 6, 7]] != 0).any() or K[8] != 1 or not (np.isfinite(K[[0, 4, 2, 5]]).all() and K[0] > 0 and K[4] > 0):
            refuse("the intrinsic matrix is not [[fx,0,cx],[0,fy,cy],[0,0,1]] with finite fx, fy > 0")
        pR = pt = None
        if prior is not None:
            pR = np.ascontiguousarray(prior[0], dtype=np.float64).reshape(9)
            pt = np.ascontiguousarray(prior[1], dtype=np.float64).reshape(3)
        return X, obs, K, pR, pt

    def _resect_info(self, info):
        out = dict(zip(self.RESECT_INFO_KEYS, info.tolist()))
        for k in ("valid", "winner_inliers", "winner_hypothesis", "winner_solution", "no_solution", "inliers", "accepted",
                  "linearisations", "status"):
            out[k] = int(out[k])
        return out

    def resect_camera(self, X, obs, K, prior=None, threshold_px=2.0, n_hyp=256, seed=0, min_inliers=6, max_iter=20):
        """mocap_resect_camera: one camera's pose from 3-D points X [N][3] and its pixels obs [N][2] (rows with a NaN are skipped),
        with the camera's own plain K -> (R [3][3], t [3], mask [N] bool, info dict).  prior: (R, t) or None; with one, hypothesis 0
        is the prior.  max_iter = 0 refines nothing, n_hyp = 0 searches nothing: both evaluate the prior only."""
        X, obs, K, pR, pt = self._resect_inputs(X, obs, K, prior, threshold_px, n_hyp, 0)
        if int(min_inliers) < 4 or int(max_iter) < 0:
            e = MocapError(f"mocap_core error {MOCAP_E_ARG}: camera resection: min_inliers must be at least 4, max_iter >= 0")
            e.code = MOCAP_E_ARG
            raise e
        N = X.shape[0]
        R, t, mask, info = np.zeros(9), np.zeros(3), np.zeros(N, dtype=np.uint8), np.zeros(RESECT_INFO)
        self._check(self.lib.mocap_resect_camera(self._h, N, _p(X), _p(obs), _p(K), _p(pR), _p(pt), float(threshold_px), int(n_hyp),
                                                 int(seed), int(min_inliers), int(max_iter), _p(R), _p(t), _p(mask), _p(info)))
        return R.reshape(3, 3), t, mask.astype(bool), self._resect_info(info)

    def resect_camera_dev(self, N, d_X, d_obs, K, prior=None, threshold_px=2.0, n_hyp=256, seed=0, min_inliers=6, max_iter=20):
        """mocap_resect_camera_dev: resect_camera with X [N][3] and obs [N][2] as device pointers, on the context's stream."""
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        pR = pt = None
        if prior is not None:
            pR = np.ascontiguousarray(prior[0], dtype=np.float64).reshape(9)
            pt = np.ascontiguousarray(prior[1], dtype=np.float64).reshape(3)
        R, t, mask, info = np.zeros(9), np.zeros(3), np.zeros(int(N), dtype=np.uint8), np.zeros(RESECT_INFO)
        self._check(self.lib.mocap_resect_camera_dev(self._h, int(N), _vp(d_X), _vp(d_obs), _p(K), _p(pR), _p(pt), float(threshold_px),
                                                     int(n_hyp), int(seed), int(min_inliers), int(max_iter), _p(R), _p(t), _p(mask),
                                                     _p(info)))
        return R.reshape(3, 3), t, mask.astype(bool), self._resect_info(info)

    def resect_hypotheses(self, X, obs, K, prior=None, threshold_px=2.0, n_hyp=256, seed=0):
        """mocap_resect_hypotheses: the candidate table of resect_camera's search -> {"sample" [H][3] input rows (-1: none), "n_sol"
        [H], "poses" [H][4][12] (R | t, NaN where there is no solution), "counts" [H][4]}."""
        X, obs, K, pR, pt = self._resect_inputs(X, obs, K, prior, threshold_px, n_hyp, 1)
        H = int(n_hyp)
        sample, n_sol = np.zeros((H, 3), dtype=np.int32), np.zeros(H, dtype=np.int32)
        poses, counts = np.zeros((H, 4, 12)), np.zeros((H, 4), dtype=np.int32)
        self._check(self.lib.mocap_resect_hypotheses(self._h, X.shape[0], _p(X), _p(obs), _p(K), _p(pR), _p(pt), float(threshold_px), H,
                                                     int(seed), _p(sample), _p(n_sol), _p(poses), _p(counts)))
        return {"sample": sample, "n_sol": n_sol, "poses": poses, "counts": counts}
