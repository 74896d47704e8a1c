/* mocap_core.h -- C ABI of the MI355X-native multi-view marker-tracking core.
 *
 * Drop-in boundary for the hot path of jyjblrd/Low-Cost-Mocap
 * (computer_code/api/helpers.py:203-421).  The reference has no FFI/plugin layer:
 * the seam is four module-level Python functions imported by name at
 * computer_code/api/index.py:1.  A Python module with the same four names
 * (low-cost-mocap_amd/mocap_core/helpers.py) binds these entry points with ctypes;
 * INTEGRATION.md shows the stub a maintainer adds to the reference.
 *
 * Conventions
 *   - plain pointers and sizes only; all matrices row-major; doubles unless stated.
 *   - "host" entry points take caller-owned host buffers, copy in/out and return
 *     after the work finished.  "_dev" entry points take DEVICE pointers, enqueue on
 *     the context's stream and return immediately (mocap_synchronize to wait).
 *   - the library never retains a caller pointer past return.
 *   - return value: 0 = ok, negative = error (MOCAP_E_*); text in mocap_last_error.
 *     Per-frame conditions (candidate/root cap overflow) are reported in `status`,
 *     never by aborting.
 *   - a context is internally locked: calls on one context from several threads
 *     serialise (Flask-SocketIO handlers and the MJPEG generator run on different
 *     threads with no locking, reference helpers.py:84-94 vs :165-186).
 *   - unseen observations are NaN (the reference uses None / [None, None]).
 */
#ifndef MOCAP_CORE_H
#define MOCAP_CORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mocap_ctx mocap_ctx;

enum {
  MOCAP_OK = 0,
  MOCAP_E_ARG = -1,      /* bad argument (null pointer, size out of range)          */
  MOCAP_E_HIP = -2,      /* a HIP runtime call failed                                */
  MOCAP_E_NOCAMS = -3,   /* mocap_set_cameras has not been called                    */
  MOCAP_E_LIMIT = -4,    /* configuration exceeds a compiled limit (see mocap_limits) */
  MOCAP_E_NOCONV = -5    /* solver hit its iteration cap (result still written)      */
};

/* per-frame status bits written by mocap_match_triangulate* */
enum {
  MOCAP_ST_ROOT_OVERFLOW = 1, /* more roots than K_max: frame output invalid          */
  MOCAP_ST_CAND_OVERFLOW = 2, /* a root has more than G_cap candidate groups: invalid */
  MOCAP_ST_HIT_OVERFLOW = 4,  /* wide frames only: a (root, camera) pair has more gated hits
                                 than hit_cap (mocap_set_frame_limits): invalid          */
  MOCAP_ST_ROUNDED = 8,       /* mocap_match_triangulate_f64 only, INFORMATIONAL (outputs valid): a coordinate of the
                                 frame was not representable in float32 and was rounded to the nearest float32 */
  MOCAP_ST_INTRACTABLE = 16,  /* set WITH MOCAP_ST_CAND_OVERFLOW by the re-submit pass: a root of the frame has more than 2^24
                                 candidate groups and the exact search over its multi-hit cameras (csrc/heavy_bb.hip) could not
                                 bound it -- no enumeration reaches it, the reference's own (helpers.py:394-400) included;
                                 bits 20..28 of the status word then hold ceil(log2(groups)) of the largest such root.  The
                                 search runs wherever every intrinsic matrix is plain ([[fx,0,cx],[0,fy,cy],[0,0,1]]), one
                                 matrix for all cameras or one per camera; with a skewed matrix such a root keeps
                                 MOCAP_ST_CAND_OVERFLOW | MOCAP_ST_FINAL alone */
  MOCAP_ST_FINAL = 32         /* set by the re-submit pass on a frame it leaves flagged: larger caps do not exist, a repeated
                                 re-submit skips the frame (frames WITHOUT this bit that are still flagged were not reached:
                                 scratch batch full -- mocap_resubmit_dev continues with them) */
};
#define MOCAP_ST_LOG2_GROUPS_SHIFT 20
#define MOCAP_ST_LOG2_GROUPS_MASK 0x1FF

/* flags for mocap_set_options */
enum {
  MOCAP_OPT_F32_ROUNDING = 1 /* default ON: reproduce OpenCV's float32 roundings of the
                                epipolar line (helpers.py:363) and of the projected point /
                                pixel (helpers.py:231-237).  OFF = all-double arithmetic. */
  ,
  MOCAP_OPT_EXHAUSTIVE_WALK = 2 /* default OFF.  ON: every candidate group of the Cartesian product is triangulated and
                                   reprojected (helpers.py:408-421 as written) -- no eigenvalue bound drops or cuts anything
                                   (csrc/frame_kernel.hip without its cut-offs instead of csrc/frame_bb.hip).  Same results
                                   bit for bit, ~3 x the time: the verification mode bench.py's full-batch parity field and
                                   tests/test_gpu_bench_scale.py compare the shipped selection against. */
  ,
  MOCAP_OPT_BOUNDED_RESUBMIT = 4 /* default OFF.  ON: the re-submit pass of the wide variant does not ENUMERATE the roots its
                                   exact search gives up on (2^16 .. 2^24 groups: ~3 ms of the whole GPU each, csrc/heavy_bb.hip
                                   heavy_enum_kernel); their frames keep MOCAP_ST_CAND_OVERFLOW | MOCAP_ST_FINAL instead.  For
                                   callers that prefer a bounded step time to the last 0.1 % of the frames of a stress batch;
                                   every frame that is returned is still exact.  Means the same on every rig the search runs on
                                   (every intrinsic matrix plain, identical or one per camera). */
};

/* ---------------------------------------------------------------- lifetime */
int mocap_create(int device_id, mocap_ctx** out);
void mocap_destroy(mocap_ctx* ctx);
const char* mocap_last_error(const mocap_ctx* ctx);
const char* mocap_version(void);
/* mocap_last_frame_kernel: which kernel the last frame batch of this context went to ("frame_bb_kernel<CW=1>" = the
 * exact branch-and-bound kernel of csrc/frame_bb.hip, "frame_kernel<256>" = the exhaustive walk, ...).  Diagnostic:
 * results never depend on it.  The string is a literal owned by the library.
 * Which rigs take the search: every intrinsic matrix plain ([[fx,0,cx],[0,fy,cy],[0,0,1]]), <= 16 cameras, <= 64 blobs
 * per camera, <= 255 roots, frames big enough for a 256-lane workgroup.  All cameras sharing ONE matrix report
 * "frame_bb_kernel<CW=1>" / "<CW=2>" (<= 8 / 9-16 cameras); one matrix PER CAMERA, as a calibration gives them, reports
 * "frame_bb_kernel<CW=1, per-camera K>" / "<CW=2, per-camera K>".  A matrix with skew (or any other entry outside that
 * form) sends the rig to the general kernel ("frame_kernel<...>"), as do MOCAP_EVAL_BB=0 and MOCAP_OPT_EXHAUSTIVE_WALK. */
const char* mocap_last_frame_kernel(mocap_ctx* ctx);

/* enqueue on an existing hipStream_t (e.g. the host framework's current stream);
 * NULL restores the context's own stream. */
int mocap_set_stream(mocap_ctx* ctx, void* hip_stream);
int mocap_synchronize(mocap_ctx* ctx);
int mocap_set_options(mocap_ctx* ctx, uint32_t flags);
/* scheduling knobs of the frame path; results are bit-identical for every setting (tested).
 *   frame_threads    workgroup size 64 | 128 | 256 (0 = automatic: 64 for tiny frames, else 256)
 *   heavy_threshold  candidate count above which a frame is cut into slices evaluated by several
 *                    workgroups (-1 = automatic, 0 = never split)
 *   slice_size       target candidates per slice (0 = automatic) */
int mocap_set_tuning(mocap_ctx* ctx, int frame_threads, int heavy_threshold, int slice_size);
/* Frames whose state does not fit the 160 KB of LDS (e.g. 64 cameras x 256 blobs) run through a
 * "wide" variant that keeps hit lists and per-lane group columns in an HBM workspace and caps the
 * gated hits kept per (root, camera) at hit_cap (default 32, 0 = keep; the reference has no cap:
 * overflow sets MOCAP_ST_HIT_OVERFLOW and the frame is re-submitted with a larger cap).
 * force_wide != 0 routes every batch through that variant (tests).  Results are identical. */
int mocap_set_frame_limits(mocap_ctx* ctx, int hit_cap, int force_wide);
/* compiled limits: max cameras, max blobs per camera */
void mocap_limits(int* max_cameras, int* max_blobs);

/* ---------------------------------------------------------------- cameras
 * Replaces the per-call rebuild of P = K [R|t] (helpers.py:305-308, :351-355) and the
 * per-(root, camera) cv.sfm.fundamentalFromProjections (helpers.py:362): builds the
 * projection table (with the reference's "intrinsics by compacted index" quirk,
 * helpers.py:296-298,305-307) and the C x C fundamental table once.
 * K [C][9], R [C][9], t [C][3]: host pointers, copied.  Natural call site:
 * Cameras.start_trangulating_points (helpers.py:171-175). */
int mocap_set_cameras(mocap_ctx* ctx, int C, const double* K, const double* R, const double* t);
/* read back the host-side fundamental table F [C][C][9] (tests / debugging) */
int mocap_get_fundamental(mocap_ctx* ctx, double* F);

/* ---------------------------------------------------------------- triangulation
 * Replaces triangulate_points (helpers.py:330-336) + calculate_reprojection_errors
 * (helpers.py:203-211) for explicit correspondences.
 *   obs [N][C][2]  pixel observations, NaN = unseen
 *   xyz [N][3]     DLT point (NaN row when < 2 views; the reference yields [None]*3)
 *   err [N]        mean squared reprojection error in px^2 (NaN when < 2 views; the
 *                  reference skips the entry).  err may be NULL. */
int mocap_triangulate(mocap_ctx* ctx, int64_t N, const double* obs, double* xyz, double* err);
int mocap_triangulate_dev(mocap_ctx* ctx, int64_t N, const double* d_obs, double* d_xyz, double* d_err);

/* mocap_reproject: replaces calculate_reprojection_errors (helpers.py:203-241) for GIVEN object points:
 * err[i] = mean over the seen cameras' 2 v pixel components of (obs - cv.projectPoints(xyz[i]))^2, NaN when
 * fewer than two cameras see point i (the reference skips the entry).  The three call sites of the reference
 * pass the triangulation of the same observations (helpers.py:272,416; index.py:275), for which
 * mocap_triangulate's `err` output is the same number; this entry honours the function's own contract.
 *   obs [N][C][2] (NaN unseen), xyz [N][3], err [N] */
int mocap_reproject(mocap_ctx* ctx, int64_t N, const double* obs, const double* xyz, double* err);

/* ---------------------------------------------------------------- frame path
 * Replaces find_point_correspondance_and_object_points (helpers.py:339-421) for a
 * batch of independent frames.
 *   blobs  [F][C][M_max][2] float32 pixel centroids (slots >= counts are ignored)
 *   counts [F][C]           int32 blobs per camera (0 = the reference's [[None, None]])
 *   gate_px                 epipolar gate, the reference hard-codes 5 (helpers.py:375,383)
 *   K_max                   capacity for roots / output points per frame
 *   G_cap                   cap on candidate groups per root (the reference enumerates the
 *                           full Cartesian product, helpers.py:394-400)
 * outputs, root order as the reference (camera-0 blobs first, then leftovers of camera 1, ...):
 *   xyz    [F][K_max][3]    winning DLT point per kept root
 *   err    [F][K_max]       its mean squared reprojection error (px^2)
 *   corr   [F][K_max][C]    int16 blob index per camera of the winning group, -1 = none
 *   n_out  [F]              number of points written for the frame (slots beyond are untouched)
 *   status [F]              MOCAP_ST_* bits; non-zero = that frame's outputs are invalid,
 *                           re-submit it with larger caps
 *   n_cand [F]              (may be NULL) candidate groups evaluated for the frame */
int mocap_match_triangulate(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs,
                            const int32_t* counts, double gate_px, int K_max, int64_t G_cap,
                            double* xyz, double* err, int16_t* corr, int32_t* n_out,
                            int32_t* status, int32_t* n_cand);
int mocap_match_triangulate_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs,
                                const int32_t* d_counts, double gate_px, int K_max, int64_t G_cap,
                                double* d_xyz, double* d_err, int16_t* d_corr, int32_t* d_n_out,
                                int32_t* d_status, int32_t* d_n_cand);

/* mocap_resubmit_dev: the re-submit stage of mocap_match_triangulate_dev_auto on its own -- for a batch whose first pass has
 * run (same arguments, same buffers): every frame that is flagged and not MOCAP_ST_FINAL is re-run with the largest caps.
 * A caller that reads d_resubmitted[0] > d_resubmitted[1] after its own synchronisation calls this until the two agree;
 * every call repairs or finalises at least one frame. */
int mocap_resubmit_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs, const int32_t* d_counts,
                       double gate_px, int K_max, double* d_xyz, double* d_err, int16_t* d_corr, int32_t* d_n_out,
                       int32_t* d_status, int32_t* d_n_cand, int32_t* d_resubmitted);

/* mocap_match_triangulate_dev_auto: mocap_match_triangulate_dev, then -- queued behind it on the context's stream, without
 * the host ever waiting -- every frame whose status is non-zero is re-run ON THE DEVICE with the largest caps the core has
 * (root capacity C * M_max as far as a kernel's LDS holds it, G_cap = 2^24 groups per root, every gated hit of a (root,
 * camera) pair kept): the reference enumerates the full product whatever its size (helpers.py:394-400).  The flagged
 * frames are gathered into a scratch batch whose length stays on the device, the frame kernel runs on it, results that
 * fit the caller's K_max slots are scattered back in place.  Status after the call has run: as
 * mocap_match_triangulate_auto (MOCAP_ST_ROOT_OVERFLOW = the frame needs n_out[f] > K_max slots and nothing was written
 * for it; consumers treat n_out > K_max as "no valid slot").  d_resubmitted (may be NULL): [2] device-accessible int32,
 * {frames flagged by the first pass, frames re-run}; the two differ only when the scratch batch could not hold every flagged
 * frame (the whole batch while that takes at most 256 MB, else one frame in eight, within MOCAP_RESUBMIT_SCRATCH_MB, default 8192; halved
 * until the allocation succeeds) -- those keep their status WITHOUT MOCAP_ST_FINAL: mocap_resubmit_dev continues with them
 * (the host-buffer entry points loop until none is left).
 * Where the second pass runs the wide variant and every intrinsic matrix is plain ([[fx,0,cx],[0,fy,cy],[0,0,1]]: one matrix
 * for all cameras or one per camera, as a calibration gives them), a root above 4 096 groups (MOCAP_RESUBMIT_G_CAP) is not
 * enumerated but handed to the exact search of csrc/heavy_bb.hip, which also solves roots no enumeration reaches (above 2^24
 * groups: two markers behind each other as seen from the root's camera); what it cannot bound is enumerated up to 2^24 groups
 * (unless MOCAP_OPT_BOUNDED_RESUBMIT) and flagged MOCAP_ST_INTRACTABLE above.  With a skewed matrix the pass enumerates up to
 * 2^24 groups per root and flags what is larger. */
int mocap_match_triangulate_dev_auto(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs,
                                     const int32_t* d_counts, double gate_px, int K_max, int64_t G_cap,
                                     double* d_xyz, double* d_err, int16_t* d_corr, int32_t* d_n_out,
                                     int32_t* d_status, int32_t* d_n_cand, int32_t* d_resubmitted);

/* mocap_match_triangulate_auto: mocap_match_triangulate, then every frame whose status is non-zero is re-submitted on the
 * GPU with the largest caps the core has (root capacity C * M_max, G_cap = 2^24 groups per root, every gated hit of a
 * (root, camera) pair kept) -- the reference enumerates the full product whatever its size (helpers.py:394-400).  After
 * return a non-zero status means: MOCAP_ST_ROOT_OVERFLOW = the frame is fine but needs n_out[f] > K_max output slots
 * (call again with a larger K_max); other bits = the frame exceeds even the largest caps.  *n_resubmitted (may be NULL)
 * = frames that took the second pass. */
int mocap_match_triangulate_auto(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs,
                                 const int32_t* counts, double gate_px, int K_max, int64_t G_cap, double* xyz,
                                 double* err, int16_t* corr, int32_t* n_out, int32_t* status, int32_t* n_cand,
                                 int32_t* n_resubmitted);

/* mocap_match_triangulate_f64: the same for DOUBLE centroids (the reference measures on whatever its image_points hold,
 * helpers.py:367-373: int64 for _find_dot's int() centroids, float64 for anything else).  blobs [F][C][M_max][2] float64.
 * Coordinates float32 can represent (every integer pixel, every float32-valued centroid) are used exactly; any other is
 * rounded to the nearest float32 and the frame's status gets MOCAP_ST_ROUNDED (informational); NaN / infinite
 * coordinates are MOCAP_E_ARG.  Everything else as mocap_match_triangulate_auto. */
int mocap_match_triangulate_f64(mocap_ctx* ctx, int64_t n_frames, int M_max, const double* blobs, const int32_t* counts,
                                double gate_px, int K_max, int64_t G_cap, double* xyz, double* err, int16_t* corr,
                                int32_t* n_out, int32_t* status, int32_t* n_cand, int32_t* n_resubmitted);

/* ---------------------------------------------------------------- before the path
 * Blob extraction: replaces the per-camera preprocessing of Cameras._camera_read (helpers.py:68-82:
 * np.rot90, make_square helpers.py:507-523, cv.undistort, cv.GaussianBlur (9,9), cv.filter2D with the 5x5
 * sharpening kernel, cv.cvtColor RGB2BGR) and Cameras._find_dot (helpers.py:143-163: grey, threshold
 * 255*0.2, cv.findContours RETR_TREE / CHAIN_APPROX_SIMPLE, cv.moments, int() centroid of every contour
 * with m00 != 0, in findContours' order) for a batch of frame sets.
 *
 * mocap_set_image_params: frame geometry and lens model, once per camera set (natural call site:
 * Cameras.__init__ / set_camera_params, helpers.py:20-22,195-201).  Builds the fixed-point undistortion
 * map cv.undistort would rebuild per frame.
 *   rows, cols   raw frame size (pseyepy RES_SMALL: 240 x 320); must be landscape with >= 8 rows of square
 *                padding above and below -- outside that domain the reference's make_square raises
 *   K [C][9]     intrinsic_matrix, dist [C][5] distortion_coef (k1 k2 p1 p2 k3)   (camera-params.json)
 *   rotation [C] quarter turns of np.rot90 (may be NULL = 0); odd values are rejected like the reference */
int mocap_set_image_params(mocap_ctx* ctx, int C, int rows, int cols, const double* K, const double* dist,
                           const int32_t* rotation);
/* read back camera `camera`'s packed map [S][S] (S = cols): fx | fy << 5 | (sx + 1) << 10 | (sy + 1) << 21,
 * sx field 2047 = every tap outside the frame (tests / debugging) */
int mocap_get_undistort_map(mocap_ctx* ctx, int camera, uint32_t* map);

/* scheduling knob of the blob stage; results are bit-identical for either setting (tested).
 *   skip_dark_tiles  default 1: a 64 x 64 tile whose source bytes span a value range <= 2 (activity map of
 *                    the pre-pass) provably yields no mask bit and is not filtered (exact early-out; IR
 *                    frames are black but for the dots).  0 = filter every tile.  2 (round 6) = the same early-out decided
 *                    INSIDE the mask pass on the range of the tile's undistorted region (no activity pass, no second read
 *                    of the image; a dark tile then pays its gather first). */
int mocap_set_blob_options(mocap_ctx* ctx, int skip_dark_tiles);

/* per-image status bits written by mocap_find_blobs* */
enum {
  MOCAP_BLOB_ST_POINT_OVERFLOW = 1, /* more centroids than M_max: the first M_max were kept            */
  MOCAP_BLOB_ST_CAP_OVERFLOW = 2    /* more than 8192 border pairs / 1024 contours in one image (noise,
                                       not blobs): count = 0                                            */
};
/* mocap_find_blobs
 *   images    [F][C][rows][cols][3] uint8 RGB, what pseyepy's Camera.read() returns per camera
 *   M_max     blob slots per camera
 *   blobs     [F][C][M_max][2] float32 centroids (x, y): exactly the frame path's input layout, so the
 *             _dev variant chains into mocap_match_triangulate_dev without leaving HBM
 *   counts    [F][C] centroids per camera (0 = the reference's [[None, None]], helpers.py:158-159)
 *   status    [F][C] MOCAP_BLOB_ST_* bits
 *   processed [F][C][cols][cols][3] (may be NULL) the BGR frame the reference streams to the UI
 *             (helpers.py:82,141).  Bare by default; with mocap_set_preview_overlay the contours (helpers.py:148) and
 *             centre marks (helpers.py:157) are painted into it on the device -- the coordinate label of helpers.py:156
 *             (cv.putText) is the one drawing that is not.  blobs, counts, status and n_contours never depend on the option.
 *   n_contours [F][C] (may be NULL) contours found, including the zero-area ones the reference skips */
int mocap_find_blobs(mocap_ctx* ctx, int64_t n_frames, const uint8_t* images, int M_max, float* blobs,
                     int32_t* counts, int32_t* status, uint8_t* processed, int32_t* n_contours);
int mocap_find_blobs_dev(mocap_ctx* ctx, int64_t n_frames, const uint8_t* d_images, int M_max, float* d_blobs,
                         int32_t* d_counts, int32_t* d_status, uint8_t* d_processed);

/* ---------------------------------------------------------------- sub-pixel centroids (the core's own contract)
 * The reference's centroid is int(m10 / m00) of the contour polygon (helpers.py:152-155): the truncation discards most of a
 * pixel before the FP64 geometry sees the point.  mocap_set_centroid_mode chooses what the blob stage stores in `blobs`:
 *   MOCAP_CENTROID_REFERENCE = 0  (default) the reference's value: every entry point writes the bytes it wrote before
 *   MOCAP_CENTROID_WEIGHTED  = 1  the grey-weighted centroid defined below
 * Any other value: MOCAP_E_ARG, nothing changes.  The mode is honoured by every call that makes blobs from images:
 * mocap_find_blobs, mocap_find_blobs_dev, mocap_find_blobs_jpeg, mocap_track_frame_images, mocap_track_frame_images_jpeg.
 * The weighted mode leaves the contours, their order and the rule "a slot per contour with m00 != 0, the first M_max kept"
 * as they are: counts, status, n_contours, the mask, `processed` and the JPEG bytes do not change, only the values in
 * `blobs`.  Hole contours are treated like any other contour.  A picture with MOCAP_BLOB_ST_CAP_OVERFLOW keeps count 0, one
 * with MOCAP_BLOB_ST_POINT_OVERFLOW its first M_max slots.  The value of a slot:
 *   window   the inclusive bounding box [x0..x1] x [y0..y1] of the contour's points as findContours(RETR_TREE,
 *            CHAIN_APPROX_SIMPLE) returns them (the extremes of the simplified vertices are those of the full trace)
 *   pixels   those of the window whose mask bit is on: grey > 51, grey = the plane the threshold is applied to
 *            (COLOR_RGB2GRAY of the BGR frame, helpers.py:145-146)
 *   weight   w = grey - 51, an integer in 1 .. 204
 *   sums     sum(w), sum(w x), sum(w y): exact integers, held in 64 bits (one saturated 320 x 320 picture: sum(w x) = 3.3e9)
 *   x = (double)sum(w x) / (double)sum(w), y likewise: IEEE division, rounded once to float32.  sum(w) > 0 always: the
 *            contour's own points are on.
 * Integer sums make the value independent of the order of the reduction: it is bit-reproducible and equals
 * np.float32(np.float64(swx) / np.float64(sw)).  Where two windows of a picture overlap, each takes every mask pixel inside
 * it, its neighbour's included.
 * The preview overlay is not touched: MOCAP_OVERLAY_CENTRES keeps truncating the stored centroid, so in weighted mode the
 * mark sits at the truncated weighted centroid. */
enum {
  MOCAP_CENTROID_REFERENCE = 0,
  MOCAP_CENTROID_WEIGHTED = 1
};
int mocap_set_centroid_mode(mocap_ctx* ctx, int mode);

/* ---------------------------------------------------------------- preview stream
 * The MJPEG preview of the reference (index.py:55-56): frames = cameras.get_frames() (helpers.py:137-141, np.hstack of the
 * processed frames), cv.imencode('.jpg', frames).  The encoder writes the file libjpeg writes with its defaults, byte for
 * byte: baseline sequential, quality as given, YCbCr 4:2:0, JDCT_ISLOW, the standard Huffman tables, no restart markers,
 * JFIF 1.01 APP0 with density 1:1 (SOI, APP0, DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, SOS, scan, EOI).
 *   bgr      [n_images][T][H][W][3] uint8 BGR: the blob stage's `processed` layout for T tiles.  Image f is the H x T*W
 *            picture whose columns t*W .. (t+1)*W-1 are tile t; the hstack is never materialised.  4-byte aligned.
 *   T >= 1; H and W multiples of 16; T*W and H <= 65520; the stream's own shape is 320 x 320*C.  Anything else: MOCAP_E_ARG.
 *   quality  1 .. 100, else MOCAP_E_ARG (libjpeg clamps; this encoder refuses)
 *   jpeg     [n_images][capacity]: every image is an independent file at the start of its slot
 *   sizes    [n_images] bytes the image needs.  An image that needs more than `capacity` writes nothing at or beyond the end of
 *            its slot (the bytes in front are the file's first `capacity` bytes), sets MOCAP_JPEG_ST_OVERFLOW and still
 *            reports the size it needed
 *   status   [n_images] MOCAP_JPEG_ST_* bits (0 = the slot holds the whole file)
 * The output is bit-reproducible from run to run.  The "_dev" form enqueues on the context's stream without any host
 * synchronisation; its workspace lives in the context and grows on demand.
 *
 * mocap_jpeg_bound: an upper bound on one image's bytes, -1 for a size the encoder does not take.  A coded block takes at
 * most 22 bits of DC (an 11-bit code at most, 11 value bits) and 63 x 26 bits of AC (a 16-bit code at most, 10 value bits; zero
 * runs only shorten this): 1660 bits.  With B = 6 * (H / 16) * (W_total / 16) blocks the scan has at most ceil(1660 B / 8) bytes,
 * every one of which may be 0xFF and then carries a stuffed 0x00:  623 (header) + 2 * ceil(1660 B / 8) + 2 (EOI). */
enum {
  MOCAP_JPEG_ST_OVERFLOW = 1 /* the image needs more than `capacity` bytes: sizes[f] says how many */
};
int64_t mocap_jpeg_bound(int H, int W_total);
int mocap_encode_jpeg_dev(mocap_ctx* ctx, int64_t n_images, int T, int H, int W, const uint8_t* d_bgr, int quality,
                          uint8_t* d_jpeg, int64_t capacity, int64_t* d_sizes, int32_t* d_status);
int mocap_encode_jpeg(mocap_ctx* ctx, int64_t n_images, int T, int H, int W, const uint8_t* bgr, int quality, uint8_t* jpeg,
                      int64_t capacity, int64_t* sizes, int32_t* status);
/* mocap_find_blobs with the preview stream instead of `processed`: per frame set one JPEG of its C processed frames side by
 * side (S x S*C, S = cols), encoded where the blob stage left them -- the processed frames never leave the device.
 *   quality, jpeg [F][capacity], capacity   as mocap_encode_jpeg
 *   jpeg_size [F]   bytes the frame set's file needs; > capacity = the slot holds only its first `capacity` bytes
 * everything else as mocap_find_blobs. */
int mocap_find_blobs_jpeg(mocap_ctx* ctx, int64_t n_frames, const uint8_t* images, int M_max, float* blobs, int32_t* counts,
                          int32_t* status, int32_t* n_contours, int quality, uint8_t* jpeg, int64_t capacity,
                          int64_t* jpeg_size);

/* ---------------------------------------------------------------- preview overlays
 * The drawings the reference puts on its preview, painted on the device into pictures of the blob stage's `processed` layout
 * ([F][C][S][S][3] uint8 BGR, S = cols).  Off by default: with flags 0 every entry point writes the bytes it wrote before.
 *   MOCAP_OVERLAY_CONTOURS  cv.drawContours(img, contours, -1, (0,255,0), 1) (helpers.py:148): every pixel a border trace of
 *                           findContours visits, outer or hole -- a mask pixel with one of its four edge neighbours off, the
 *                           outside of the picture counting as off -- becomes (0,255,0)
 *   MOCAP_OVERLAY_CENTRES   cv.circle(img, (cx,cy), 1, (100,255,100), -1) (helpers.py:157): the pixel and its four edge
 *                           neighbours of every stored centroid (the first `counts` of M_max), clipped to the picture; over
 *                           the contours
 *   MOCAP_OVERLAY_EPILINES  one epipolar line per point and camera (drawlines, helpers.py:365), see mocap_draw_epilines
 * Bits 1 and 2 are honoured by the calls that produce a picture: mocap_find_blobs (processed != NULL), mocap_find_blobs_dev
 * (d_processed != NULL), mocap_find_blobs_jpeg and mocap_track_frame_images_jpeg; bit 4 by mocap_track_frame_images_jpeg, which
 * queues the line kernel between its export and the encoder (still one enqueue and one event wait).  A picture whose status
 * carries MOCAP_BLOB_ST_CAP_OVERFLOW is left undrawn.  Any other bit: MOCAP_E_ARG, nothing changes. */
enum {
  MOCAP_OVERLAY_CONTOURS = 1,
  MOCAP_OVERLAY_CENTRES = 2,
  MOCAP_OVERLAY_EPILINES = 4
};
int mocap_set_preview_overlay(mocap_ctx* ctx, uint32_t flags);
/* mocap_draw_epilines: the epipolar lines of a frame batch's points, with the cameras of mocap_set_cameras.
 *   bgr [F][C][S][S][3] in and out; S <= 65535
 *   blobs [F][C][M_max][2], counts [F][C]                          the frame path's inputs
 *   corr [F][K_max][C], n_pts [F] (its n_out), status [F]          its outputs
 * For every point k < n_pts[f] of a frame with status == 0, r = the lowest camera with corr[k][r] >= 0; in the picture of every
 * camera i > r the line (a, b, c) = computeCorrespondEpilines of blob corr[k][r] of camera r under
 * fundamentalFromProjections(P_r, P_i) -- the line the frame kernels gate on, float32 under MOCAP_OPT_F32_ROUNDING -- is
 * painted, in double: |b| >= |a| and b != 0: y = rint(-(a x + c) / b) for every column x; else a != 0: x = rint(-(b y + c) / a)
 * for every row y (rint = to nearest, ties to even); else nothing; pixels outside the picture are dropped.  Point k has colour
 * palette[k % 6], BGR (255,0,0) (0,0,255) (255,255,0) (255,0,255) (0,255,255) (255,128,0); lines are applied in ascending k.
 * (The reference draws, in random colours, the lines of every root alive at camera i, including roots that end with fewer
 * than two views, and raises on a vertical line: this contract is the core's own.)
 * The "_dev" form enqueues on the context's stream; the host form uploads, draws and downloads. */
int mocap_draw_epilines_dev(mocap_ctx* ctx, int64_t n_frames, int S, uint8_t* d_bgr, int M_max, const float* d_blobs,
                            const int32_t* d_counts, int K_max, const int16_t* d_corr, const int32_t* d_n_pts,
                            const int32_t* d_status);
int mocap_draw_epilines(mocap_ctx* ctx, int64_t n_frames, int S, uint8_t* bgr, int M_max, const float* blobs,
                        const int32_t* counts, int K_max, const int16_t* corr, const int32_t* n_pts, const int32_t* status);

/* ---------------------------------------------------------------- after the path
 * World-coordinate epilogue of the frame loop (helpers.py:96-103), fused into the frame path's store:
 * with a matrix set, `xyz` of mocap_match_triangulate* leaves the kernel as
 *   p' = diag(-1,-1,1) p ;  h = to_world [p'; 1] ;  q = h[:3] / h[3] ;  (q.x, q.z, q.y)
 * to_world: 16 doubles row-major (Cameras.to_world_coords_matrix), copied; NULL switches it off. */
int mocap_set_world_transform(mocap_ctx* ctx, const double* to_world);

/* locate_objects (helpers.py:424-480): the 3-LED drone patterns among each frame's points.
 *   xyz [F][K_max][3], err [F][K_max], n_pts [F]   the frame path's outputs (world coordinates)
 *   pos [F][O_max][3]   midpoint of the 0.15 m pair            ("pos")
 *   heading [F][O_max]  -atan2 of the pair direction, folded into [-pi/2, pi/2]   ("heading")
 *   oerr [F][O_max]     mean error of the three points          ("error")
 *   drone [F][O_max]    0 / 1 by the side the lead point is on  ("droneIndex")
 *   lead [F][O_max]     (may be NULL) index of the lead point
 *   n_obj [F]           objects found (entries beyond O_max are dropped, the count is not) */
int mocap_locate_objects(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const double* err,
                         const int32_t* n_pts, int O_max, double* pos, double* heading, double* oerr,
                         int32_t* drone, int32_t* lead, int32_t* n_obj);
int mocap_locate_objects_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz,
                             const double* d_err, const int32_t* d_n_pts, int O_max, double* d_pos,
                             double* d_heading, double* d_oerr, int32_t* d_drone, int32_t* d_lead,
                             int32_t* d_n_obj);

/* mocap_track_frame: the body of the reference's live loop in ONE call (Cameras._camera_read, helpers.py:94-133):
 *   find_point_correspondance_and_object_points (helpers.py:94) -> world coordinates (helpers.py:96-103, needs
 *   mocap_set_world_transform; without it the points stay in camera-0 coordinates) -> locate_objects (helpers.py:107-108,
 *   when O_max > 0 = Cameras.is_locating_objects) -> everything the `object-points` event carries (helpers.py:128-133).
 * One enqueue (frame kernel, then one wave per frame that runs the object search and exports the valid slots into pinned
 * host memory), one event wait; frames that hit a candidate / hit-list cap are re-submitted with the core's largest caps
 * before the call returns -- those frames only, root-capacity overflow included.  Meant for one or a few frames per call
 * (host buffers; for batches use the _dev form).
 *   blobs, counts, gate_px, K_max, G_cap, xyz, err, corr (may be NULL), status   as mocap_match_triangulate
 *   n_pts [F]      points of the frame (mocap_match_triangulate's n_out)
 *   O_max          object slots per frame; 0 = no object search (pos .. n_obj may then be NULL)
 *   pos [F][O_max][3], heading [F][O_max], oerr [F][O_max], drone [F][O_max], n_obj [F]   as mocap_locate_objects
 * status & MOCAP_ST_ROOT_OVERFLOW after return: the frame has n_pts[f] > K_max points (call again with that K_max). */
int mocap_track_frame(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts,
                      double gate_px, int K_max, int64_t G_cap, double* xyz, double* err, int16_t* corr,
                      int32_t* n_pts, int32_t* status, int O_max, double* pos, double* heading, double* oerr,
                      int32_t* drone, int32_t* n_obj);
/* the same from RAW camera frames (helpers.py:68-133: _camera_read's preprocessing + _find_dot in front, needs
 * mocap_set_image_params): images [F][C][rows][cols][3] uint8 RGB (host); additionally returns the image points
 * (blobs [F][C][M_max][2], counts [F][C], blob_status [F][C] as mocap_find_blobs; the `image-points` event of
 * helpers.py:92 reads them). */
int mocap_track_frame_images(mocap_ctx* ctx, int64_t n_frames, const uint8_t* images, int M_max, double gate_px,
                             int K_max, int64_t G_cap, float* blobs, int32_t* counts, int32_t* blob_status,
                             double* xyz, double* err, int16_t* corr, int32_t* n_pts, int32_t* status, int O_max,
                             double* pos, double* heading, double* oerr, int32_t* drone, int32_t* n_obj);
/* mocap_track_frame_images with the preview stream (quality, jpeg, capacity, jpeg_size as mocap_find_blobs_jpeg): the
 * encoder is queued behind the export, its bytes land in the same pinned block as the rest of the payload: still one enqueue
 * and one event wait, and what crosses PCIe is the file, not the frames. */
int mocap_track_frame_images_jpeg(mocap_ctx* ctx, int64_t n_frames, const uint8_t* images, int M_max, double gate_px,
                                  int K_max, int64_t G_cap, float* blobs, int32_t* counts, int32_t* blob_status,
                                  double* xyz, double* err, int16_t* corr, int32_t* n_pts, int32_t* status, int O_max,
                                  double* pos, double* heading, double* oerr, int32_t* drone, int32_t* n_obj, int quality,
                                  uint8_t* jpeg, int64_t capacity, int64_t* jpeg_size);
/* device-pointer form for batches: frame kernel, device-side re-submission of the frames that hit a cap (as
 * mocap_match_triangulate_dev_auto) and object search, all enqueued on the context's stream. */
int mocap_track_frame_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs, const int32_t* d_counts,
                          double gate_px, int K_max, int64_t G_cap, double* d_xyz, double* d_err, int16_t* d_corr,
                          int32_t* d_n_pts, int32_t* d_status, int O_max, double* d_pos, double* d_heading,
                          double* d_oerr, int32_t* d_drone, int32_t* d_n_obj);

/* ---------------------------------------------------------------- rigid bodies (the core's own contract)
 * 6-DoF poses of user-defined marker sets among a frame's 3-D points.  The reference's only object model is locate_objects
 * (two hard-coded 3-LED drones, a position and a folded yaw, nothing when one LED is hidden); this stage is opt-in and the
 * core's own: with no bodies registered nothing that existed before changes.
 *
 * mocap_set_rigid_bodies: registers B <= MOCAP_RB_MAX_BODIES bodies of 3 .. MOCAP_RB_MAX_MARKERS markers each.
 *   n_markers [B], markers [B][8][3] f64 body coordinates (rows >= n_markers[b] are not read): host pointers, copied
 *   tol      metres, > 0: gate on every pairwise distance
 *   max_rms  metres, > 0: a fit whose residual is larger is rejected
 *   work_cap gate-passing extensions one (frame, body) search may make; 0 = MOCAP_RB_DEFAULT_WORK_CAP; < 0 is MOCAP_E_ARG
 * B = 0 clears the registration.  MOCAP_E_ARG, and NOTHING changes (the previous registration stays in force), for: B > 8; a
 * body with fewer than 3 or more than 8 markers; a non-finite coordinate; tol or max_rms not > 0; two markers of one body
 * less than 2 tol apart (D < 2 tol); a body whose full marker set is not posable.
 *   D(p, q) = sqrt(dx dx + dy dy + dz dz), the sum taken in x, y, z order, no fused operation; d_ij = D(q_i, q_j) on the model.
 *   A marker subset is POSABLE iff it has >= 3 markers and holds a triple (i < j < k) with
 *     |(q_j - q_i) x (q_k - q_i)| >= 0.1 |q_j - q_i| |q_k - q_i|
 *   (u = q_j - q_i, v = q_k - q_i, cross = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x), the three norms as D, the
 *   right side as (0.1 |u|) |v|).  The host tabulates this once per body as a 256-bit mask over the subsets; the kernel looks it up.
 *
 * Result per (frame, body).  A frame's points are the first n_pts[f] of its K_max slots; K_max <= MOCAP_RB_MAX_POINTS (64), more
 * is MOCAP_E_ARG; n_pts[f] outside 0 .. K_max counts as 0 (the "no valid slot" rule of mocap_locate_objects).  Bodies are taken in
 * index order; the points claimed by an earlier FOUND body are removed first.  A point with a non-finite coordinate passes no gate.
 *   An ASSIGNMENT is a tuple a[0..N), a[m] = a point index or -1, assigned points distinct, the assigned marker subset posable,
 *   every assigned pair with | D(p_a[i], p_a[j]) - d_ij | < tol (strict).
 *   score = sum over assigned pairs i < j of (D - d_ij)^2, added in (i, j) lexicographic order, unfused.
 *   The winner is the lexicographic minimum of (-number assigned, score, tuple), tuples compared element-wise with -1 below every
 *   index: the optimum over the whole search space, independent of the order of evaluation.  No assignment: not found, status 0.
 *   (An exact duplicate of a point is a valid alternative with an equal score: the smaller index wins.  A body with a symmetry
 *   has several equally good labellings: the one returned is deterministic but arbitrary.)
 * Pose of the winner: centroids qb, pb of the assigned model points and their world points; S = sum (q_i - qb)(p_i - pb)^T; Horn's
 * symmetric 4 x 4 matrix of S; its dominant eigenvector by cyclic Jacobi (accuracy does not rest on an eigen-gap) is the unit
 * quaternion (w, x, y, z) of R; t = pb - R qb; rms = sqrt(mean |R q_i + t - p_i|^2), evaluated in centred coordinates.  R comes
 * from a quaternion, so it is always proper: a mirrored match shows as a large rms.
 *   rms > max_rms: not found, status MOCAP_RB_ST_RMS, nothing claimed.  There is NO second-best search: the body stays unfound for
 *   this frame even if another assignment would have fitted.
 * Work cap: the search is exponential on adversarial input (a lattice of points at the model's own spacings).  It is a depth-first
 * walk over the markers in index order; at marker m the candidate points are those still free that pass the gate against every
 * marker assigned so far, taken in ascending index, then "m unassigned".  A branch is left when the markers assigned plus those
 * still to come cannot reach 3, or cannot reach the largest count of a complete assignment this same search has seen; there is no
 * other pruning.  Every candidate point the walk puts a marker on is one EXTENSION.  The counter is per (frame, body) and starts
 * at zero for each; when it would exceed work_cap the search stops: status MOCAP_RB_ST_WORK_CAP, not found, nothing claimed, later
 * bodies still see the points.  Flag and outputs are a function of the frame's points and the registration alone.
 *
 * Outputs, all [F][B_max] (B_max = body slots per frame, >= the registered bodies, else MOCAP_E_ARG); the entries of a body that
 * is not found, and the slots beyond the registered bodies, are ZERO-filled -- `assign` included: read it only where found = 1.
 *   found i32    1 = found                      n_used i32   assigned markers
 *   assign [8] i8  point index per marker, -1 = unassigned (markers >= N: -1)
 *   R [9] f64 row-major, t [3] f64: world = R body + t      rms f64      score f64 (the winner's)
 *   status i32   0 | MOCAP_RB_ST_RMS | MOCAP_RB_ST_WORK_CAP
 * Out of scope: identity over time (the "body tracker" section below), filtering of the poses, a second-best search, more than
 * 64 points per frame. */
#define MOCAP_RB_MAX_BODIES 8
#define MOCAP_RB_MAX_MARKERS 8
#define MOCAP_RB_MAX_POINTS 64
#define MOCAP_RB_DEFAULT_WORK_CAP 65536
enum {
  MOCAP_RB_ST_RMS = 1,      /* the winner's fit has rms > max_rms: not found */
  MOCAP_RB_ST_WORK_CAP = 2  /* the search needed more than work_cap extensions: not found */
};
int mocap_set_rigid_bodies(mocap_ctx* ctx, int B, const int32_t* n_markers, const double* markers, double tol, double max_rms,
                           int64_t work_cap);
/* xyz [F][K_max][3], n_pts [F]: as the frame path writes them (mocap_match_triangulate's xyz and n_out).  One wave per frame,
 * lane = point.  The "_dev" form enqueues on the context's stream (for batches); the host form uploads, runs and downloads. */
int mocap_locate_rigid_bodies(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts, int B_max,
                              int32_t* found, int32_t* n_used, int8_t* assign, double* R, double* t, double* rms, double* score,
                              int32_t* status);
int mocap_locate_rigid_bodies_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts,
                                  int B_max, int32_t* d_found, int32_t* d_n_used, int8_t* d_assign, double* d_R, double* d_t,
                                  double* d_rms, double* d_score, int32_t* d_status);
/* mocap_track_frame / mocap_track_frame_dev with the body outputs appended (every other argument and every shared output as
 * there, bit for bit).  The host form queues the rigid-body kernel behind the export; it reads the frame's points where the frame
 * path left them and writes into the same pinned block as the rest of the payload: still one enqueue and one event wait.  With
 * no bodies registered the body outputs are zero-filled (and K_max may exceed 64). */
int mocap_track_frame_bodies(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts,
                             double gate_px, int K_max, int64_t G_cap, double* xyz, double* err, int16_t* corr, int32_t* n_pts,
                             int32_t* status, int O_max, double* pos, double* heading, double* oerr, int32_t* drone,
                             int32_t* n_obj, int B_max, int32_t* rb_found, int32_t* rb_n_used, int8_t* rb_assign, double* rb_R,
                             double* rb_t, double* rb_rms, double* rb_score, int32_t* rb_status);
int mocap_track_frame_bodies_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs, const int32_t* d_counts,
                                 double gate_px, int K_max, int64_t G_cap, double* d_xyz, double* d_err, int16_t* d_corr,
                                 int32_t* d_n_pts, int32_t* d_status, int O_max, double* d_pos, double* d_heading,
                                 double* d_oerr, int32_t* d_drone, int32_t* d_n_obj, int B_max, int32_t* d_rb_found,
                                 int32_t* d_rb_n_used, int8_t* d_rb_assign, double* d_rb_R, double* d_rb_t, double* d_rb_rms,
                                 double* d_rb_score, int32_t* d_rb_status);

/* ---------------------------------------------------------------- marker tracker (the core's own contract)
 * Identity over time: which point of this frame is the marker that was which point of the last one.  Every stage above treats a
 * frame on its own; this one gives each marker a number that it keeps while it moves, through a few frames of occlusion and
 * past another marker.  Opt-in and the core's own: with the tracker off nothing that existed before changes.
 *
 * State (on the device, in the context): T_max track slots, 1 <= T_max <= MOCAP_MT_MAX_TRACKS (64), each with
 *   live, id (i32), p[3], v[3] (f64), t_seen (f64), missed, hits (i32)
 * and next_id (i32), which starts at 0.  A session of more than 2^31 - 1 births is out of scope.
 *
 * mocap_set_marker_tracker: allocates and clears the state (and clears it when called again).
 *   T_max       track slots; 0 switches the tracker off and frees the state; < 0 or > 64 is MOCAP_E_ARG
 *   gate        metres, finite and > 0; g2 = gate * gate is formed once on the host in double
 *   max_missed  >= 0: frames a track may go unseen before it is retired
 *   vel_alpha   in [0, 1]: weight of the newest finite-difference velocity
 * A bad value returns MOCAP_E_ARG and NOTHING changes (the previous settings and the state stay in force).
 *
 * One frame at time t has the points x_j, j < n: the first n_pts[f] of its K_max slots as the frame path writes them (world
 * coordinates when a world transform is set).  K_max <= MOCAP_MT_MAX_POINTS (64), more is MOCAP_E_ARG; n_pts[f] outside
 * 0 .. K_max counts as 0 (the "no valid slot" rule of mocap_locate_objects).  A non-finite t: status MOCAP_MT_ST_BAD_TIME,
 * the frame's id are -1, its hits and n_tracks 0, and the state is untouched -- the "_dev" forms report it this way; the host
 * forms reject a non-finite t with MOCAP_E_ARG before anything runs.
 *
 * All arithmetic is IEEE double, no fused operation, in the order written here.
 *   1. Prediction.  For every live slot i: dt_i = t - t_seen_i.  dt_i > 0: pred_i = p_i + v_i * dt_i per component (product,
 *      then sum); otherwise pred_i = p_i.
 *   2. Admissible pairs.  (i, j) is admissible iff slot i is live, point j < n has three finite coordinates, and
 *      d2_ij = dx dx + dy dy + dz dz < g2 (strict), d = x_j - pred_i, the sum taken in x, y, z order.
 *   3. Association.  The admissible pairs are taken in ascending lexicographic order of (d2, slot i, point j); a pair is
 *      committed when neither its slot nor its point has been taken: the greedy global nearest neighbour, a function of the
 *      state and the frame alone, independent of the order of evaluation.
 *   4. Matched slot i with point j.  dt_i > 0: u = (x_j - p_i) / dt_i per component (difference, then IEEE division) and
 *      v_i = v_i + vel_alpha * (u - v_i); otherwise v_i is unchanged.  Then p_i = x_j, t_seen_i = t, missed_i = 0, hits_i += 1.
 *   5. Unmatched live slot.  missed_i += 1; missed_i > max_missed: the track is retired and its slot is free from this moment,
 *      this frame's births included.  A coasting track keeps p, v and t_seen: its prediction goes on extrapolating from its
 *      last sighting.
 *   6. Births.  The unmatched finite points, in ascending j, each take the LOWEST free slot: id = next_id++, p = x_j, v = 0,
 *      t_seen = t, missed = 0, hits = 1.  With no free slot the point gets no track, the frame's status carries
 *      MOCAP_MT_ST_FULL and next_id does not advance.  (The slot rule is part of the contract: slots break ties in step 3.)
 *
 * Outputs per frame:
 *   id [K_max] i32     the track of point j; -1 for slots >= n, non-finite points and points that found no slot
 *   hits [K_max] i32   that track's hits after this frame, 0 where id is -1 (hits >= 2 hides one-frame ghosts)
 *   n_tracks i32       live slots after the frame
 *   status i32         0 | MOCAP_MT_ST_FULL | MOCAP_MT_ST_BAD_TIME
 * Cutting a session into calls of any lengths gives bit-identical outputs and state.  Every entry point of this section
 * returns MOCAP_E_ARG before mocap_set_marker_tracker, with the tracker off, or with K_max > 64.
 * Out of scope: a minimum-cost (Hungarian) assignment, filtering of the positions, identities for rigid bodies, merging or
 * splitting of tracks, more than 64 points or tracks. */
#define MOCAP_MT_MAX_TRACKS 64
#define MOCAP_MT_MAX_POINTS 64
enum {
  MOCAP_MT_ST_FULL = 1,     /* a finite point of the frame found no free slot: it has no track */
  MOCAP_MT_ST_BAD_TIME = 2  /* the frame's time stamp is not finite: no output, the state untouched */
};
int mocap_set_marker_tracker(mocap_ctx* ctx, int T_max, double gate, int max_missed, double vel_alpha);
/* clears all tracks and sets next_id = 0; enqueued on the context's stream */
int mocap_reset_marker_tracker(mocap_ctx* ctx);
/* n_frames consecutive frames, in order: t [F], xyz [F][K_max][3], n_pts [F] (mocap_match_triangulate's xyz and n_out) ->
 * id [F][K_max], hits [F][K_max], n_tracks [F], status [F].  One wave walks the frames, lane = track slot and point.  The
 * "_dev" form enqueues on the context's stream (for batches); the host form uploads, runs and downloads. */
int mocap_track_markers(mocap_ctx* ctx, int64_t n_frames, const double* t, int K_max, const double* xyz, const int32_t* n_pts,
                        int32_t* id, int32_t* hits, int32_t* n_tracks, int32_t* status);
int mocap_track_markers_dev(mocap_ctx* ctx, int64_t n_frames, const double* d_t, int K_max, const double* d_xyz,
                            const int32_t* d_n_pts, int32_t* d_id, int32_t* d_hits, int32_t* d_n_tracks, int32_t* d_status);
/* the live slots in slot order (synchronises): *n of them; id, t_seen, missed, hits [64], pos, vel [64][3] (host) */
int mocap_get_marker_tracks(mocap_ctx* ctx, int32_t* n, int32_t* id, double* pos, double* vel, double* t_seen, int32_t* missed,
                            int32_t* hits);
/* mocap_track_frame / mocap_track_frame_dev with the tracker's outputs appended: t [F] in, mk_id, mk_hits [F][K_max],
 * mk_n_tracks, mk_status [F] out; every other argument and every shared output as there, bit for bit.  The host form queues
 * the tracker behind the export; it reads the frame's points where the frame path left them and writes into the same pinned
 * block as the rest of the payload: still one enqueue and one event wait. */
int mocap_track_frame_ids(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts, double gate_px,
                          int K_max, int64_t G_cap, double* xyz, double* err, int16_t* corr, int32_t* n_pts, int32_t* status,
                          int O_max, double* pos, double* heading, double* oerr, int32_t* drone, int32_t* n_obj, const double* t,
                          int32_t* mk_id, int32_t* mk_hits, int32_t* mk_n_tracks, int32_t* mk_status);
int mocap_track_frame_ids_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs, const int32_t* d_counts,
                              double gate_px, int K_max, int64_t G_cap, double* d_xyz, double* d_err, int16_t* d_corr,
                              int32_t* d_n_pts, int32_t* d_status, int O_max, double* d_pos, double* d_heading, double* d_oerr,
                              int32_t* d_drone, int32_t* d_n_obj, const double* d_t, int32_t* d_mk_id, int32_t* d_mk_hits,
                              int32_t* d_mk_n_tracks, int32_t* d_mk_status);

/* ---------------------------------------------------------------- body tracker (the core's own contract)
 * The registered rigid bodies over time.  The rigid-body stage treats a frame on its own: a body with a symmetry changes its
 * labelling, and so its R, from frame to frame; a body with fewer than three visible markers vanishes; nothing ties body b of
 * this frame to body b of the last.  This stage associates each frame's points against the pose predicted from the last one,
 * falls back on the per-frame search, and coasts through a few frames of occlusion.  Opt-in and the core's own: with the
 * tracker off every entry point that existed before writes the bytes it wrote before.
 *
 * State (on the device, in the context): one slot per registered body b < MOCAP_RB_MAX_BODIES, each with
 *   live (i32), R[9], p[3], v[3], t_seen (f64), missed, hits (i32)       world = R body + p (p is the t of "rigid bodies")
 *
 * mocap_set_body_tracker: on = 1 allocates and clears the state (and clears it when called again); on = 0 switches the tracker
 * off and frees the state, the other arguments are ignored; any other value is MOCAP_E_ARG.
 *   gate        metres, finite and > 0; g2 = gate * gate is formed once on the host in double
 *   max_missed  >= 0: frames a body may coast before its slot is retired
 *   vel_alpha   in [0, 1]: weight of the newest finite-difference velocity
 * A bad value returns MOCAP_E_ARG and NOTHING changes.  tol, max_rms, the models and the posable tables are those of
 * mocap_set_rigid_bodies.  A successful mocap_set_rigid_bodies (B = 0 included) clears the tracker's state -- the slots mean
 * other bodies now -- and keeps its settings; with the tracker off that call does exactly what it did before.
 *
 * One frame at time t.  Inputs: the frame's points x_j, j < n (the first n_pts[f] of its K_max slots; K_max <= 64, more is
 * MOCAP_E_ARG; n_pts[f] outside 0 .. K_max counts as 0, the "no valid slot" rule), and for every body the per-frame search's
 * found[b] and assign[b][8] for this same frame: the search runs first, over the whole batch in parallel, exactly as
 * mocap_locate_rigid_bodies_dev does, and the tracker reads its result arrays.
 * All arithmetic is IEEE double, no fused operation, in the order written; sums of three terms are (a + b) + c.  Cl is the set
 * of points claimed so far in this frame; it starts empty.  Bodies are taken in index order.
 *   1. Prediction (live_b only).  dt = t - t_seen; p^ = p + v * dt per component when dt > 0, else p^ = p; R^ = R (the
 *      orientation is held).
 *   2. Guided association (live_b only), up to two rounds; round 1 starts from (Rc, pc) = (R^, p^).
 *      Predicted markers m^_i[r] = ((Rc[3r] q_i0 + Rc[3r+1] q_i1) + Rc[3r+2] q_i2) + pc[r], i < N.
 *      A pair (marker i, point j) is admissible iff j < n, x_j has three finite coordinates, j is not in Cl and
 *      d2 = dx dx + dy dy + dz dz < g2 (strict), d = x_j - m^_i, the sum taken in x, y, z order.
 *      The admissible pairs are taken in ascending lexicographic (d2, i, j); a pair is committed when neither its marker nor
 *      its point is taken.
 *      The round PASSES iff the assigned marker subset is posable (the body's 256-bit table) and the pose of that assignment --
 *      the procedure of "rigid bodies", unchanged: centroids, S, Horn's matrix, cyclic Jacobi, quaternion -> R, t, rms in
 *      centred coordinates -- has rms <= max_rms.
 *      Round 1 fails: guided fails.  Round 1 passes: round 2 repeats association and fit from round 1's (R, t) over the same
 *      point set (round 1's points are free again); round 2 stands if it passes, otherwise round 1 stands.
 *   3. Outcome, the first that applies.
 *      GUIDED  step 2 gave a result.
 *      SEARCH  found[b] == 1 and none of the search's assigned points is in Cl: the assignment is the search's, the pose is
 *              recomputed by the same procedure (the same arithmetic: the search's own R, t, rms).
 *      COAST   live_b.  missed += 1; missed > max_missed: the slot is retired (live = 0) and the frame's outputs for the body
 *              are those of NONE.  Otherwise the outputs carry (R^, p^) with n_used = 0, assign all -1 and rms = 0.  Nothing is
 *              claimed; R, p, v, t_seen are kept.
 *      NONE
 *   4. Update on GUIDED / SEARCH.  Slot live and dt > 0: u = (t_new - p) / dt per component, v = v + vel_alpha * (u - v);
 *      slot live and dt <= 0: v unchanged; slot not live: v = 0, hits = 0.  Then R = R_new, p = t_new, t_seen = t, missed = 0,
 *      hits += 1, live = 1, and the assigned points join Cl.
 * A non-finite t: status MOCAP_BT_ST_BAD_TIME, the frame's outputs are zero and the state is untouched -- the "_dev" forms
 * report it this way; the host forms reject a non-finite t with MOCAP_E_ARG before anything runs.
 * Cutting a session into calls of any lengths gives bit-identical outputs and state.
 *
 * Outputs, all [F][B_max] but status; zero-filled where source = NONE and in the slots beyond the registered bodies:
 *   tracked i32   1 for GUIDED / SEARCH / COAST          source i32   MOCAP_BT_SRC_NONE | _GUIDED | _SEARCH | _COAST
 *   n_used i32    assigned markers                        assign [8] i8  point index per marker, -1 = unassigned
 *   R [9], t [3], rms f64: world = R body + t             hits, missed i32  the slot's, after the frame
 *   status [F] i32  0 | MOCAP_BT_ST_BAD_TIME
 * Every entry point of this section returns MOCAP_E_ARG with the tracker off, with K_max > 64, with B_max below the registered
 * bodies, or with a null buffer.  With no bodies registered the outputs are zero-filled.
 * Out of scope: angular velocity in the prediction (a body that turns while fully hidden re-acquires through the search and
 * may change labelling there), a partial update from one or two markers, low-pass filtering of the poses, more than 64 points. */
enum {
  MOCAP_BT_SRC_NONE = 0,    /* the body has no pose in this frame */
  MOCAP_BT_SRC_GUIDED = 1,  /* associated against the predicted pose */
  MOCAP_BT_SRC_SEARCH = 2,  /* (re-)acquired from the per-frame search */
  MOCAP_BT_SRC_COAST = 3    /* not seen: the predicted pose */
};
enum {
  MOCAP_BT_ST_BAD_TIME = 1  /* the frame's time stamp is not finite: no output, the state untouched */
};
int mocap_set_body_tracker(mocap_ctx* ctx, int on, double gate, int max_missed, double vel_alpha);
/* clears all slots; enqueued on the context's stream */
int mocap_reset_body_tracker(mocap_ctx* ctx);
/* n_frames consecutive frames, in order: t [F], xyz [F][K_max][3], n_pts [F] (mocap_match_triangulate's xyz and n_out) -> the
 * outputs above.  The search runs into context-owned scratch, then one wave walks the frames, lane = point, both on the
 * context's stream.  The "_dev" form enqueues (for batches); the host form uploads, runs and downloads. */
int mocap_track_bodies(mocap_ctx* ctx, int64_t n_frames, const double* t, int K_max, const double* xyz, const int32_t* n_pts,
                       int B_max, int32_t* tracked, int32_t* source, int32_t* n_used, int8_t* assign, double* R, double* t_pose,
                       double* rms, int32_t* hits, int32_t* missed, int32_t* status);
int mocap_track_bodies_dev(mocap_ctx* ctx, int64_t n_frames, const double* d_t, int K_max, const double* d_xyz,
                           const int32_t* d_n_pts, int B_max, int32_t* d_tracked, int32_t* d_source, int32_t* d_n_used,
                           int8_t* d_assign, double* d_R, double* d_t_pose, double* d_rms, int32_t* d_hits, int32_t* d_missed,
                           int32_t* d_status);
/* all eight slots as they are (synchronises): live, t_seen, missed, hits [8], R [8][9], p, v [8][3] (host) */
int mocap_get_body_tracks(mocap_ctx* ctx, int32_t* live, double* R, double* p, double* v, double* t_seen, int32_t* missed,
                          int32_t* hits);
/* mocap_track_frame_bodies / mocap_track_frame_bodies_dev with t [F] in and the tracker's outputs appended; every other
 * argument and every shared output (the search's rb_* included) as there, bit for bit.  The host form queues the tracker
 * behind the rigid-body kernel and writes into the same pinned block: still one enqueue and one event wait.  Point
 * consolidation is honoured like in the other forms. */
int mocap_track_frame_bodies_tracked(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts,
                                     double gate_px, int K_max, int64_t G_cap, double* xyz, double* err, int16_t* corr,
                                     int32_t* n_pts, int32_t* status, int O_max, double* pos, double* heading, double* oerr,
                                     int32_t* drone, int32_t* n_obj, int B_max, int32_t* rb_found, int32_t* rb_n_used,
                                     int8_t* rb_assign, double* rb_R, double* rb_t, double* rb_rms, double* rb_score,
                                     int32_t* rb_status, const double* t, int32_t* bt_tracked, int32_t* bt_source,
                                     int32_t* bt_n_used, int8_t* bt_assign, double* bt_R, double* bt_t, double* bt_rms,
                                     int32_t* bt_hits, int32_t* bt_missed, int32_t* bt_status);
int mocap_track_frame_bodies_tracked_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs,
                                         const int32_t* d_counts, double gate_px, int K_max, int64_t G_cap, double* d_xyz,
                                         double* d_err, int16_t* d_corr, int32_t* d_n_pts, int32_t* d_status, int O_max,
                                         double* d_pos, double* d_heading, double* d_oerr, int32_t* d_drone, int32_t* d_n_obj,
                                         int B_max, int32_t* d_rb_found, int32_t* d_rb_n_used, int8_t* d_rb_assign,
                                         double* d_rb_R, double* d_rb_t, double* d_rb_rms, double* d_rb_score,
                                         int32_t* d_rb_status, const double* d_t, int32_t* d_bt_tracked, int32_t* d_bt_source,
                                         int32_t* d_bt_n_used, int8_t* d_bt_assign, double* d_bt_R, double* d_bt_t,
                                         double* d_bt_rms, int32_t* d_bt_hits, int32_t* d_bt_missed, int32_t* d_bt_status);

/* ---------------------------------------------------------------- rigid-body learning (the core's own contract)
 * The marker coordinates mocap_set_rigid_bodies wants, learned from a capture of the body in motion: the constellation of the
 * selected track ids averaged over the capture's frames, and how rigid it was.  Inputs as they lie after a session with the
 * marker tracker on: xyz [F][K_max][3], n_pts [F] (the frame path's), id [F][K_max] (the tracker's), status [F] or NULL.  Not a
 * stage of the live loop: with nothing called nothing changes.  All arithmetic is IEEE double, no fused operation.
 *
 * Arguments.  MOCAP_E_ARG, `result` untouched, for: n_frames < 1; K_max outside 1 .. 64; N outside 3 .. 8; a negative or repeated
 * entry in sel [N] (a HOST pointer in both forms); iters outside 1 .. 16; max_rms not > 0 (+inf is allowed: no gate);
 * ref_frame < -1 or >= n_frames; a null buffer (status may be NULL).
 * Valid frame (the calibration tail's rule): status[f] == 0 when a status array is given, and 0 <= n_pts[f] <= K_max.  Slots
 *   >= n_pts[f] are never read.
 * Gather.  In a valid frame marker m is PRESENT at the lowest j < n_pts[f] with id[f][j] == sel[m] and three finite coordinates in
 *   xyz[f][j]; no such j: absent.  In a frame that is not valid every marker is absent.
 * Reference frame.  ref_frame, or with ref_frame = -1 the lowest valid frame in which all N markers are present.  No such frame,
 *   or the given frame not valid and complete: `result` is zero but for [126] = -1 and [128] = MOCAP_LB_ST_NO_REF; the call returns 0.
 *   Template Q^0_m = p_m - c over that frame's N points, c = (sum of the p_m in marker order) * (1.0 / N), per coordinate.
 * Round r = 1 .. iters.  A frame with >= 3 present markers is POSED against Q^(r-1) on its present subset, with the arithmetic of the
 *   rigid-body section's pose, operation for operation: count c; inv = 1.0 / c; centroids qb, pb = (sums in marker order) * inv;
 *   S[i][j] = sum in marker order of (q - qb)_i (p - pb)_j; Horn's 4 x 4 matrix; cyclic Jacobi; the eigenvector of the largest
 *   eigenvalue (the lowest index on a tie) divided by its norm ((w w + x x) + y y) + z z -> R; t_i = pb_i - ((R_i0 qb_0 + R_i1 qb_1) +
 *   R_i2 qb_2); rms = sqrt(ss * inv), ss the sum in (marker, coordinate) order of the squares of ((R_i0 u_0 + R_i1 u_1) + R_i2 u_2) -
 *   (p - pb)_i, u = q - qb.  The frame is USED in round r iff rms <= max_rms.
 *   A used frame maps each present marker back: d = p_m - t, y_k = (R_0k d_0 + R_1k d_1) + R_2k d_2 (y = R^T d), and contributes
 *   y (3 values), 1 to the marker's count, ((e_0 e_0 + e_1 e_1) + e_2 e_2), e = y - Q^(r-1)_m, to the marker's squared error; 1 to
 *   the frames used and rms * rms to the rms sum.  These are reduced over all frames through the tree below.
 *   Q^r_m = (sum y_m) / count_m per coordinate; a marker with count 0 keeps Q^(r-1)_m and sets MOCAP_LB_ST_MARKER_UNSEEN (the flag
 *   stays set through the later rounds).  Then the centroid of all N markers, taken like c above, is subtracted.  The body frame
 *   keeps the orientation the body had in the reference frame; there is no principal-axis step.
 * Pair statistics (independent of the rounds).  For each pair i < j over the frames in which both are present: c_ij the count,
 *   d_ij = (sum D) / c_ij with the rigid-body section's D, and in a second pass s_ij = sqrt((sum (D - d_ij)^2) / c_ij); both 0 when
 *   c_ij = 0.  A marker that is not on the body shows as a large s_ij.
 * One tree, a function of F alone (the calibration tail's): one lane per frame, 256 frames per workgroup, grid ceil(F / 256); lane
 *   -> wave by shuffles (offsets 32 .. 1, v = v + other), wave -> workgroup through LDS in wave order, one partial per workgroup into
 *   a slab; a final launch of one wave whose lane l folds the slab entries [l ceil(P / 64), ...) in index order from 0.0, then the
 *   same shuffle tree.  No atomics.  The final launch of a round leaves Q^r in device memory for the next: the call is one chain of
 *   4 + 2 iters launches on the context's stream, no host round trip inside it.
 * result [MOCAP_LB_RESULT] doubles:
 *   [0, 24)   markers [8][3], rows >= N zero            [24, 32)  per-marker rms of the last round, sqrt(sum |y - q|^2 / count)
 *   [32, 40)  per-marker counts of the last round       [40, 68)  d_ij, (i, j) lexicographic over 8 markers, unused zero
 *   [68, 96)  s_ij          [96, 124) c_ij              [124] frames used in the last round      [125] valid frames
 *   [126] reference frame index      [127] rms of the last round, sqrt(sum rms^2 / used), 0 when none      [128] status flags
 * The "_dev" form enqueues on the context's stream (d_result device-accessible); the host form uploads, runs and downloads. */
#define MOCAP_LB_RESULT 129 /* doubles */
enum {
  MOCAP_LB_ST_NO_REF = 1,        /* no valid frame shows every selected marker (or the given ref_frame does not) */
  MOCAP_LB_ST_MARKER_UNSEEN = 2  /* a marker had no used frame in some round and kept its previous position */
};
int mocap_learn_rigid_body(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts, const int32_t* id,
                           const int32_t* status, int N, const int32_t* sel, int64_t ref_frame, int iters, double max_rms,
                           double* result);
int mocap_learn_rigid_body_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts,
                               const int32_t* d_id, const int32_t* d_status, int N, const int32_t* sel, int64_t ref_frame,
                               int iters, double max_rms, double* d_result);

/* ---------------------------------------------------------------- trajectories (the core's own contract)
 * A recorded session as one time series per marker: the frame-major cloud xyz [F][K_max][3] with the marker tracker's id [F][K_max]
 * gathered into rows, then each row smoothed, short occlusions filled, and velocity and acceleration given beside the position.  Two
 * stages, each with a host and a "_dev" form.  Not a stage of the live loop: with nothing called nothing changes.
 *
 * mocap_gather_tracks[_dev]: traj [R][F][3], time contiguous within a row.
 *   relabel [n_ids] i32: the row of id i; a value outside 0 .. R-1 (-1 by convention) = the id has no row.  Two ids may share a row.
 *   traj[r][f] = xyz[f][j] of the LOWEST slot j < n_pts[f] with 0 <= id[f][j] < n_ids, relabel[id[f][j]] == r,
 *   hits[f][j] >= min_hits (when hits is not NULL) and three finite coordinates; no such slot: three NaN.  n_pts[f] outside
 *   0 .. K_max counts as 0 (the "no valid slot" rule).  Every byte of traj is written.  One lane per frame, no atomics.
 *   MOCAP_E_ARG, traj untouched, for: n_frames < 1; K_max outside 1 .. 64; R outside 1 .. MOCAP_TS_MAX_ROWS; R * n_frames > 2^31;
 *   n_ids < 1; a null buffer (hits may be NULL).  In the "_dev" form every array, relabel included, is device-accessible.
 *
 * mocap_smooth_tracks[_dev]: t [F], traj [R][F][3] (any such table, e.g. a tracked body's t_pose per body) -> pos, vel, acc
 * [R][F][3], res [R][F] f64, n_used, flag [R][F] i32: a local polynomial of degree d per output sample, by least squares.
 *   d        1, 2 or 3                                    W      half window in frames, 1 .. MOCAP_TS_MAX_HALF_WINDOW
 *   span     seconds, > 0; +inf = none                     n_min  d + 1 .. 2 W + 1: samples a fit needs
 *   max_gap  0 .. W: the longest run of missing frames that is filled; 0 = fill nothing
 *   MOCAP_E_ARG, every output untouched, for a value outside these, n_frames < 1, R outside 1 .. MOCAP_TS_MAX_ROWS,
 *   R * n_frames > 2^31 or a null buffer.  The host form also rejects a t with no finite entry.
 * All arithmetic is IEEE double, no fused operation, in the order written here; / and sqrt are correctly rounded.
 *   Good time.  Frame f has a good time iff t_f is finite and t_f > the maximum of the finite t_g, g < f (the maximum of nothing is
 *     -inf): a function of t alone.  The good times increase strictly.
 *   Present.  (r, f) is present iff f has a good time and traj[r][f] is three finite values.
 *   Samples of (r, f), f with a good time: the present frames g of row r with |g - f| <= W and |s_g| <= span, s_g = t_g - t_f;
 *     n is their number.
 *   Fillable.  (r, f) is fillable iff it is not present, max_gap > 0, the nearest present frames a < f < b of the row both exist,
 *     b - a - 1 <= max_gap, and a and b are both samples of (r, f).  (max_gap <= W puts both inside the frame window: a fill is
 *     never an extrapolation.)
 *   flag and n_used, the first rule that applies:
 *     f has no good time             flag = MOCAP_TS_BAD_TIME, n_used = 0
 *     neither present nor fillable   flag = 0, n_used = n
 *     n < n_min                      flag = MOCAP_TS_FEW, n_used = n
 *     a pivot of the fit fails       flag = MOCAP_TS_SINGULAR, n_used = n
 *     otherwise                      flag = MOCAP_TS_SMOOTHED (present) or MOCAP_TS_FILLED (fillable), n_used = n
 *     Only the last rule makes an output; under every other pos, vel, acc and res are NaN.  Every byte of every output is written.
 *   Fit.  h = max |s_g| over the samples (> 0: n >= 2 and good times differ); u_g = s_g / h; p_0 = 1, p_i = p_(i-1) * u_g;
 *     S_i = sum_g p_i for i <= 2 d; B_i[k] = sum_g (p_i * x_g[k]) for i <= d, x_g = traj[r][g]; every sum starts from 0 and takes
 *     the samples in ascending g.  A_ij = S_(i+j), i, j <= d.  Cholesky A = L L^T row by row: for i = 0 .. d, for j = 0 .. i:
 *     s = A_ij, then s = s - L_ik * L_jk for k = 0 .. j-1 in turn; j < i: L_ij = s / L_jj; j = i: the pivot s fails unless it is
 *     finite and > 0, L_ii = sqrt(s).  Per coordinate k: forwards y_i = (B_i[k] - L_i0 * y_0 - ... - L_i,i-1 * y_(i-1)) / L_ii, the
 *     products subtracted in turn, i = 0 .. d; backwards c_i = (y_i - L_(i+1)i * c_(i+1) - ... - L_di * c_d) / L_ii, likewise,
 *     i = d .. 0.
 *   Results.  pos = c_0; vel = c_1 / h; acc = ((2 * c_2) / h) / h for d >= 2, NaN for d = 1;
 *     res = sqrt(ss / (3 n)), ss = the sum from 0, over the samples in ascending g and then k = 0, 1, 2, of e * e,
 *     e = x_g[k] - q, q = c_d, then q = q * u_g + c_i for i = d-1 .. 0 (Horner; product, then sum).
 * Two calls on the same input give the same bytes; the host form and the "_dev" form give the same bytes.  One workgroup of 256
 * lanes per 256 consecutive frames of a row (grid ceil(F / 256) x R) stages its tile and a halo of W frames in LDS; the good-time
 * bits come from a prefix maximum over t in three small launches.  No atomics.  The "_dev" forms enqueue on the context's stream;
 * the host forms upload, run and download.
 * The fragments of one marker that got several ids are found by the next section, "track stitching" (relabel is its seam: it gives
 * them one row).  Out of scope: smoothing of rotations, a fixed-lag or streaming form, weighted windows, outlier rejection, more
 * than 1024 rows or a half window above 32. */
#define MOCAP_TS_MAX_ROWS 1024
#define MOCAP_TS_MAX_HALF_WINDOW 32
enum {
  MOCAP_TS_SMOOTHED = 1,  /* the sample was present and is the fit's value at its own time */
  MOCAP_TS_FILLED = 2,    /* the sample was missing inside a gap of at most max_gap frames: the fit's value */
  MOCAP_TS_FEW = 4,       /* fewer than n_min samples in the window: no output */
  MOCAP_TS_SINGULAR = 8,  /* a Cholesky pivot was not finite or not > 0: no output */
  MOCAP_TS_BAD_TIME = 16  /* the frame's time stamp is not finite or does not exceed every earlier one: no output */
};
int mocap_gather_tracks(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts, const int32_t* id,
                        const int32_t* hits, int min_hits, int n_ids, const int32_t* relabel, int R, double* traj);
int mocap_gather_tracks_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts,
                            const int32_t* d_id, const int32_t* d_hits, int min_hits, int n_ids, const int32_t* d_relabel, int R,
                            double* d_traj);
int mocap_smooth_tracks(mocap_ctx* ctx, int64_t n_frames, int R, const double* t, const double* traj, int degree, int W, double span,
                        int n_min, int max_gap, double* pos, double* vel, double* acc, double* res, int32_t* n_used, int32_t* flag);
int mocap_smooth_tracks_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_t, const double* d_traj, int degree, int W,
                            double span, int n_min, int max_gap, double* d_pos, double* d_vel, double* d_acc, double* d_res,
                            int32_t* d_n_used, int32_t* d_flag);

/* ---------------------------------------------------------------- track stitching (the core's own contract)
 * Which rows of a gathered session are the same marker.  The marker tracker retires a track after max_missed unseen frames (marker
 * tracker, step 5), so a marker hidden for longer comes back under a new id and mocap_gather_tracks gives it a second row, NaN where
 * the first one lives.  This stage links such fragments into chains and numbers the chains; helpers.stitch_table turns that into
 * the relabel of a second mocap_gather_tracks, which then writes one row per marker.  Opt-in: with nothing called nothing changes.
 *
 * mocap_stitch_tracks[_dev]: n_frames, R, t [F], traj [R][F][3] as mocap_gather_tracks writes and mocap_smooth_tracks reads them.
 *   fit_frames  1 .. MOCAP_ST_MAX_FIT: frames at a fragment's end that feed its end model
 *   max_dt      seconds, > 0; +inf allowed: the longest hidden time that is bridged
 *   gate        metres, finite and > 0                  gate_rate  metres per second, finite and >= 0
 *   MOCAP_E_ARG, every output untouched, for a value outside these, n_frames < 1, R outside 1 .. MOCAP_TS_MAX_ROWS,
 *   R * n_frames > 2^31 or a null buffer.  The host form also rejects a t with no finite entry.
 * Outputs, every byte written:
 *   ext [R][3] i32   a_r, b_r, n_r: the first and the last present frame of row r and the number of present ones; -1, -1, 0 for an
 *                    empty row
 *   next, prev [R] i32   the linked successor and predecessor row, -1 = none
 *   cost [R] f64     the cost of the link r -> next[r], NaN where none
 *   chain [R] i32    the row at the head of r's chain (follow prev until it is -1); a row without links, an empty one included, is
 *                    its own head.  An empty row is never linked.
 *   row_of [R] i32   the number of r's chain, chains counted 0, 1, ... in ascending order of their head row; -1 for an empty row
 *   n_chains i32     (one value) the number of chains of non-empty rows
 * All arithmetic is IEEE double, no fused operation, in the order written here; / is correctly rounded; there is no sqrt.
 *   Good time, present.  As in "trajectories": a function of t, and of t and traj[r][f].
 *   Extent.  a_r = the smallest, b_r = the largest present frame of row r, n_r their number.
 *   End models.  Row r, n_r > 0, has a tail model at frame e = b_r over the window lo = max(b_r - fit_frames, 0) .. b_r, and a head
 *     model at e = a_r over a_r .. min(a_r + fit_frames, n_frames - 1).  Samples: the present frames g of the row inside the window
 *     (e is one); m their number; s_g = t_g - t_e; h = the largest |s_g|, found in ascending g from 0.  With m >= 2: u_g = s_g / h;
 *     S0 = sum 1, S1 = sum u_g, S2 = sum (u_g * u_g), B0[k] = sum x_g[k], B1[k] = sum (u_g * x_g[k]), x_g = traj[r][g], every sum from
 *     0 in ascending g; det = S0 * S2 - S1 * S1 (two products, then the difference).  If det is finite and > 0:
 *       pos[k] = (S2 * B0[k] - S1 * B1[k]) / det         (the line's value at t_e, where u = 0)
 *       vel[k] = ((S0 * B1[k] - S1 * B0[k]) / det) / h
 *     With m < 2, or a det that is not finite or not > 0: pos = x_e, vel = 0.  The model's time is t_e.
 *   Pair (p -> q), p != q, n_p > 0, n_q > 0, T = the tail model of p, H = the head model of q.  dt = t_(a_q) - t_(b_p);
 *     g = gate + gate_rate * dt; g2 = g * g; for k = 0, 1, 2:
 *       d_k = H.pos[k] - (T.pos[k] + T.vel[k] * dt)      (where the tail expects the head)
 *       e_k = T.pos[k] - (H.pos[k] - H.vel[k] * dt)      (where the head expects the tail)
 *     d2 = (d_0 * d_0 + d_1 * d_1) + d_2 * d_2, e2 likewise; c = 0.5 * (d2 + e2).  The pair is admissible iff b_p < a_q (strictly
 *     later, never overlapping), dt <= max_dt and c < g2 (false for a NaN on either side).
 *   Association.  The admissible pairs are taken in ascending lexicographic order of (c, p, q); a pair is committed iff p has no
 *     successor yet and q has no predecessor yet: next[p] = q, prev[q] = p, cost[p] = c.  This is the marker tracker's greedy
 *     global nearest neighbour over fragments, and a function of the input alone (the device commits mutually best pairs in
 *     rounds, which gives the same links under this total order).  Links run forward in frames: no chain closes into a cycle.
 *   Chains.  chain[r]: follow prev from r until it is -1.  row_of and n_chains as above.
 * Two calls on the same input give the same bytes; the host form and the "_dev" form give the same bytes.  Extents are combined
 * with 32-bit integer atomics (order-independent); there are no floating-point atomics.  The "_dev" form enqueues on the context's
 * stream (every pointer device-accessible); the host form uploads, runs and downloads.
 * Out of scope: a minimum-cost (Hungarian or min-cost-flow) assignment instead of the greedy one; splitting a track that swapped
 * markers; rigid-body geometry as a cue; overlapping fragments (twins: point consolidation handles those); a streaming form. */
#define MOCAP_ST_MAX_FIT 64
int mocap_stitch_tracks(mocap_ctx* ctx, int64_t n_frames, int R, const double* t, const double* traj, int fit_frames, double max_dt,
                        double gate, double gate_rate, int32_t* ext, int32_t* next, int32_t* prev, double* cost, int32_t* chain,
                        int32_t* row_of, int32_t* n_chains);
int mocap_stitch_tracks_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_t, const double* d_traj, int fit_frames,
                            double max_dt, double gate, double gate_rate, int32_t* d_ext, int32_t* d_next, int32_t* d_prev,
                            double* d_cost, int32_t* d_chain, int32_t* d_row_of, int32_t* d_n_chains);

/* ---------------------------------------------------------------- rigid groups (the core's own contract)
 * Which rows of a gathered session keep their mutual distances: those rows are the markers of one rigid body.  The stage between
 * the session pipeline (track markers, gather, stitch: one row per marker) and the rigid-body pipeline (learn, register, track),
 * which so far started from a hand-typed list of track ids; helpers.find_rigid_groups and helpers.learn_session_bodies are the
 * glue.  Opt-in: with nothing called nothing changes.
 *
 * mocap_rigid_groups[_dev]: n_frames, R, traj [R][F][3] as mocap_gather_tracks writes it.  No time stamps: rigidity does not depend
 * on time.  A sample (r, f) is present iff traj[r][f] is three finite values.
 *   min_common  >= 2: frames two rows must share (and a row must have) to be judged
 *   tol         metres, finite and > 0: the largest standard deviation of a pair's distance that still counts as rigid
 *   max_dist    metres, > 0; +inf allowed: the largest mean distance of an edge
 *   min_travel  metres, finite and >= 0: the smallest bounding-box diagonal of a row that takes part
 *   MOCAP_E_ARG, every output untouched, for a value outside these, n_frames outside 1 .. MOCAP_RG_MAX_FRAMES, R outside
 *   1 .. MOCAP_RG_MAX_ROWS or a null buffer.
 * Outputs, every byte written:
 *   cnt [R][R] i32, dist, spread [R][R] f64   per pair, symmetric, the diagonal included: frames in common, mean and standard
 *                                             deviation of the distance; NaN, NaN where cnt is 0
 *   travel [R] f64                            the diagonal of the row's bounding box; NaN for an empty row
 *   group_of [R] i32                          the row's group, -1 = none
 *   gsize, ghead, gconf [R] i32, gspread [R] f64   per group g < n_groups: rows, lowest row, conflicts, largest spread over its
 *                                             edges; -1, -1, -1, NaN for g >= n_groups
 *   n_groups i32                              (one value)
 * All arithmetic is IEEE double, no fused operation, in the order written here; / and sqrt are correctly rounded.
 *   1. Pair statistics, for p <= q ([q][p] is the copy of [p][q]; the diagonal follows the same rule and gives dist = spread = 0):
 *      over the frames f at which both rows are present, with dx = x_p - x_q, dy, dz likewise:
 *        D_f = sqrt((dx * dx + dy * dy) + dz * dz)
 *        cnt = the number of such frames;  dist = SUM(D) / cnt;  spread = sqrt(SUM((D - dist) * (D - dist)) / cnt), a second pass
 *        over the same frames with the rounded dist; cnt = 0: dist = spread = NaN.
 *   2. SUM is the project's reduction tree (csrc/tree_fold.hpp) over frames in tiles of 256: lane l of tile T carries frame
 *      256 T + l; a frame that is absent for the pair or beyond n_frames carries +0.0.  Within each wave of 64 lanes, for
 *      off = 32, 16, 8, 4, 2, 1 in turn: v[l] = v[l] + v[l + off] for l < off.  The tile's sum is ((w0 + w1) + w2) + w3 over the
 *      v[0] of its four waves.  The P = ceil(n_frames / 256) tile sums are folded by 64 lanes: with c = ceil(P / 64), lane l starts
 *      from 0.0 and adds the tile sums c l, c l + 1, ... below min(c l + c, P) in turn; then the same six halving steps; v[0] is SUM.
 *      (How the device arrives at this association order is its own business -- it folds 64 pairs at once, transposed, and counts
 *      from presence bits -- the bits are not.)
 *   3. Travel.  Over the present samples of row r: e_k = max_k - min_k per axis (exact in any order);
 *      travel = sqrt((e_0 * e_0 + e_1 * e_1) + e_2 * e_2); no present sample: NaN.
 *   4. Row r is eligible iff cnt[r][r] >= min_common and travel[r] >= min_travel.  There is an edge p - q, p != q, iff both rows are
 *      eligible, cnt[p][q] >= min_common, spread[p][q] <= tol and dist[p][q] <= max_dist.  A NaN fails every test.
 *   5. Groups are the connected components of the edge graph with at least two rows, numbered 0, 1, ... by ascending lowest row.
 *      gsize = its rows, ghead = its lowest row, gconf = the pairs p < q inside it with cnt[p][q] >= min_common and NOT
 *      spread[p][q] <= tol (a conflict: the component is a linkage, or two bodies bridged by a marker, not one body),
 *      gspread = the largest spread over its edges.
 * Two calls on the same input give the same bytes; the host form and the "_dev" form give the same bytes.  The bounding boxes are
 * combined with 64-bit integer atomics on an order-preserving key (order-independent); there are no floating-point atomics.  The
 * "_dev" form enqueues on the context's stream (every pointer device-accessible), with no host round trip; the host form uploads,
 * runs and downloads.  The workspace of one call stays under 256 MB: the pairs go through it in rounds.
 * What the stage cannot know: two bodies that never move relative to each other during the capture are one group, and so are
 * markers that lie still (on the floor, on a tripod) -- any two of them keep their distance.  min_travel is the handle for those;
 * a capture in which every body moves on its own is the user's part.
 * Out of scope: robust (median or inlier-fraction) spreads; splitting a linkage at its conflicts; cliques instead of components;
 * more than 256 rows or 2^22 frames; a streaming form; rigid-body geometry as a cue for the stitcher. */
#define MOCAP_RG_MAX_ROWS 256
#define MOCAP_RG_MAX_FRAMES 4194304
int mocap_rigid_groups(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int min_common, double tol, double max_dist,
                       double min_travel, int32_t* cnt, double* dist, double* spread, double* travel, int32_t* group_of,
                       int32_t* gsize, int32_t* ghead, int32_t* gconf, double* gspread, int32_t* n_groups);
int mocap_rigid_groups_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_traj, int min_common, double tol, double max_dist,
                           double min_travel, int32_t* d_cnt, double* d_dist, double* d_spread, double* d_travel,
                           int32_t* d_group_of, int32_t* d_gsize, int32_t* d_ghead, int32_t* d_gconf, double* d_gspread,
                           int32_t* d_n_groups);

/* ---------------------------------------------------------------- body trajectories (the core's own contract)
 * A session's rigid bodies as 6-DoF time series.  Behind "rigid groups" and the learner the rows of a body are known and so are
 * its marker coordinates: the assignment the live body tracker searches for per frame is given.  Three stages, each with a host and
 * a "_dev" form: the pose per (body, frame) from the labelled rows with a sign-continuous quaternion; the orientation smoothed,
 * with angular velocity; the session's rows with hidden markers filled from the body's pose.  The body origin is smoothed by
 * mocap_smooth_tracks itself (t_pose [B][F][3] is a table it accepts).  Offline and opt-in: with nothing called nothing changes;
 * the context's registration (mocap_set_rigid_bodies) is neither read nor changed.
 *
 * The bodies of a call: B in 1 .. MOCAP_BP_MAX_BODIES; n_markers [B] i32, each 3 .. MOCAP_RB_MAX_MARKERS; rows [B][8] i32, the
 * session row of each marker; markers [B][8][3] f64, body coordinates as mocap_learn_rigid_body returns them.  Entries at or beyond
 * n_markers[b] are not read.  The three arrays are HOST memory in both forms (as mocap_set_rigid_bodies' are): the host checks
 * them, tabulates each body's 256-bit posable mask by the rigid-body section's rule, and hands the table to the device inside
 * kernel arguments -- a "_dev" call neither waits nor keeps a pointer to them.
 *   MOCAP_E_ARG, every output untouched, for: B outside 1 .. 64; n_markers[b] outside 3 .. 8; a row outside 0 .. R-1; a row used
 *   twice, within one body or across bodies; a non-finite coordinate; a body whose full marker set is not POSABLE (rigid bodies);
 *   R outside 1 .. MOCAP_TS_MAX_ROWS; R * n_frames > 2^31; n_frames < 1; a null buffer; and what each stage names below.
 * All arithmetic is IEEE double, no fused operation, in the order written here; / and sqrt are correctly rounded.  Every byte of
 * every output is written.  Two calls on the same input give the same bytes; the host form and the "_dev" form give the same
 * bytes.  No floating-point atomics (one 32-bit integer maximum in LDS, exact in any order).
 *
 * 1. mocap_pose_rows[_dev]: traj [R][F][3] as mocap_gather_tracks writes it, the bodies, max_rms (> 0, +inf allowed, else
 *    MOCAP_E_ARG) -> all [B][F]: n_used i32, present i32, quat [4] (w, x, y, z), Rm [9] row-major, t_pose [3], rms f64, flag i32.
 *      present  bit m: traj[rows[b][m]][f] is three finite values (m < n_markers[b]);  n_used = the number of set bits
 *      flag, the first rule that applies:
 *        n_used < 3                                   MOCAP_BP_FEW
 *        the present subset is not posable            MOCAP_BP_DEGENERATE   (the body's table at index `present`)
 *        the fit's rms > max_rms                      MOCAP_BP_RMS
 *        otherwise                                    MOCAP_BP_POSED
 *      The fit (made under RMS and POSED) is the rigid-body section's pose of the present markers, operation for operation, the
 *      markers in ascending m (csrc/rb_pose.hpp): c = n_used, inv = 1 / c; qb, pb = the sums from 0 of the model points and of the
 *      samples, each * inv; per marker mq = q_m - qb, wp = p_m - pb, S_ij = S_ij + mq_i * wp_j from 0; Horn's matrix
 *        A00 = (S00 + S11) + S22, A11 = (S00 - S11) - S22, A22 = (S11 - S00) - S22, A33 = (S22 - S00) - S11, A01 = S12 - S21,
 *        A02 = S20 - S02, A03 = S01 - S10, A12 = S01 + S10, A13 = S20 + S02, A23 = S12 + S21;
 *      cyclic Jacobi, at most 40 sweeps, a sweep begins with off = the sum of |A01|, |A02|, |A03|, |A12|, |A13|, |A23| in that
 *      order and ends the iteration when off == 0; the pairs (p, q) in the order 01, 02, 03, 12, 13, 23; a pair with A_pq == 0
 *      is skipped; with g = 100 |A_pq|, from the fifth sweep on, |A_pp| + g == |A_pp| and |A_qq| + g == |A_qq| set A_pq = 0
 *      instead; else theta = (A_qq - A_pp) / (2 A_pq), t = 1 / (|theta| + sqrt(theta theta + 1)), negated for theta < 0,
 *      cs = 1 / sqrt(t t + 1), sn = t cs, A_pp = A_pp - t A_pq, A_qq = A_qq + t A_pq, A_pq = 0, and for k = 0 .. 3: (k not p, q)
 *      A_kp = cs A_kp - sn A_kq, A_kq = sn A_kp + cs A_kq from the old values, mirrored; V_kp = cs V_kp - sn V_kq,
 *      V_kq = sn V_kp + cs V_kq, V from the identity.  The column of the largest diagonal entry (the first among equals) is
 *      (w, x, y, z); qn = sqrt(((w w + x x) + y y) + z z); each / qn;
 *        R00 = ((w w + x x) - y y) - z z   R01 = 2 (x y - w z)               R02 = 2 (x z + w y)
 *        R10 = 2 (x y + w z)               R11 = ((w w - x x) + y y) - z z   R12 = 2 (y z - w x)
 *        R20 = 2 (x z - w y)               R21 = 2 (y z + w x)               R22 = ((w w - x x) - y y) + z z
 *      t_i = pb_i - ((R_i0 qb_0 + R_i1 qb_1) + R_i2 qb_2); ss = the sum from 0 over the markers and then i = 0, 1, 2 of r r,
 *      r = ((R_i0 mq_0 + R_i1 mq_1) + R_i2 mq_2) - wp_i; rms = sqrt(ss * inv).
 *      Under every flag but POSED quat, Rm and t_pose are NaN; rms is NaN under FEW and DEGENERATE (no fit was made).
 *    Sign continuity.  An eigenvector's sign is arbitrary; a smoother needs one hemisphere.  Over the POSED frames of a body in
 *    ascending f, s = the sign state (0 = as computed, 1 = negated), out = the quaternion written:
 *      the first:   s = 1 iff its first non-zero component in (w, x, y, z) order is negative;
 *      every later: d = ((w w' + x x') + y y') + z z' of the frame's computed quaternion against the previous POSED frame's `out`;
 *                   d < 0: s = 1; d > 0: s = 0; d zero or NaN: s stays what it was (no flip);
 *      out = the computed quaternion, all four components negated iff s = 1.  Rm does not depend on the sign.
 *    Negation is exact, so s is the prefix parity of the flips [d_raw < 0] between consecutive computed quaternions (and the
 *    first frame's bit): the device finds the previous POSED frame by a prefix maximum and the parity by a prefix XOR, in tiles
 *    of 256 frames -- four small launches behind the pose kernel, no walk over frames.
 *
 * 2. mocap_smooth_rotations[_dev]: t [F], quat [B][F][4] (stage 1's), degree, W, span, n_min, max_gap with the ranges and refusals
 *    of mocap_smooth_tracks (B in the place of R: 1 .. MOCAP_BP_MAX_BODIES; the host form also rejects a t with no finite entry)
 *    -> quat_s [B][F][4], omega [B][F][3] (rad/s, world axes), res [B][F] f64, n_used, flag [B][F] i32 (MOCAP_TS_* values).
 *      Good time, samples, fillable, the flag rules and the fit are those of "trajectories", word for word, with four coordinates
 *      k = 0 .. 3 instead of three, and: (b, f) is present iff f has a good time and quat[b][f] is four finite values.
 *      With p = c_0 and p' = c_1 / h (four components each, / per component):
 *        n2 = ((p_w p_w + p_x p_x) + p_y p_y) + p_z p_z; not finite or not > 0: flag = MOCAP_TS_SINGULAR (n_used = n)
 *        quat_s = p / sqrt(n2) per component
 *        omega_x = (2 * ((p_w * p'_x - p'_w * p_x) - (p'_y * p_z - p'_z * p_y))) / n2
 *        omega_y = (2 * ((p_w * p'_y - p'_w * p_y) - (p'_z * p_x - p'_x * p_z))) / n2
 *        omega_z = (2 * ((p_w * p'_z - p'_w * p_z) - (p'_x * p_y - p'_y * p_x))) / n2
 *        res = sqrt(ss / (4 n)), ss over the samples in ascending g and then k = 0 .. 3, Horner as in "trajectories".
 *      omega = 2 vec(p' (x) conj(p)) / |p|^2 is the exact angular velocity of the normalised polynomial; with world = R body it is
 *      expressed in world axes.  Only SMOOTHED and FILLED make an output; under every other flag quat_s, omega and res are NaN.
 *      mocap_smooth_tracks over t_pose with the same parameters gives the same flag and n_used: the presence pattern is the same
 *      (POSED) and the pivots depend on the times alone -- save where this stage's n2 rule fires.
 *
 * 3. mocap_fill_rows[_dev]: traj [R][F][3], the bodies, stage 1's flag, Rm, t_pose [B][F], and optionally -- all three or none
 *    (NULL), anything else is MOCAP_E_ARG -- flag_s [B][F] i32, quat_s [B][F][4] (stage 2's) and pos_s [B][F][3]
 *    (mocap_smooth_tracks' pos over t_pose) -> filled [R][F][3] f64, src [R][F] i32, per (row, frame) by the first rule that applies:
 *      traj[r][f] is three finite values                          those bytes, MOCAP_BP_SRC_MEASURED
 *      r is marker m of body b and flag[b][f] is POSED            x_i = ((Rm_i0 * q_0 + Rm_i1 * q_1) + Rm_i2 * q_2) + t_pose_i,
 *                                                                 q = markers[b][m], MOCAP_BP_SRC_RIGID
 *      ... the optional arrays are given and flag_s[b][f] is      R from quat_s[b][f] by the formula of stage 1,
 *          MOCAP_TS_FILLED                                        x_i = ((R_i0 * q_0 + R_i1 * q_1) + R_i2 * q_2) + pos_s_i,
 *                                                                 MOCAP_BP_SRC_RIGID_FILLED
 *      otherwise                                                  three NaN, MOCAP_BP_SRC_NONE
 *    A row of no body falls under the first and the last rule only.  filled is a table mocap_smooth_tracks, mocap_stitch_tracks
 *    and mocap_rigid_groups read unchanged.  A marker hidden for seconds is there as long as three others of its body that span
 *    a plane are seen.
 * One lane per (body, frame) for the poses and per (row, frame) for the fill, frames along the lanes; the rotation smoother stages
 * 256 frames and a halo of W in LDS as "trajectories" does.  The "_dev" forms enqueue on the context's stream (every pointer but
 * the body description device-accessible), with no host round trip; the host forms upload, run and download.
 * Out of scope: angular acceleration; a geodesic (SO(3)) fit instead of the component-wise polynomial; re-learning the template
 * from the filled rows; body geometry as a cue for the stitcher; a pose from fewer than three markers; weighted or robust fits; a
 * streaming form; more than 64 bodies or 8 markers per body; writing C3D or TRC files. */
#define MOCAP_BP_MAX_BODIES 64
enum {
  MOCAP_BP_POSED = 1,       /* a pose was fitted to the present markers and its rms is within max_rms */
  MOCAP_BP_FEW = 2,         /* fewer than three markers of the body are present: no fit */
  MOCAP_BP_DEGENERATE = 4,  /* the present markers are not a posable subset (collinear): no fit */
  MOCAP_BP_RMS = 8          /* the fit's rms exceeds max_rms: rms is written, the pose is not */
};
enum {
  MOCAP_BP_SRC_NONE = 0,         /* no sample and nothing to fill it from: NaN */
  MOCAP_BP_SRC_MEASURED = 1,     /* the row's own sample */
  MOCAP_BP_SRC_RIGID = 2,        /* the frame's pose applied to the marker's body coordinates */
  MOCAP_BP_SRC_RIGID_FILLED = 3  /* the smoothers' gap-filled pose applied to them */
};
int mocap_pose_rows(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int B, const int32_t* n_markers, const int32_t* rows,
                    const double* markers, double max_rms, int32_t* n_used, int32_t* present, double* quat, double* Rm, double* t_pose,
                    double* rms, int32_t* flag);
int mocap_pose_rows_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_traj, int B, const int32_t* n_markers,
                        const int32_t* rows, const double* markers, double max_rms, int32_t* d_n_used, int32_t* d_present,
                        double* d_quat, double* d_Rm, double* d_t_pose, double* d_rms, int32_t* d_flag);
int mocap_smooth_rotations(mocap_ctx* ctx, int64_t n_frames, int B, const double* t, const double* quat, int degree, int W, double span,
                           int n_min, int max_gap, double* quat_s, double* omega, double* res, int32_t* n_used, int32_t* flag);
int mocap_smooth_rotations_dev(mocap_ctx* ctx, int64_t n_frames, int B, const double* d_t, const double* d_quat, int degree, int W,
                               double span, int n_min, int max_gap, double* d_quat_s, double* d_omega, double* d_res,
                               int32_t* d_n_used, int32_t* d_flag);
int mocap_fill_rows(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int B, const int32_t* n_markers, const int32_t* rows,
                    const double* markers, const int32_t* flag, const double* Rm, const double* t_pose, const int32_t* flag_s,
                    const double* quat_s, const double* pos_s, double* filled, int32_t* src);
int mocap_fill_rows_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_traj, int B, const int32_t* n_markers,
                        const int32_t* rows, const double* markers, const int32_t* d_flag, const double* d_Rm, const double* d_t_pose,
                        const int32_t* d_flag_s, const double* d_quat_s, const double* d_pos_s, double* d_filled, int32_t* d_src);

/* ---------------------------------------------------------------- joints (the core's own contract)
 * Which bodies of a recorded session are joined, where, and how.  "body trajectories" ends at bodies that know nothing of each other;
 * this section finds, for every pair of bodies, the point (ball joint) or the line (hinge) the two share throughout the capture,
 * builds a skeleton from the pairs that have one, and gives a joint's motion per frame.  The fit is the classical linear one:
 * symmetrical centre of rotation estimation (SCoRE) for the centre, symmetrical axis of rotation analysis (SARA) for the axis.
 * Offline and opt-in: with nothing called nothing changes.  helpers.session_joints and helpers.session_joint_motion are the glue.
 *
 * A. mocap_find_joints[_dev]: n_frames F in 1 .. MOCAP_RG_MAX_FRAMES; B in 2 .. MOCAP_BP_MAX_BODIES; flag [B][F] i32, Rm [B][F][9],
 *    t_pose [B][F][3] as mocap_pose_rows writes them;
 *      min_common  >= 6: frames two bodies must share to be judged
 *      tol_rank    finite, in (0, 1): an eigenvalue at or below it counts as zero
 *      max_sep     metres, > 0; +inf allowed: the largest rms distance between the two images of a joint's centre
 *    MOCAP_E_ARG, every output untouched, for a value outside these or a null buffer.
 *    All arithmetic is IEEE double, no fused operation, in the order written here; / and sqrt are correctly rounded.
 *    1. Pair sums, per pair a < b, over the frames f at which both flags are MOCAP_BP_POSED and the 24 values Rm_a, t_a, Rm_b, t_b
 *       are finite (n = their number, exact):
 *         Rel_ij = (Rm_a[0][i] * Rm_b[0][j] + Rm_a[1][i] * Rm_b[1][j]) + Rm_a[2][i] * Rm_b[2][j]      (Rel = Rm_a^T Rm_b)
 *         dt = t_b - t_a per component;  d_i = (Rm_a[0][i] * dt_0 + Rm_a[1][i] * dt_1) + Rm_a[2][i] * dt_2   (d = Rm_a^T (t_b - t_a))
 *         g_j = (Rel_0j * d_0 + Rel_1j * d_1) + Rel_2j * d_2                                      (g = Rel^T d)
 *         dd = (d_0 * d_0 + d_1 * d_1) + d_2 * d_2
 *       Sixteen sums: the nine Rel_ij, d (3), g (3) and dd, each by SUM exactly as "rigid groups" item 2 defines it (tiles of 256
 *       frames, the tree of csrc/tree_fold.hpp, an absent frame carries +0.0).  (No output of this version depends on SUM(dd): it fills the
 *       sixteenth slot of a pair's fold, and is what a closed-form residual would start from.)  How the device arrives at that association
 *       order is its own business.
 *    2. System.  Rbar = SUM(Rel) / n per entry, dbar, gbar likewise;  M = [[I, -Rbar], [-Rbar^T, I]], 6 x 6, I with exact 1 and 0;
 *       rhs = (dbar_0, dbar_1, dbar_2, -gbar_0, -gbar_1, -gbar_2).  Cyclic Jacobi on M by the very rules "body trajectories" item 1
 *       spells out for Horn's 4 x 4 matrix -- the sweep's off = the sum of the |A_pq| in pair order and the end at off == 0, the skip
 *       rule, the g = 100 |A_pq| rule from the fifth sweep on, the rotation formulae, V from the identity -- with the index running
 *       0 .. 5, k = 0 .. 5, and the 15 pairs in lexicographic order 01, 02, .. 05, 12, .. 45; at most 30 sweeps (every input of the
 *       tests ends within 9; the limit only bounds a matrix with a NaN in it).  lambda = the diagonal, ordered ascending, the lower
 *       index first among equals.
 *    3. Kind, the first rule that applies:
 *         n < min_common                          MOCAP_JT_UNSEEN    nothing computed, every double NaN
 *         a lambda or an entry of V not finite    MOCAP_JT_SINGULAR  every double NaN
 *         two or more lambda <= tol_rank          MOCAP_JT_FIXED     the bodies did not turn against each other: no centre is determined
 *         exactly one lambda <= tol_rank          MOCAP_JT_HINGE
 *         none                                    MOCAP_JT_BALL
 *    4. Solution, the minimum-norm one: x = 0; over the k with lambda_k > tol_rank in the order of item 2:
 *       h = (the sum from 0 over i = 0 .. 5 of V_ik * rhs_i) / lambda_k, then x_i = x_i + h * V_ik.  c_a = x[0 .. 3) in a's coordinates,
 *       c_b = x[3 .. 6) in b's.  Under HINGE every point of the axis is a centre; the one found is the point of the axis this
 *       minimum-norm rule picks (the one nearest the two bodies' origins, taken together), not a point of any anatomical meaning.
 *       Under FIXED it is whatever the kept directions give.
 *    5. Axis, under HINGE only (else NaN): with k0 the first of the order, axis_a = (V_0k0, V_1k0, V_2k0) / na,
 *       na = sqrt((x * x + y * y) + z * z) of those three, axis_b likewise from the rows 3 .. 5 with its own norm nb; both are negated
 *       iff the first non-zero component of axis_a is negative.  na or nb not > 0: MOCAP_JT_SINGULAR.
 *    6. Residual, a second pass over the same frames with the rounded centres, under FIXED, HINGE and BALL:
 *         w_a,i = ((Rm_a[i][0] * c_a0 + Rm_a[i][1] * c_a1) + Rm_a[i][2] * c_a2) + t_a,i;  w_b likewise;  e = w_a - w_b
 *         sep = sqrt(SUM((e_0 * e_0 + e_1 * e_1) + e_2 * e_2) / n)
 *       accepted iff the kind is HINGE or BALL and sep <= max_sep (a NaN fails).
 *    7. Skeleton.  Kruskal over the accepted pairs a < b in ascending order of (the bits of sep as an unsigned integer, a, b): a pair
 *       whose bodies are not yet connected becomes a tree edge.  In each component the lowest body is the root;
 *       parent[b] = b's neighbour on the tree path towards its root, -1 for a root and for a body with no accepted pair;
 *       n_joints = the number of tree edges.
 *    Outputs, every byte written; each [B][B] table is symmetric save centre and axis:
 *      cnt [B][B] i32        n; the diagonal follows the same rule (the body's POSED frames with twelve finite values)
 *      kind [B][B] i32       MOCAP_JT_*; the diagonal is UNSEEN
 *      accepted [B][B] i32   the diagonal is 0
 *      lam [B][B][3] f64     the three smallest lambda in order
 *      sep [B][B] f64
 *      centre [B][B][3] f64  centre[p][q] is the joint of the pair {p, q} IN p's COORDINATES: c_a at [a][b], c_b at [b][a]
 *      axis [B][B][3] f64    likewise: axis_a at [a][b], axis_b at [b][a]
 *      parent [B] i32, n_joints i32 (one value)
 *    Two calls on the same input give the same bytes, and so do the host form and the "_dev" form (any NaN equal to any NaN).  No
 *    floating-point atomics.  The "_dev" form enqueues on the context's stream (every pointer device-accessible) and does not wait;
 *    the host form uploads, runs and downloads.  The workspace of one call stays under 256 MB: the pairs go through it in rounds.
 *
 * B. mocap_joint_series[_dev]: a joint's motion per frame.  The joints of a call: J in 1 .. MOCAP_JT_MAX_JOINTS; body_a, body_b [J]
 *    i32 (in 0 .. B-1, different), kind [J] i32 (a MOCAP_JT_* value), c_a, c_b [J][3] (finite), axis_b [J][3] (read and finite under
 *    HINGE), q_ref [J][4] (w, x, y, z; finite, |q|^2 within 1e-6 of 1): a reference orientation of b in a, the identity allowed.
 *    These seven arrays are HOST memory in both forms: the host checks them and hands them to the device inside kernel arguments, as
 *    "body trajectories" does with its bodies -- a "_dev" call neither waits nor keeps a pointer to them.  flag [B][F] i32,
 *    quat [B][F][4], Rm [B][F][9], t_pose [B][F][3] are mocap_pose_rows'; n_frames and B as under A.
 *    MOCAP_E_ARG, every output untouched, for anything else or a null buffer.
 *    Per (joint j, frame f), all [J][F]:
 *      present i32      1 iff both flags are MOCAP_BP_POSED; every double below is NaN where it is 0
 *      centre [3]       w_a, w_b as in A.6 from the given c_a, c_b;  centre_i = (w_a,i + w_b,i) * 0.5
 *      gap              e = w_a - w_b;  gap = sqrt((e_0 * e_0 + e_1 * e_1) + e_2 * e_2)
 *      quat_rel [4]     conj(q_ref) (x) (conj(q_a) (x) q_b), conj negating x, y, z, the Hamilton product p (x) q term by term:
 *                         w = ((p_w * q_w - p_x * q_x) - p_y * q_y) - p_z * q_z      x = ((p_w * q_x + p_x * q_w) + p_y * q_z) - p_z * q_y
 *                         y = ((p_w * q_y - p_x * q_z) + p_y * q_w) + p_z * q_x      z = ((p_w * q_z + p_x * q_y) - p_y * q_x) + p_z * q_w
 *                       mocap_pose_rows' sign walk makes q_a and q_b continuous along f, so the product is continuous too.
 *      twist [2]        under HINGE: s = (x * ax + y * ay) + z * az of quat_rel against axis_b, m = sqrt(w * w + s * s),
 *                       twist = (w / m, s / m): cosine and sine of HALF the hinge angle against q_ref.  NaN where m is not > 0 and
 *                       under every other kind.
 *    There is no atan2 on the device: the angle 2 atan2(twist_1, twist_0) is the helper's step, so every double here is + - * / sqrt.
 *    quat_rel [J][F][4] is a table mocap_smooth_rotations accepts unchanged (J in the place of B), centre [J][F][3] one
 *    mocap_smooth_tracks accepts.  One lane per (joint, frame), frames along the lanes.
 * Out of scope: joints between more than two bodies; universal or sliding joints as kinds of their own; robust fits; weighting by
 * marker count; a streaming form. */
#define MOCAP_JT_MAX_JOINTS 64
enum {
  MOCAP_JT_UNSEEN = 0,    /* fewer than min_common frames in common: nothing computed */
  MOCAP_JT_SINGULAR = 1,  /* the eigen-problem gave a value that is not finite */
  MOCAP_JT_FIXED = 2,     /* two or more eigenvalues at or below tol_rank: the bodies did not turn against each other */
  MOCAP_JT_HINGE = 3,     /* exactly one: a line is shared */
  MOCAP_JT_BALL = 4       /* none: a point is shared (if sep says so) */
};
int mocap_find_joints(mocap_ctx* ctx, int64_t n_frames, int B, const int32_t* flag, const double* Rm, const double* t_pose,
                      int min_common, double tol_rank, double max_sep, int32_t* cnt, int32_t* kind, int32_t* accepted, double* lam,
                      double* sep, double* centre, double* axis, int32_t* parent, int32_t* n_joints);
int mocap_find_joints_dev(mocap_ctx* ctx, int64_t n_frames, int B, const int32_t* d_flag, const double* d_Rm, const double* d_t_pose,
                          int min_common, double tol_rank, double max_sep, int32_t* d_cnt, int32_t* d_kind, int32_t* d_accepted,
                          double* d_lam, double* d_sep, double* d_centre, double* d_axis, int32_t* d_parent, int32_t* d_n_joints);
int mocap_joint_series(mocap_ctx* ctx, int64_t n_frames, int B, const int32_t* flag, const double* quat, const double* Rm,
                       const double* t_pose, int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind, const double* c_a,
                       const double* c_b, const double* axis_b, const double* q_ref, int32_t* present, double* centre, double* gap,
                       double* quat_rel, double* twist);
int mocap_joint_series_dev(mocap_ctx* ctx, int64_t n_frames, int B, const int32_t* d_flag, const double* d_quat, const double* d_Rm,
                           const double* d_t_pose, int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind,
                           const double* c_a, const double* c_b, const double* axis_b, const double* q_ref, int32_t* d_present,
                           double* d_centre, double* d_gap, double* d_quat_rel, double* d_twist);

/* ---------------------------------------------------------------- joint poses (the core's own contract)
 * Bodies with hidden markers posed through their joints.  mocap_pose_rows poses every body alone: with fewer than three markers
 * seen, or a collinear set, the frame is MOCAP_BP_FEW or MOCAP_BP_DEGENERATE and its pose NaN.  With the skeleton of "joints" known
 * such a frame is determined by a neighbour's pose: a ball joint gives the hidden body one point, a hinge a line, and the fit is
 * stage 1's own with one or two more correspondences.  The fit propagates along the skeleton from every posed body.  Offline and
 * opt-in: with nothing called nothing changes.  helpers.session_joint_poses is the glue.
 *
 * mocap_pose_joints[_dev]:
 *   traj [R][F][3], R, n_frames F, and the bodies (B, n_markers, rows, markers; HOST memory) with the ranges and refusals of "body
 *     trajectories"; B in 2 .. MOCAP_BP_MAX_BODIES.
 *   flag [B][F] i32, quat [B][F][4], Rm [B][F][9], t_pose [B][F][3]: mocap_pose_rows' outputs over the same traj and bodies.
 *   The joints, HOST memory in both forms as "joints" B takes them (checked on the host, handed to the device inside kernel
 *     arguments; a "_dev" call neither waits nor keeps a pointer to them): J in 1 .. B-1; body_a, body_b [J] i32 in 0 .. B-1 and
 *     different; kind [J] i32, MOCAP_JT_HINGE or MOCAP_JT_BALL only; c_a, c_b [J][3] finite: the joint's centre in a's and in b's
 *     coordinates; axis_a, axis_b [J][3]: the hinge's axis in a's and in b's coordinates as mocap_find_joints signs them (both map to
 *     ONE world direction), read under HINGE alone and then finite with (x x + y y) + z z within 1e-6 of 1.  The joints form a
 *     forest: no pair of bodies appears twice and there is no cycle (a union-find over the bodies in joint order).
 *   axis_len   metres, finite, > 0: how far along the axis a hinge's second virtual point lies
 *   max_rms    metres, > 0, +inf allowed: the largest rms of a fit through a joint
 *   max_rounds 1 .. MOCAP_JP_MAX_ROUNDS: how many joints away from a POSED body a pose may travel
 *   MOCAP_E_ARG, every output untouched, for anything else or a null buffer.
 *   -> all [B][F]: flag_j, hops, via i32; quat_j [4], Rm_j [9], t_j [3], rms_j f64.
 * All arithmetic is IEEE double, no fused operation, in the order written here; / and sqrt are correctly rounded.  Every byte of
 * every output is written.  Two calls on the same input give the same bytes, and so do the host form and the "_dev" form (any NaN
 * equal to any NaN).  No floating-point atomics (one 32-bit integer maximum in LDS, exact in any order).
 * Per frame f:
 *   Round 0.  A body whose flag is MOCAP_BP_POSED: hops = 0, via = -1, flag_j = POSED, quat_j, Rm_j, t_j = its quat, Rm, t_pose
 *     (copied), rms_j = NaN.  Every other body starts with hops = -1.
 *   Round r = 1 .. max_rounds.  A body y with hops = -1 whose input flag is FEW or DEGENERATE is a candidate (an RMS frame never
 *     is).  Its joints are tried in ascending joint index; a joint is tried only if its other body x has hops = r - 1 exactly (so
 *     every directed joint is tried at most once per frame, and a body is posed from the nearest posed body of its tree).  The first
 *     try that succeeds sets flag_j = MOCAP_BP_JOINTED, hops = r, via = the joint's index and the four doubles' tables; a failed
 *     try leaves y a candidate for its later joints and for later rounds.
 *   A try of y through a joint with x.  Presence is stage 1's (traj[rows[y][m]][f] is three finite values), k = the number present.
 *     The point list: the present markers of y in ascending m (model markers[y][m], world the sample), then the joint's virtual
 *     points, with c_y, axis_y the joint's centre and axis in y's coordinates, c_x, axis_x in x's, and Rx, tx = Rm_j, t_j of x:
 *       first    model v0 = c_y;  world w0_i = ((Rx_i0 * c_x0 + Rx_i1 * c_x1) + Rx_i2 * c_x2) + tx_i
 *       second, under HINGE only    model v1_i = c_y,i + axis_len * axis_y,i;  world w1_i = w0_i + axis_len * u_i,
 *                u_i = (Rx_i0 * axis_x0 + Rx_i1 * axis_x1) + Rx_i2 * axis_x2
 *     The try is POSSIBLE iff the model points of the list hold three that span a plane by the rigid-body section's rule,
 *     |u x v| >= 0.1 |u| |v| (the host tabulates this as a 256-bit mask per directed joint, indexed by the present subset, as it
 *     does per body for stage 1).  The fit is stage 1's, operation for operation, over the list in its order, c = k + 1 or k + 2:
 *     the centroids, S, Horn's matrix, the Jacobi sweep, the top eigenvector, R, t, and rms over all c points.
 *     The try SUCCEEDS iff it is possible, w, x, y, z are finite and rms <= max_rms (a NaN fails).  Then quat_j = (w, x, y, z) as
 *     computed, Rm_j = R, t_j = t, rms_j = rms.
 *   After the last round a body still at hops = -1 keeps its input flag in flag_j, via = -1, and NaN in quat_j, Rm_j, t_j, rms_j.
 *   Sign continuity.  quat_j goes through stage 1's walk over the frames whose flag_j is POSED or JOINTED, in ascending f; the
 *     "computed" quaternion of a POSED frame is the input's.  (A POSED frame's quat_j may so be the negative of its quat.)
 * flag_j with JOINTED read as POSED, Rm_j and t_j are tables mocap_fill_rows, mocap_find_joints and mocap_joint_series accept
 * unchanged; quat_j and t_j are tables mocap_smooth_rotations and mocap_smooth_tracks accept.
 * One launch per round, one lane per (body, frame), frames along the lanes; the sign walk is stage 1's kernels.  The "_dev" form
 * enqueues on the context's stream (every pointer but the bodies and the joints device-accessible; no output may overlap an
 * input) and does not wait; the host form uploads, runs and downloads.
 * Out of scope: a global least-squares fit of the whole skeleton (all joints closed at once); joint limits; a pose from a BALL
 * joint and one marker; two anchors in one fit; weights for the virtual points; the live loop; any change to mocap_fill_rows or
 * mocap_joint_series. */
#define MOCAP_JP_MAX_ROUNDS 16
enum {
  MOCAP_BP_JOINTED = 16  /* mocap_pose_joints' flag_j: no pose from the body's own markers, one through a joint */
};
int mocap_pose_joints(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int B, const int32_t* n_markers, const int32_t* rows,
                      const double* markers, const int32_t* flag, const double* quat, const double* Rm, const double* t_pose, int J,
                      const int32_t* body_a, const int32_t* body_b, const int32_t* kind, const double* c_a, const double* c_b,
                      const double* axis_a, const double* axis_b, double axis_len, double max_rms, int max_rounds, int32_t* flag_j,
                      int32_t* hops, int32_t* via, double* quat_j, double* Rm_j, double* t_j, double* rms_j);
int mocap_pose_joints_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_traj, int B, const int32_t* n_markers,
                          const int32_t* rows, const double* markers, const int32_t* d_flag, const double* d_quat, const double* d_Rm,
                          const double* d_t_pose, int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind,
                          const double* c_a, const double* c_b, const double* axis_a, const double* axis_b, double axis_len,
                          double max_rms, int max_rounds, int32_t* d_flag_j, int32_t* d_hops, int32_t* d_via, double* d_quat_j,
                          double* d_Rm_j, double* d_t_j, double* d_rms_j);

/* ---------------------------------------------------------------- skeleton fit (the core's own contract)
 * All joints of a frame closed at once.  After mocap_pose_joints a POSED body ignores its joints and a JOINTED body sees one
 * neighbour.  This stage fits every posed body of a frame together: the markers' residuals and, per joint, the weighted distance
 * between the joint's two images, by a fixed number of Levenberg-Marquardt steps per frame.  Offline and opt-in: with nothing
 * called nothing changes.  helpers.session_skeleton_fit is the glue.
 *
 * mocap_fit_skeleton[_dev]:
 *   traj [R][F][3], R, n_frames F, and the bodies (B, n_markers, rows, markers; HOST memory) exactly as mocap_pose_joints takes
 *     them; B in 2 .. MOCAP_BP_MAX_BODIES.
 *   flag [B][F] i32, quat [B][F][4], t_pose [B][F][3]: mocap_pose_joints' flag_j, quat_j, t_j, or mocap_pose_rows' tables.  A
 *     (body, frame) is ACTIVE iff its flag is MOCAP_BP_POSED or MOCAP_BP_JOINTED and its seven doubles are finite.
 *   The joints, HOST memory in both forms, with mocap_pose_joints' rules and refusals (one check function serves both calls).
 *   axis_len   metres, finite, > 0: how far along the axis a hinge's second virtual point lies
 *   w_joint    finite, > 0: the weight of a virtual point's squared residual against a marker's
 *   iters      1 .. MOCAP_SK_MAX_ITERS: the passes of the loop, all of them run
 *   MOCAP_E_ARG, every output untouched, for anything else or a null buffer.
 *   -> [B][F]: quat_s [4], Rm_s [9], t_s [3], rms_s;  [F]: cost0, cost f64, steps, n_act i32.
 * All arithmetic is IEEE double, no fused operation, in the order written here; / and sqrt are correctly rounded; no
 * trigonometric function.  Every byte of every output is written.  Two calls on the same input give the same bytes, and so do
 * the host form and the "_dev" form (any NaN equal to any NaN).  No floating-point atomics (the sign walk's one 32-bit integer
 * maximum in LDS, exact in any order).  Sums written "a + b + c" run left to right.
 * Tables (host).  The root of a component of the forest is its lowest body; every other body has a parent, a depth (joints to
 *   the root) and the joint to its parent.  The ELIMINATION ORDER is by (depth descending, body ascending).
 * Per frame f, with q_b, t_b the current pose of body b (at the start quat and t_pose as given, not normalised):
 *   R_b = the rigid-body section's quaternion -> R formula on q_b.  rot(R, p)_i = (R_i0 p_0 + R_i1 p_1) + R_i2 p_2.
 *   Presence is stage 1's (traj[rows[b][m]][f] is three finite values).  A joint is ACTIVE iff both its bodies are.
 *   A point of a body is (y, r, w): y its place relative to t_b in world axes, r its residual, w its weight.  In this order:
 *     the present markers in ascending m: y = rot(R_b, markers[b][m]), r_i = (y_i + t_b,i) - x_i, w = 1;
 *     then the body's active joints in ascending joint index, c, axis the joint's centre and axis in b's coordinates, and the
 *     same with ' for the body on the other side: y0 = rot(R_b, c), W0_i = y0_i + t_b,i, u = rot(R_b, axis),
 *     y1_i = y0_i + axis_len * u_i, W1_i = W0_i + axis_len * u_i; the first point is (y0, W0 - W0', w_joint), the second, under
 *     HINGE only, (y1, W1 - W1', w_joint).
 *   The body's terms, all starting at 0, per point:  S00 += w * (y1 y1 + y2 y2); S01 -= w * (y0 y1); S02 -= w * (y0 y2);
 *     S11 += w * (y0 y0 + y2 y2); S12 -= w * (y1 y2); S22 += w * (y0 y0 + y1 y1); m_i += w * y_i; s += w;
 *     g0 += w * (y1 r2 - y2 r1); g1 += w * (y2 r0 - y0 r2); g2 += w * (y0 r1 - y1 r0); g_3+i += w * r_i.
 *   The body's own block H (6 x 6 symmetric; step = (omega, tau), a point moves by omega x y + tau, J = [-[y]x, I]), its diagonal
 *     damped: H_kk = d + lam * d for d = S00, S11, S22, s, s, s; H10 = S01, H20 = S02, H21 = S12; H31 = m2, H32 = -m1, H40 = -m2,
 *     H42 = m0, H50 = m1, H51 = -m0; every other entry 0.
 *   The coupling C [child's rows][parent's columns] of an active joint between a body c and its parent p, over the joint's one or
 *     two points k with yc_k, yp_k the y above on either side: E_k,ij = [i = j] ((yc0 yp0 + yc1 yp1) + yc2 yp2) - yp_i * yc_j
 *     (off the diagonal -(yp_i * yc_j)); C_ij = -(w_joint * (E_0,ij [+ E_1,ij])) for i, j < 3; u = w_joint * (yc_0 [+ yc_1]),
 *     v = w_joint * (yp_0 [+ yp_1]); C04 = u2, C05 = -u1, C13 = -u2, C15 = u0, C23 = u1, C24 = -u0; C31 = -v2, C32 = v1, C40 = v2,
 *     C42 = -v0, C50 = -v1, C51 = v0; C33 = C44 = C55 = -(w_joint * n), n = 1 or 2; every other entry 0.
 *   Cost shares: a body's = the sum over its present markers, ascending m, of (r0 r0 + r1 r1) + r2 r2; a joint's =
 *     w_joint * e0 [+ w_joint * e1] with e_k the same expression of the joint's residuals taken from its child's side.  The
 *     frame's cost = the active bodies' shares in ascending b, then the active joints' in ascending joint index, added to 0.
 *   Solve.  Walk the elimination order; for an active body i: M = its own block, from which the complements of its active
 *     children have been subtracted in elimination order; M = L D L^T without pivoting, "point refinement"'s rule at 6 x 6:
 *     t_ik = a_ik - sum_{m<k} l_im t_km, l_ik = t_ik / d_k, d_i = a_ii - sum_{k<i} l_ik t_ik, each sum subtracted term by term in
 *     ascending index.  x = M^-1 b: u_i = b_i - sum_{k<i} l_ik u_k; x_i = u_i / d_i - sum_{k>i} l_ki x_k, ascending k, i from 5
 *     down.  z = M^-1 g.  If its parent p is active: W = M^-1 C column by column, and for the parent
 *     H_rc -= ((C_0r W_0c + C_1r W_1c) + ... + C_5r W_5c) for r >= c, g_r -= ((C_0r z_0 + C_1r z_1) + ... + C_5r z_5).
 *     Then in reverse order: delta_i = -(z_i + ((W_i0 delta_p,0 + W_i1 delta_p,1) + ...)) with an active parent, else -z_i.
 *     An inactive body contributes nothing and cuts the tree: the subtrees on either side are solved as they stand.
 *   Update (trial pose).  h = omega * 0.5; nd = sqrt(((1 + hx hx) + hy hy) + hz hz); d = (1 / nd, hx / nd, hy / nd, hz / nd);
 *     q' = d (x) q (Hamilton's product, each component summed left to right in the order d_w, d_x, d_y, d_z), divided by
 *     sqrt(((w w + x x) + y y) + z z); t' = t + tau.
 *   Levenberg-Marquardt, "point refinement"'s rule at the scale of a frame: lam = 1e-3; exactly `iters` passes: the terms and the
 *     cost at the current poses, the solve, the trial poses, the trial cost.  ACCEPT iff every pivot of every active body is
 *     finite and > 0, cost0 is finite, and the trial cost is finite and < the current cost.  On accept the trial poses become
 *     current, lam = lam / 10 and steps += 1; otherwise lam = lam * 10.  Accept and reject are selects.  A frame whose start cost
 *     is not finite, or which has no active body, is so left as it came with steps = 0.
 *   -> quat_s, t_s = the current pose; Rm_s = R of quat_s; rms_s = sqrt(share / k) over the body's k present markers at that
 *     pose, NaN with k = 0; an inactive (body, frame) gets NaN in every double.  cost0 = the cost at the start, cost = at the
 *     returned poses, steps = the accepted passes, n_act = the active joints.
 *   Sign continuity.  quat_s then goes through stage 1's walk over the frames whose input flag is POSED or JOINTED.
 * The caller keeps using its flag: with JOINTED read as POSED, Rm_s and t_s are tables mocap_fill_rows, mocap_find_joints and
 * mocap_joint_series accept unchanged; quat_s and t_s are tables mocap_smooth_rotations and mocap_smooth_tracks accept.
 * Four launches per pass (terms: one lane per (body, frame); solve: one lane per frame; trial cost; accept), the frames taken in
 * rounds of whole tiles under a fixed workspace cap -- no result depends on where a round ends.  The "_dev" form enqueues on the
 * context's stream (every pointer but the bodies and the joints device-accessible; no output may overlap an input) and does not
 * wait; the host form uploads, runs and downloads.
 * Out of scope: joint limits; a robust (Huber) cost; acceptance per component instead of per frame; a pose for a body that is
 * not active at the start (a BALL joint and one marker); body geometry or joint centres as unknowns; the live loop; any change
 * to an existing stage. */
#define MOCAP_SK_MAX_ITERS 16
int mocap_fit_skeleton(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int B, const int32_t* n_markers, const int32_t* rows,
                       const double* markers, const int32_t* flag, const double* quat, const double* t_pose, int J,
                       const int32_t* body_a, const int32_t* body_b, const int32_t* kind, const double* c_a, const double* c_b,
                       const double* axis_a, const double* axis_b, double axis_len, double w_joint, int iters, double* quat_s,
                       double* Rm_s, double* t_s, double* rms_s, double* cost0, double* cost, int32_t* steps, int32_t* n_act);
int mocap_fit_skeleton_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_traj, int B, const int32_t* n_markers,
                           const int32_t* rows, const double* markers, const int32_t* d_flag, const double* d_quat,
                           const double* d_t_pose, int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind,
                           const double* c_a, const double* c_b, const double* axis_a, const double* axis_b, double axis_len,
                           double w_joint, int iters, double* d_quat_s, double* d_Rm_s, double* d_t_s, double* d_rms_s,
                           double* d_cost0, double* d_cost, int32_t* d_steps, int32_t* d_n_act);

/* ---------------------------------------------------------------- point consolidation (the core's own contract)
 * Each blob supports at most one point.  The frame path reproduces the reference's find_point_correspondance_and_object_points,
 * in which a blob that is not the closest match of any root becomes a root of its own: one marker often comes back as two or three
 * points that share image blobs.  This stage, between the frame path (its re-submit included) and everything that reads its points,
 * compacts each frame's points to a set in which no two share a blob.  Opt-in and the core's own: with the mode off every entry
 * point writes the bytes it wrote before, and the mocap_match_triangulate* family never consolidates.
 *
 * Per frame f, over the points k in 0 .. n_out[f]) with their rows corr[f][k][0 .. C):
 *   views(k)   the number of cameras c with corr[k][c] >= 0
 *   conflict   i and j conflict iff corr[i][c] >= 0 and corr[i][c] == corr[j][c] for some camera c
 *   key(k)     (-views(k), bits(err[k]) as an unsigned 64-bit integer, k), compared lexicographically: a total order, no tolerance
 *              and no floating-point arithmetic (more views first, then the smaller error bits, then the smaller index)
 *   selection  the kept set is what this walk yields: the points in ascending key, a point kept iff it conflicts with no point
 *              kept before it.  A function of the input alone (the device computes it in rounds, in any order).  A suppressed
 *              point suppresses nothing: in a chain A-B-C with key(A) < key(B) < key(C), A and C not in conflict, A and C are
 *              kept and B is dropped.
 *   compaction the kept points move, in place, to the slots 0 .. kept count) in ascending original index; the rows of xyz, err
 *              and corr move together and n_out[f] becomes the kept count.  The slots from the new n_out up to the old one keep
 *              whatever they held.  xyz is moved, never read for a decision: the rule is the same before and after the world
 *              transform.
 * A frame is processed iff status[f] & (MOCAP_ST_ROOT_OVERFLOW | MOCAP_ST_CAND_OVERFLOW | MOCAP_ST_HIT_OVERFLOW) == 0 and
 * 0 <= n_out[f] <= K_max and every entry of its first n_out[f] rows lies in -1 .. 255.  Every other frame is left byte for byte as
 * it is.
 *
 * mocap_set_point_consolidation: MOCAP_CONSOLIDATE_OFF (0, the default) | MOCAP_CONSOLIDATE_BLOBS (1); any other value is
 * MOCAP_E_ARG and nothing changes.  The mode is honoured by every mocap_track_frame* entry point (host, images, _jpeg, and the
 * _dev forms of plain, filtered, bodies and ids): the object search and the export, the rigid bodies, the marker tracker, the
 * object filter and the epipolar-line overlay all see the consolidated points.  With the mode on K_max <= MOCAP_PC_MAX_POINTS
 * (more is MOCAP_E_LIMIT) and a _dev call with d_corr == NULL is MOCAP_E_ARG.
 *
 * mocap_consolidate_points_dev / mocap_consolidate_points: the staged call on arrays as the frame path writes them, whatever the
 * mode; C comes from mocap_set_cameras (MOCAP_E_NOCAMS without).
 *   xyz [F][K_max][3], err [F][K_max], corr [F][K_max][C], n_pts [F]   in and out (mocap_match_triangulate's xyz, err, corr, n_out)
 *   status [F]        in, may be NULL (= 0 for every frame)
 *   src [F][K_max]    out, may be NULL: the original slot of each kept point (entries from the kept count on are not written)
 *   n_in [F]          out, may be NULL: the count before consolidation, -1 = the frame was not processed
 *   K_max             1 .. MOCAP_PC_MAX_POINTS (256): below is MOCAP_E_ARG, above MOCAP_E_LIMIT with the figure in the text
 * One workgroup per frame, lane = point: one wave while K_max <= 64, 256 lanes above.  The "_dev" form
 * enqueues on the context's stream (for batches); the host form uploads, runs and downloads, every array whole.
 * Out of scope: re-triangulating a kept point from the union of its twins' blobs, a 3-D merge radius, more than 256 point slots
 * per frame. */
#define MOCAP_PC_MAX_POINTS 256
enum {
  MOCAP_CONSOLIDATE_OFF = 0,   /* the frame path's points as the reference's algorithm gives them (default) */
  MOCAP_CONSOLIDATE_BLOBS = 1  /* no two points of a frame share a blob */
};
int mocap_set_point_consolidation(mocap_ctx* ctx, int mode);
int mocap_consolidate_points(mocap_ctx* ctx, int64_t n_frames, int K_max, double* xyz, double* err, int16_t* corr, int32_t* n_pts,
                             const int32_t* status, int32_t* src, int32_t* n_in);
int mocap_consolidate_points_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, double* d_xyz, double* d_err, int16_t* d_corr,
                                 int32_t* d_n_pts, const int32_t* d_status, int32_t* d_src, int32_t* d_n_in);

/* ---------------------------------------------------------------- point refinement (the core's own contract)
 * Least-squares points with each camera's own K.  Every point of the sections above is the reference's DLT point: the null vector
 * of an algebraic system, built -- for rigs with one intrinsic matrix per camera -- with the intrinsics taken by compacted index
 * (helpers.py:296-307), so a group that skips a camera is triangulated, and scored, with the wrong K for every later view.  This
 * stage re-triangulates each kept group by minimising the true reprojection error: a fixed number of Levenberg-Marquardt steps in
 * double on the device, from the DLT point.  Opt-in and the core's own: with the mode off every entry point writes the bytes it
 * wrote before, and the mocap_match_triangulate* family never refines.
 *
 * Per point, the views are the cameras c, ascending, that see it: corr[c] >= 0 in the frame-path forms, an observation without a
 * NaN in the observation forms.  Observations (u_c, v_c) are doubles (the float32 blobs widened exactly); v = number of views.
 *   camera table   P_c = K_c [R_c | t_c] with the camera's OWN K_c (any 3 x 3 matrix, skew included), built on the host once per
 *                  mocap_set_cameras:  P[i][j] = K[i][0] RT[0][j] + K[i][1] RT[1][j] + K[i][2] RT[2][j], RT = [R | t], left to right.
 *   start          the DLT point mocap_triangulate gives for the same observations (compacted-index quirk included), in camera-0
 *                  coordinates, recomputed with the device functions of that call.  xyz is WRITTEN, NEVER READ: the stage is
 *                  indifferent to whether a world transform is set.
 *   evaluation     at X = (X, Y, Z), per view:  a = P00 X + P01 Y + P02 Z + P03, b and w likewise from rows 1 and 2, each summed
 *                  left to right.  VALID iff every w is finite and > 0.  pu = a / w, pv = b / w, ru = pu - u_c, rv = pv - v_c;
 *                  cost = 0, then per view cost = cost + ru ru, cost = cost + rv rv.
 *   normal eq.     per view  Ju[k] = (P0k - pu P2k) / w,  Jv[k] = (P1k - pv P2k) / w,  k < 3.  The six entries of H (00 01 02 11 12 22)
 *                  and the three of g start at 0 and take, per view,  H_ij = H_ij + Ju[i] Ju[j],  H_ij = H_ij + Jv[i] Jv[j],  then
 *                  g_k = g_k + Ju[k] ru,  g_k = g_k + Jv[k] rv.
 *   one step       d0 = H00 + lam H00, a11 = H11 + lam H11, a22 = H22 + lam H22 (the off-diagonal entries are H's);
 *                  L D L^T without pivoting:  l10 = H01 / d0, l20 = H02 / d0, d1 = a11 - l10 H01, t21 = H12 - l20 H01, l21 = t21 / d1,
 *                  d2 = (a22 - l20 H02) - l21 t21;   z0 = -g0, z1 = -g1 - l10 z0, z2 = (-g2 - l20 z0) - l21 z1;   y_i = z_i / d_i;
 *                  e2 = y2, e1 = y1 - l21 e2, e0 = (y0 - l10 e1) - l20 e2;   trial = X + e per component.
 *                  ACCEPTED iff d0, d1, d2 are finite and > 0, the evaluation at the trial is valid and cost_trial < cost (strict).
 *                  Accepted: X = trial (cost, H, g those of the trial), lam = lam / 10.  Otherwise X stays, lam = lam * 10.
 *   iteration      lam = 1e-3, then exactly `iters` steps, no early exit.
 *   result         xyz = the last accepted X (the start when no step was accepted); err = cost / (2 v), px^2, plain double, no
 *                  float32 rounding: the frame path's quantity with the right matrices.  In the frame-path forms the point leaves
 *                  through the frame path's own store, so the world transform applies when one is set.
 * All arithmetic is IEEE double, no fused operation, `/` IEEE division, in the order written.
 *
 * A point is left UNTOUCHED -- xyz and err byte for byte -- and says why in info, when
 *   MOCAP_RF_FEW_VIEWS   it has fewer than 2 views;
 *   MOCAP_RF_BAD_INDEX   a corr entry >= 0 is >= counts[f][c] or >= M_max (that blob is not read);
 *   MOCAP_RF_BAD_OBS     an observation (of an entry with a good index) has a coordinate that is not finite;
 *   MOCAP_RF_BAD_START   none of the above, and the start is not finite or its evaluation is not valid.
 * The first three are found in one pass over the row and may come together.  In the observation forms xyz and err are outputs
 * only: an untouched row is NaN there (fewer than 2 views: as in mocap_triangulate).
 * A FRAME is left byte for byte when status[f] & (MOCAP_ST_ROOT_OVERFLOW | MOCAP_ST_CAND_OVERFLOW | MOCAP_ST_HIT_OVERFLOW) or when
 * n_pts[f] lies outside 0 .. K_max (the consolidation's rule); slots >= n_pts[f] are never written.  corr, n_pts and status are
 * never changed.
 *   info [F][K_max] i32, may be NULL: 0 = the slot is beyond n_pts[f] or the frame was skipped; otherwise MOCAP_RF_REFINED with
 *   the number of accepted steps in bits 8-15 (info >> MOCAP_RF_STEPS_SHIFT), or the reasons above.
 *
 * mocap_set_point_refinement: iters = 0 is off (the default), 1 .. MOCAP_REFINE_MAX_ITERS is on; anything else is MOCAP_E_ARG and
 * nothing changes.  Four steps reach the converged optimum to 2e-8 relative on this project's rigs.  The mode is honoured by every
 * mocap_track_frame* entry point (host, images, _jpeg, and the _dev forms of plain, filtered, bodies, ids and bodies_tracked): one
 * more kernel behind the re-submit and BEFORE the consolidation, so the consolidation's key, the object search and the export, the
 * rigid bodies, the trackers, the object filter and the epipolar-line overlay all see refined points and refined errors.  With the
 * mode on a _dev call with d_corr == NULL is MOCAP_E_ARG.
 *
 * mocap_refine_points_dev / mocap_refine_points: the staged call on arrays as the frame path writes them (blobs, counts in;
 * mocap_match_triangulate's xyz, err in and out; corr, n_out, status in), whatever the mode; iters 1 .. 16, any K_max >= 1;
 * MOCAP_E_NOCAMS without cameras.  mocap_triangulate_refined / _dev: the same refinement for explicit correspondences, obs
 * [N][C][2] with NaN for unseen as mocap_triangulate takes them; xyz [N][3], err [N] (may be NULL), info [N] (may be NULL); the
 * world transform does not apply, as in mocap_triangulate.  One lane per point; the "_dev" forms enqueue on the context's stream.
 * Out of scope: a robust cost, lens distortion in the model, changing which group wins a root (the search selects by the
 * reference's err), re-triangulating from the union of consolidated twins' blobs. */
#define MOCAP_REFINE_MAX_ITERS 16
enum {
  MOCAP_RF_REFINED = 1,     /* the point was refined: xyz and err are the stage's */
  MOCAP_RF_FEW_VIEWS = 2,   /* untouched: fewer than 2 views */
  MOCAP_RF_BAD_INDEX = 4,   /* untouched: a corr entry beyond counts[f][c] or M_max */
  MOCAP_RF_BAD_OBS = 8,     /* untouched: an observation that is not finite */
  MOCAP_RF_BAD_START = 16   /* untouched: the DLT start is not finite or lies behind a camera */
};
#define MOCAP_RF_STEPS_SHIFT 8
int mocap_set_point_refinement(mocap_ctx* ctx, int iters);
int mocap_refine_points(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts, int K_max, int iters,
                        double* xyz, double* err, const int16_t* corr, const int32_t* n_pts, const int32_t* status, int32_t* info);
int mocap_refine_points_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs, const int32_t* d_counts, int K_max,
                            int iters, double* d_xyz, double* d_err, const int16_t* d_corr, const int32_t* d_n_pts,
                            const int32_t* d_status, int32_t* d_info);
int mocap_triangulate_refined(mocap_ctx* ctx, int64_t N, const double* obs, int iters, double* xyz, double* err, int32_t* info);
int mocap_triangulate_refined_dev(mocap_ctx* ctx, int64_t N, const double* d_obs, int iters, double* d_xyz, double* d_err,
                                  int32_t* d_info);

/* ---------------------------------------------------------------- object filter
 * `filtered_objects` of the live loop (helpers.py:109, self.kalman_filter.predict_location(objects)): per drone index a
 * cv.KalmanFilter(9, 6) in float32 (constant acceleration, measurement = position and finite-difference velocity, nearest
 * candidate to the prediction wins) whose PREDICTED state is reported, the velocity and the chosen object's heading passed
 * through the reference's LowPassFilter (lfilter from a zero state over a buffer that is cut back to its newer half whenever
 * it reaches buffer_size, last sample kept).  computer_code/api/KalmanFilter.py and LowPassFilter.py, quirks included; the
 * one difference is that the time stamp is an argument instead of time.time().  The state (Kalman vectors and matrices,
 * previous positions, previous time, low-pass buffers) lives on the device, in the context.
 *
 * mocap_set_object_filter: allocates and zeroes the state (KalmanFilter.__init__).  num_objects = drone indices filtered
 * (<= 8; 0 switches the filter off); b, a [n_taps] = the low-pass coefficients, e.g. scipy.signal.butter(5, 20 / 30)
 * (n_taps <= 16); buffer_size as LowPassFilter's (2 .. 1024, reference 300); process_noise / measurement_noise = the
 * diagonals of Q and R (reference 1e-2 and 1).  Beyond the limits: MOCAP_E_LIMIT. */
int mocap_set_object_filter(mocap_ctx* ctx, int num_objects, int n_taps, const double* b, const double* a, int buffer_size,
                            double process_noise, double measurement_noise);
/* KalmanFilter.reset (KalmanFilter.py:103-108) at time `now`: the previous time becomes now - 20, every statePost and previous
 * position is zeroed; covariances and low-pass buffers are NOT cleared.  Enqueued on the context's stream. */
int mocap_reset_object_filter(mocap_ctx* ctx, double now);
/* mocap_filter_objects: predict_location for n_frames consecutive frames, in order.
 *   t [F] f64          the frames' time stamps (what time.time() returned in the reference)
 *   O_max, pos [F][O_max][3], heading [F][O_max], drone [F][O_max], n_obj [F]   exactly mocap_locate_objects*'s outputs
 *                      (n_obj > O_max counts as O_max; O_max <= 64)
 *   fpos [F][D][3] f32, fvel [F][D][3] f32, fheading [F][D] f64   "pos", "vel", "heading" of drone index d (D = num_objects)
 *   chosen [F][D] i32  index of the object the drone was associated with; -1 = the drone is not in `filtered_objects` this
 *                      frame (no object carried its index): its state is untouched and fpos / fvel / fheading are NaN
 * Cutting a session into calls of any lengths gives bit-identical outputs.  Before mocap_set_object_filter: MOCAP_E_ARG. */
int mocap_filter_objects(mocap_ctx* ctx, int64_t n_frames, const double* t, int O_max, const double* pos, const double* heading,
                         const int32_t* drone, const int32_t* n_obj, float* fpos, float* fvel, double* fheading, int32_t* chosen);
int mocap_filter_objects_dev(mocap_ctx* ctx, int64_t n_frames, const double* d_t, int O_max, const double* d_pos,
                             const double* d_heading, const int32_t* d_drone, const int32_t* d_n_obj, float* d_fpos,
                             float* d_fvel, double* d_fheading, int32_t* d_chosen);
/* mocap_track_frame / mocap_track_frame_dev with the filter behind the object search (O_max >= 1): t [F] in, the four filter
 * outputs out, everything else as there.  The host form queues the filter's two kernels directly behind the export, their
 * outputs land in the same pinned block as the rest of the payload: still one enqueue and one event wait. */
int mocap_track_frame_filtered(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts,
                               double gate_px, int K_max, int64_t G_cap, double* xyz, double* err, int16_t* corr,
                               int32_t* n_pts, int32_t* status, int O_max, double* pos, double* heading, double* oerr,
                               int32_t* drone, int32_t* n_obj, const double* t, float* fpos, float* fvel, double* fheading,
                               int32_t* chosen);
int mocap_track_frame_filtered_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs, const int32_t* d_counts,
                                   double gate_px, int K_max, int64_t G_cap, double* d_xyz, double* d_err, int16_t* d_corr,
                                   int32_t* d_n_pts, int32_t* d_status, int O_max, double* d_pos, double* d_heading,
                                   double* d_oerr, int32_t* d_drone, int32_t* d_n_obj, const double* d_t, float* d_fpos,
                                   float* d_fvel, double* d_fheading, int32_t* d_chosen);

/* ---------------------------------------------------------------- calibration tail
 * The three handlers a user runs after `calculate-camera-pose` and before flying, over a whole capture as the frame path
 * leaves it on the device (the UI's objectPoints.current, App.tsx:458,475,492):
 *   xyz [F][K_max][3], n_pts [F] (mocap_match_triangulate's n_out), status [F] (may be NULL)
 * A frame contributes when status[f] == 0 (if status is given) and 0 <= n_pts[f] <= K_max -- the "no valid slot" rule of
 * mocap_locate_objects; slots >= n_pts[f] are never read.  Results are bit-identical from run to run, between the host and
 * the _dev form, and from machine to machine: the reductions have one fixed shape that depends on F alone.
 *
 * mocap_determine_scale: `determine-scale` (index.py:290-309).  Every frame with exactly two points yields
 * d = sqrt(sum((p0 - p1)^2)), bit-exact against NumPy; result [4] = {scale_factor = actual_distance / mean(d), mean(d),
 * pairs used, frames skipped as invalid}.  The caller multiplies every pose's t by scale_factor (index.py:306-307).  No pair at
 * all: scale_factor and mean are NaN (np.mean of an empty list) and the call returns MOCAP_OK.
 *   actual_distance   the reference hard-codes 0.15
 *   pair_dist [F]     (may be NULL) d per frame, NaN where the frame yields no pair
 *   d_result          device-accessible (device or pinned host memory), written by the last kernel */
int mocap_determine_scale(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts,
                          const int32_t* status, double actual_distance, double* pair_dist, double* result);
int mocap_determine_scale_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts,
                              const int32_t* d_status, double actual_distance, double* d_pair_dist, double* d_result);
/* mocap_floor_factor: the reduction of `acquire-floor` (index.py:158-172).  factor [17] = the 4 x 4 upper-triangular R of the
 * QR factorisation of the rows [x, y, 1 | z] of every valid point (row-major, zeros below the diagonal, diagonal >= 0),
 * then the number of points.  Built by Givens rotations per lane and combined pairwise (TSQR): backward stable like the
 * reference's scipy.linalg.lstsq, where a sum of normal equations would square the condition number of [x y 1] (captures taken
 * before set-origin sit metres from the origin).  |R[3][3]| / sqrt(points) is the RMS residual of the plane. */
int mocap_floor_factor(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts,
                       const int32_t* status, double* factor);
int mocap_floor_factor_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts,
                           const int32_t* d_status, double* d_factor);
/* mocap_floor_from_factor: the rest of `acquire-floor` (index.py:172-192) from the 17 doubles above.  Host-only arithmetic,
 * ctx may be NULL (like mocap_ba_trust_region_step).  Back-substitutes the fit z = a x + b y + c, then restates the handler:
 * normal (a, b, -1), up (0, 0, 1), G, F, R = F G F^-1, R diag(1, -1, 1); to_world [16] = [[R, 0], [0, 0, 0, 1]] row-major.
 *   info [6] (may be NULL) = {a, b, c, points, RMS residual, tilt of the plane against z = const in rad}
 * Deviations from the reference, both on inputs where its answer means nothing:
 *   - fewer than 3 points, or a pivot |R_ii| <= points * eps * max |R_jj| (i, j < 3: collinear or coincident points):
 *     MOCAP_E_ARG, nothing written.  The reference returns gelsd's minimum-norm fit of the rank-deficient system.
 *   - a floor parallel to the xy-plane: `up - (up.n) n` has norm ~ 0 and the reference's F is noise divided by noise.  The
 *     matrix is written as the arithmetic gives it (NaN when the norm is exactly 0) and the call returns MOCAP_E_NOCONV
 *     ("result still written") when that norm is below 1e-8. */
int mocap_floor_from_factor(mocap_ctx* ctx, const double* factor, double* to_world, double* info);
/* mocap_world_set_origin: `set-origin` (index.py:200-207): y and z of `point` [3] swapped, to_world_out = T(-p) to_world_in.
 * Host-only arithmetic, ctx may be NULL; in and out may be the same buffer. */
int mocap_world_set_origin(mocap_ctx* ctx, const double* to_world_in, const double* point, double* to_world_out);

/* ---------------------------------------------------------------- initial poses
 * The pose-chaining loop of the `calculate-camera-pose` handler (index.py:229-270), i.e. the caller of
 * bundle_adjustment: per neighbouring camera pair cv.findFundamentalMat(FM_RANSAC, threshold, confidence)
 * on the points both cameras saw (index.py:241-246), cv.sfm.essentialFromFundamental with the intrinsics of
 * cameras 0 and 1 (index.py:247), cv.sfm.motionFromEssential (index.py:248), the cheirality vote over the four
 * candidates through triangulate_points (index.py:250-262), R = R_c R_prev, t = t_prev + R_prev t_c (:264-265).
 *   obs [N][C][2]   calibration points, NaN = unseen (the handler's `cameraPoints` payload, index.py:232)
 *   K [C][9]        intrinsics; like the reference only those of cameras 0 and 1 are read
 *   threshold, confidence, max_iters   cv.findFundamentalMat arguments (reference: 1, 0.99999, default 1000)
 *   R [C][9], t [C][3]   poses, camera 0 = (I, 0); t has the unit scale of motionFromEssential per pair
 *   info [C-1][4]   (may be NULL) per pair: correspondences, RANSAC inliers, RANSAC iterations, candidate index
 * RANSAC draws its subsets from cv::RNG((uint64)-1) exactly like cv::RANSACPointSetRegistrator and replays its
 * bookkeeping over per-model inlier counts computed on the GPU.  Fewer than 15 common points: MOCAP_E_ARG
 * (OpenCV would silently switch to LMedS). */
int mocap_initial_poses(mocap_ctx* ctx, int C, int64_t N, const double* obs, const double* K, double threshold,
                        double confidence, int max_iters, double* R, double* t, int32_t* info);
/* cv.findFundamentalMat(p1, p2, FM_RANSAC, threshold, confidence, max_iters): p1, p2 [n][2] float32 (host),
 * F [9] row-major with F[8] = 1, mask [n] (may be NULL) 1 = inlier, info [3] (may be NULL) = inliers,
 * iterations run, iteration that produced F.  The result is the best minimal 7-point model (OpenCV does not
 * refit on the inliers). */
int mocap_find_fundamental(mocap_ctx* ctx, int64_t n, const float* p1, const float* p2, double threshold,
                           double confidence, int max_iters, double* F, uint8_t* mask, int32_t* info);

/* ---------------------------------------------------------------- exchange payload (multi-GPU gather)
 * The frame path's outputs are fixed-capacity ([F][K_max] slots).  For the one exchange of a frame-sharded run
 * (final tracks -> the gathering rank over RCCL/xGMI) only the valid slots need to travel:
 * mocap_compact_tracks_dev packs them, in frame order, into records of mocap_track_record_bytes(C) bytes
 *     { xyz f64[3] | err f64 | corr i16[C] | zero pad to a multiple of 8 }
 * and writes the exclusive prefix sum of n_out: offsets[f] = first record of frame f, offsets[F] = number of
 * records (also to *d_total when given -- e.g. pinned host memory, so the host learns the payload size without
 * a separate copy).  Records beyond `capacity` are dropped (offsets still count them).  All pointers are DEVICE
 * pointers (d_total: device-accessible); enqueued on the context's stream. */
int mocap_track_record_bytes(int C);
int mocap_compact_tracks_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const int32_t* d_n_out,
                             const double* d_xyz, const double* d_err, const int16_t* d_corr,
                             int64_t* d_offsets, void* d_records, int64_t capacity, int64_t* d_total);

/* ---------------------------------------------------------------- bundle adjustment
 * Parameter vector as the reference (helpers.py:278-285):
 *   x = [f0, (f_i, rotvec_i[3], t_i[3]) for i = 1..C-1],  n = 1 + 7 (C-1); camera 0 = (I, 0).
 * The focal entries are carried but have no effect, exactly as in the reference
 * (helpers.py:267-270 writes them into a temporary copy).  Intrinsics come from
 * mocap_set_cameras (R, t given there are ignored by the BA entry points).
 *
 * mocap_ba_residuals: replaces residual_function (helpers.py:264-276) for a batch of P
 * parameter vectors: r[p][i] = mean squared reprojection error of point i re-triangulated
 * with the poses of params[p] (float64; the reference then casts to float32);
 * NaN where the point has < 2 views (the reference drops the entry).
 *   params [P][n], obs [N][C][2] (NaN unseen), r [P][N] */
int mocap_ba_residuals(mocap_ctx* ctx, int P, const double* params, int64_t N, const double* obs,
                       double* r);

/* mocap_ba_normal_eq: one linearisation at x: forward-difference Jacobian (step rule of
 * scipy.optimize._numdiff for the given residual precision: rel_step = sqrt(eps),
 * h = rel_step * sign(x) * max(1, |x|)), Cauchy loss scaling (scipy _lsq/least_squares.py
 * `cauchy`, `scale_for_robust_loss_function`), then the dense contractions on the matrix
 * cores:  JtJ [n][n] = J^T J,  Jtr [n] = J^T f,  cost = 0.5 * sum(rho(f^2)).
 *   f32_residuals != 0 reproduces the reference's float32 cast of the residuals
 *   (helpers.py:273) and the resulting float32 step size.
 *   J_out (may be NULL): [m][n] the scaled Jacobian, m = number of valid points (returned in *m_out) */
int mocap_ba_normal_eq(mocap_ctx* ctx, const double* x, int64_t N, const double* obs,
                       int f32_residuals, int use_cauchy, double* JtJ, double* Jtr, double* cost,
                       double* J_out, int64_t* m_out);

/* mocap_ba_trust_region_step: the subproblem of one iteration exactly as mocap_ba_solve solves it -- replaces
 * scipy.optimize._lsq.common.solve_lsq_trust_region (scipy _lsq/common.py:57-, called from _lsq/trf.py:495) --
 *     min 0.5 p^T JtJ p + Jtr^T p   subject to |p| <= Delta
 * stated on the normal equations (JtJ [n][n], Jtr [n] as mocap_ba_normal_eq returns them; m = rows of J, used
 * only by scipy's full-rank threshold eps*m*s_max).  *alpha_io: Levenberg-Marquardt parameter in (scipy's
 * initial_alpha; 0 = none) and out.  method 0 = what mocap_ba_solve does (exactly-zero rows/columns deflated;
 * Cholesky secular iteration when any were found, i.e. scipy's rank-deficient branch; symmetric
 * eigen-decomposition otherwise or when a pivot collapses), 1 = eigen-decomposition always, 2 = Cholesky
 * (MOCAP_E_NOCONV when a pivot collapses).  step [n] out; info [2] (may be NULL) = {method used (1|2), live
 * parameters}.  Host-only arithmetic: exported so that parity tests can compare the step itself. */
int mocap_ba_trust_region_step(mocap_ctx* ctx, int n, int64_t m, const double* JtJ, const double* Jtr,
                               double Delta, double* alpha_io, int method, double* step, int32_t* info);

/* mocap_set_ba_progress: the reference's residual_function emits the current poses to the UI on every
 * evaluation (socketio.emit("camera-pose"), helpers.py:274; App.tsx animates them).  mocap_ba_solve has no
 * per-evaluation host round trip; it calls `cb(x, n, user)` once per ACCEPTED step with the parameter vector
 * (on the calling thread of mocap_ba_solve, context lock held: do not call back into the same context).
 * NULL switches it off. */
int mocap_set_ba_progress(mocap_ctx* ctx, void (*cb)(const double* x, int n, void* user), void* user);

/* mocap_ba_profile: measurement aid (bench.py's `ba.roofline`).  `reps` linearisations at x exactly as the LM loop
 * issues them, timed with HIP events on the context's stream, then `reps` trust-region subproblems on the
 * resulting normal equations.  out [8] = {GPU microseconds per linearisation (event to event: every launch of
 * one linearisation), wall-clock microseconds per linearisation (launch + wait for the result on the host),
 * host microseconds per trust-region subproblem, kernel launches per linearisation, valid points m, padded
 * row length NP of [J | f], 1 if the one-launch kernel ran, cost at x}. */
int mocap_ba_profile(mocap_ctx* ctx, const double* x, int64_t N, const double* obs, int f32_residuals,
                     int use_cauchy, int reps, double* out);

/* mocap_ba_solve: resident Levenberg-Marquardt / trust-region loop (the algorithm of
 * scipy.optimize.least_squares(method="trf", loss="cauchy"), helpers.py:287-289, restated
 * on the normal equations).  x [n] in/out.
 *   ftol, xtol, gtol    termination tolerances (reference: ftol=1e-2, others 1e-8)
 *   max_iter            cap on LM iterations (0 = 100*n like scipy's max_nfev)
 *   f32_residuals       see above
 *   info [8]            (may be NULL) {iterations, nfev, status, cost0, cost, optimality, m, elapsed_ms}:
 *                       nfev / status / cost / optimality as scipy's OptimizeResult reports them; iterations also
 *                       counts passes whose every trial was rejected.  EXACTLY 8 doubles are written: this symbol
 *                       keeps the buffer size it was first exported with. */
int mocap_ba_solve(mocap_ctx* ctx, double* x, int64_t N, const double* obs, double ftol, double xtol,
                   double gtol, int max_iter, int f32_residuals, int use_cauchy, double* info);

/* mocap_ba_solve_ex: the same solve; `info_len` = doubles the caller's `info` holds, min(info_len,
 * MOCAP_BA_INFO_DOUBLES) are written: the 8 above, then [8] njev (= 1 + accepted steps, scipy's count), [9] number of
 * linearisations that had to be launched a second time because the kernel launched ahead of the host's decision had
 * abandoned itself (device watchdog, 2 s: the host was held up between two iterations; 0 in normal operation), [10] base
 * points handed over to a kernel that was launched ahead of them (0: every linearisation got its point by value -- a
 * rig or point count outside the launch-ahead's range, MOCAP_BA_NO_PREARM, or the chain schedule), [11] 1 when the
 * one-launch linearisation kernel ran, 0 for the chain of five launches. */
#define MOCAP_BA_INFO_DOUBLES 12
int mocap_ba_solve_ex(mocap_ctx* ctx, double* x, int64_t N, const double* obs, double ftol, double xtol,
                      double gtol, int max_iter, int f32_residuals, int use_cauchy, double* info, int info_len);

/* ---------------------------------------------------------------- joint bundle adjustment (the core's own contract)
 * The camera poses AND all 3-D points as unknowns, optionally one focal scale per camera: the true reprojection error, every camera
 * with its own K, analytic Jacobians, a Huber cost, Levenberg-Marquardt on the Schur-reduced camera system.  The entry points above
 * restate the reference's bundle_adjustment (helpers.py:244-290) with its limits: dead focal entries, a forward-difference Jacobian
 * with a float32 step, points that are never variables but re-triangulated by DLT at every evaluation -- with the intrinsics by
 * compacted index -- and a mean of squared errors per point.  Opt-in and beside them: with nothing called nothing changes.
 *
 * Cameras.  Intrinsics from mocap_set_cameras (its R, t are ignored); every K must be plain, [[fx,0,cx],[0,fy,cy],[0,0,1]].  Poses
 *   are the arguments R [C][9] (row-major), t [C][3], in and out; camera 0 is fixed and NEVER written.  2 <= C <=
 *   MOCAP_BAJ_MAX_CAMERAS.  obs [N][C][2] with NaN for unseen, as mocap_ba_solve takes them; 1 <= N <= MOCAP_BAJ_MAX_POINTS.
 * Unknowns.  Per camera c >= 1 a rotation increment w (R <- exp([w]x) R, linearised at w = 0) and t: columns 6 (c - 1) .. + 5 of
 *   the reduced system, w first.  With MOCAP_BAJ_FOCAL (C >= 3: with two cameras the scale of the focal lengths is not
 *   observable) one scale s_c per camera, camera 0 included: fx = fx0 s_c, fy = fy0 s_c, column 6 (C - 1) + c; fscale [C] in and
 *   out (without the flag it is not read and every s_c = 1).  Per point X [3].  n_c = 6 (C - 1) + (C with the flag); NP = n_c + 1
 *   rounded up to a multiple of 16 (<= 112).
 * Points.  A point TAKES PART iff it has >= 2 views (observations without a NaN), all of them finite, and a usable position: in
 *   mocap_ba_joint_solve the DLT point of its views -- dlt_accumulate / solve_point, the device functions of mocap_triangulate,
 *   on the table P_c = K_c [R_c | t_c] of each camera's OWN K at the poses as they came, P[i][j] = (K[i][0] M[0][j] + K[i][1] M[1][j])
 *   + K[i][2] M[2][j], M = [R | t] -- which must be finite and have w = ((P20 X0 + P21 X1) + P22 X2) + P23 finite and > 0 in every
 *   view; in mocap_ba_joint_normal_eq the given X row, which must be finite.  The other points are counted in info and are NaN in
 *   X_out.
 * One view of a point at X, camera (R, t, fx, fy, cx, cy), observation (u, v), huber_px = d:
 *   P_i = (R_i0 X0 + R_i1 X1) + R_i2 X2;  Y_i = P_i + t_i.  The view is USED iff Y2 is finite and > 0 (a view that is not used
 *   contributes nothing anywhere, and is counted).  xn = Y0 / Y2, yn = Y1 / Y2;  ru = (fx xn + cx) - u, rv = (fy yn + cy) - v;
 *   s2 = ru ru + rv rv, s = sqrt(s2).  Down-weighted iff d > 0 and s > d: w = d / s, rho = (2 d) s - d d; otherwise w = 1, rho = s2.
 *   IRLS: every row is scaled by sw = sqrt(w) of the linearisation point:  r = (sw ru, sw rv);
 *   du0 = sw (fx / Y2), dv1 = sw (fy / Y2), du2 = -(du0 xn), dv2 = -(dv1 yn)          (the rows of sw dr/dY: (du0, 0, du2), (0, dv1, dv2))
 *   B = dr/dX:      Bu[j] = du0 R_0j + du2 R_2j,   Bv[j] = dv1 R_1j + dv2 R_2j
 *   A = dr/d(w, t): Au = (du2 P1,  du0 P2 - du2 P0,  -(du0 P1),  du0, 0, du2),   Av = (dv2 P1 - dv1 P2,  -(dv2 P0),  dv1 P0,  0, dv1, dv2)
 *   focal column:   Au[6] = sw (fx xn), Av[6] = sw (fy yn): the derivative for the update s <- s (1 + delta), at the current fx, fy.
 * One linearisation at damping lam (Marquardt: lam times the diagonals of V and of U), per point over its used views in camera order:
 *   rho_p = sum rho;  V (00 01 02 11 12 22):  V_ij = V_ij + (Bu[i] Bu[j] + Bv[i] Bv[j]);  g_p[j] = g_p[j] + (Bu[j] ru + Bv[j] rv), from 0.
 *   V_lam = L L^T:  a_ii = V_ii + lam V_ii;  l00 = sqrt(a00), l10 = V01 / l00, l20 = V02 / l00, d1 = a11 - l10 l10, l11 = sqrt(d1),
 *   l21 = (V12 - l20 l10) / l11, d2 = (a22 - l20 l20) - l21 l21, l22 = sqrt(d2).  a00, d1, d2 finite and > 0, else the point is
 *   SINGULAR for this linearisation: its E and z are zero and it does not move (MOCAP_BAJ_ST_POINT_SINGULAR).
 *   z = L^-1 g_p:  z0 = g0 / l00, z1 = (g1 - l10 z0) / l11, z2 = ((g2 - l20 z0) - l21 z1) / l22.
 *   Per used view and parameter k of its camera:  W = (Au[k] Bu[j] + Av[k] Bv[j]), j < 3;  the column of E = L^-1 W^T by the same
 *   forward substitution.  The columns of cameras that do not see the point are zero.
 *   Per camera over the points in the tree below:  U (upper triangle of 7 x 7) = sum (Au[i] Au[j] + Av[i] Av[j]),  g_c[i] = sum (Au[i] ru
 *   + Av[i] rv);  cost = sum of rho_p over the points.
 *   sum_p E^T E and sum_p E^T z: the point's three rows [E | z] of a row-major matrix [3 N padded to a multiple of 4][NP], padding
 *   zero, through the FP64 matrix cores (v_mfma_f64_16x16x4_f64) and the fixed slice order of the Gram of mocap_ba_normal_eq.
 *   Host (plain double loops):  S = U_lam - sum E^T E with U_lam's diagonal U_ii + lam U_ii,  rhs = -g_c + sum E^T z;  S delta = rhs by
 *   a dense Cholesky (row by row, sums left to right), which fails on a pivot that is not finite or not > 0.
 * One iteration.  delta from the system at lam; per point y = z + E delta (columns ascending), L^T x = y backwards, X_trial = X - x;
 *   cameras R <- exp([delta_w]x) R (Rodrigues on the host), t <- t + delta_t, s <- s (1 + delta_s).  The trial is linearised at
 *   lam' = max(lam / 10, 1e-12), the damping it will have if it is accepted.  ACCEPTED iff S factorised, the trial cost is finite, no
 *   view of a participating point is unused, and cost_trial < cost (strict): then lam = lam' and the trial's linearisation IS the
 *   next iteration's system -- it is never computed twice.  REJECTED: lam = 10 lam, and the current point is linearised again at
 *   the new damping (E and L depend on it).  lam_0 = 1e-3.  The solve stops when an accepted step lowers the cost by <= ftol * cost,
 *   when lam > 1e12 (MOCAP_BAJ_ST_LAMBDA), or after max_iter passes (MOCAP_BAJ_ST_MAX_ITER); a pass is one trial.
 * Gauge.  The scale is free: at the end every t and X is multiplied by |t_1 in| / |t_1 out|, so a scale set by
 *   mocap_determine_scale survives.  A camera with no observation on a participating point (MOCAP_BAJ_ST_CAMERA_UNSEEN), or no
 *   participating point at all (MOCAP_BAJ_ST_NO_POINTS): the call returns 0 with R, t, fscale untouched and X_out the start.
 * One tree for U, g_c, the cost and the counters, a function of N alone (the calibration tail's): one lane per point, 256 points per
 *   workgroup, grid ceil(N / 256) x C; lane -> wave by shuffles, wave -> workgroup through LDS in wave order, one partial per
 *   workgroup into a slab; one wave per camera folds its slab.  No floating-point atomics anywhere: two calls on the same input
 *   give the same bytes.  All arithmetic is IEEE double, no fused operation.  A pass is 6 launches (linearise, Gram, Gram reduce,
 *   camera blocks, fold, back-substitution) and one host round trip, S down and delta up; a rejected trial costs a second one.
 *
 * mocap_ba_joint_normal_eq: ONE linearisation at the given poses and the given points X [N][3] (NaN rows do not take part), at
 *   damping `lambda` (finite, >= 0): S [n_c][n_c], rhs [n_c] and *cost (may be NULL) to the host.  Exported, like mocap_ba_normal_eq,
 *   so that tests can check the linearisation itself.  info (may be NULL): [5] .. [8] below; MOCAP_BAJ_ST_BAD_DEPTH when a view
 *   was not used.
 * mocap_ba_joint_solve: the loop.  X_out [N][3] (may be NULL).  info [MOCAP_BAJ_INFO] (may be NULL):
 *   [0] passes  [1] accepted steps  [2] cost at the start  [3] cost  [4] final lam  [5] participating points  [6] excluded points
 *   [7] views down-weighted in the last accepted linearisation  [8] MOCAP_BAJ_ST_* flags  [9] elapsed ms (host clock, the whole
 *   call)  [10] ms inside the passes between device events  [11] linearisations made.
 *   mocap_set_ba_progress is honoured: cb(x, n, user) once per accepted step, x in the reference's layout [f0, (f_i, rotvec_i, t_i)],
 *   n = 1 + 7 (C - 1), f = fx0 s.
 * MOCAP_E_NOCAMS without cameras.  MOCAP_E_ARG, every output untouched, for: C or N out of range; a K that is not plain; MOCAP_BAJ_FOCAL
 *   with C = 2; unknown flag bits; huber_px, ftol or lambda negative or not finite; max_iter < 1; a null obs, R, t, X, S or rhs, or a
 *   null fscale with MOCAP_BAJ_FOCAL.
 * Out of scope: lens distortion and the principal point as unknowns (they are unknowns of mocap_ba_lens_solve, "lens calibration"
 *   below), more than 16 cameras, a sparse reduced system. */
#define MOCAP_BAJ_MAX_CAMERAS 16
#define MOCAP_BAJ_MAX_POINTS 131072
#define MOCAP_BAJ_INFO 12 /* doubles */
#define MOCAP_BAJ_FOCAL 1u /* flags: one focal scale per camera is an unknown */
enum {
  MOCAP_BAJ_ST_CAMERA_UNSEEN = 1,   /* a camera has no observation on a participating point: nothing was changed */
  MOCAP_BAJ_ST_NO_POINTS = 2,       /* no point takes part: nothing was changed */
  MOCAP_BAJ_ST_SINGULAR = 4,        /* the reduced system had no Cholesky factor in some pass (that trial was rejected) */
  MOCAP_BAJ_ST_POINT_SINGULAR = 8,  /* some point's V_lambda had no Cholesky factor in some linearisation (the point did not move) */
  MOCAP_BAJ_ST_LAMBDA = 16,         /* stopped because lam > 1e12 */
  MOCAP_BAJ_ST_MAX_ITER = 32,       /* stopped after max_iter passes */
  MOCAP_BAJ_ST_BAD_DEPTH = 64       /* mocap_ba_joint_normal_eq: a view was not used (depth not finite or <= 0) */
};
int mocap_ba_joint_normal_eq(mocap_ctx* ctx, int64_t N, const double* obs, const double* R, const double* t, const double* fscale,
                             const double* X, uint32_t flags, double huber_px, double lambda, double* S, double* rhs, double* cost,
                             double* info);
int mocap_ba_joint_solve(mocap_ctx* ctx, int64_t N, const double* obs, double* R, double* t, double* fscale, double* X_out,
                         uint32_t flags, double huber_px, double ftol, int max_iter, double* info);

/* ---------------------------------------------------------------- camera resection (the core's own contract)
 * ONE camera's pose from 3-D points in the rig's frame and where that camera saw them (PnP): minimal-sample hypotheses, every
 * candidate pose scored against every row, a least-squares refinement over the inliers.  The rig's scale, frame and world transform
 * are those of the points: nothing else is touched.  The reference has no counterpart (a knocked camera means a new calibration
 * there).  Opt-in and beside everything above: with nothing called nothing changes.  Needs no mocap_set_cameras.
 *
 * Inputs.  X [N][3], obs [N][2] (pixels), 1 <= N <= MOCAP_RESECT_MAX_POINTS; a row that holds a NaN or an infinity is skipped; the
 *   VALID rows keep their order and are numbered 0 .. n-1.  K [9] row-major, plain: [[fx,0,cx],[0,fy,cy],[0,0,1]], fx, fy finite
 *   and > 0 -- the camera's own matrix, used as it is (no intrinsics-by-index here); a K with skew is refused.  A pose is R [9]
 *   row-major and t [3], x = R X + t in the camera's frame.  prior_R / prior_t: both or neither.
 * One view at the pose (R, t):  P_i = (R_i0 X0 + R_i1 X1) + R_i2 X2,  x_i = P_i + t_i;  xn = x0 / x2, yn = x1 / x2;
 *   du = (fx xn + cx) - u, dv = (fy yn + cy) - v, s2 = du du + dv dv.  INLIER iff x2 > 0 and s2 < thr2 (strict),
 *   thr2 = threshold_px threshold_px.  IEEE +, -, x, / and comparisons only: counts and masks are reproducible bit for bit.
 * Sampler.  mix(z): z += 0x9e3779b97f4a7c15; z = (z ^ (z >> 30)) 0xbf58476d1ce4e5b9; z = (z ^ (z >> 27)) 0x94d049bb133111eb;
 *   z ^ (z >> 31) (splitmix64, 64-bit wrapping).  Draw k of hypothesis h: r_k = mix(seed + (3 h + k) 0x9e3779b97f4a7c15).
 *   i0 = r0 mod n;  i1 = r1 mod (n - 1), + 1 if >= i0;  i2 = r2 mod (n - 2), + 1 if >= min(i0, i1), then + 1 if >= max(i0, i1):
 *   three distinct valid rows, a pure function of (seed, h, n).
 * Three-point solver (Grunert).  Bearings j_k = (x, y, 1) / |(x, y, 1)|, x = (u - cx) / fx, y = (v - cy) / fy.  a = |P2 - P3|,
 *   b = |P1 - P3|, c = |P1 - P2|; cos alpha = j2.j3, cos beta = j1.j3, cos gamma = j1.j2; q = (a2 - c2) / b2, p = (a2 + c2) / b2.
 *   The quartic in v = s3 / s1:
 *     A4 = (q - 1)^2 - 4 (c2 / b2) cos2 alpha
 *     A3 = 4 [q (1 - q) cos beta - (1 - p) cos alpha cos gamma + 2 (c2 / b2) cos2 alpha cos beta]
 *     A2 = 2 [q^2 - 1 + 2 q^2 cos2 beta + 2 ((b2 - c2) / b2) cos2 alpha - 4 p cos alpha cos beta cos gamma + 2 ((b2 - a2) / b2) cos2 gamma]
 *     A1 = 4 [-q (1 + q) cos beta + 2 (a2 / b2) cos2 gamma cos beta - (1 - p) cos alpha cos gamma]
 *     A0 = (1 + q)^2 - 4 (a2 / b2) cos2 gamma
 *   solved in closed form (Ferrari on the resolvent cubic m^3 + p' m^2 + (p'^2 / 4 - r') m - q'^2 / 8 of the depressed quartic, its
 *   largest real root), every real root polished by two Newton steps on the quartic.  Per root v > 0:
 *   u = [(q - 1) v^2 - 2 q cos beta v + 1 + q] / (2 (cos gamma - v cos alpha)), kept when u > 0;  s1 = b / sqrt(1 + v^2 - 2 v cos beta);
 *   camera-frame points Q1 = s1 j1, Q2 = u s1 j2, Q3 = v s1 j3;  R = T_cam T_world^T with T the orthonormal triad of a triple (e1
 *   along 1 -> 2, e3 = e1 x (1 -> 3) normalised, e2 = e3 x e1, as columns);  t = Q1 - R P1.  Up to 4 poses per hypothesis, in root
 *   order (the roots of y^2 - s y + .. before those of y^2 + s y + .., the + sqrt before the - sqrt).  No pose from a sample that is
 *   collinear or near-coincident (|e x f|^2 <= 1e-12 b2 c2, or a squared side <= 1e-18 of the longest), or whose |A4| <= 1e-14 max |A_i|.
 *   The solver calls acos, cos, cbrt, sqrt: its poses are specified by their residuals, not by their bits.
 * Hypotheses.  H = max(n_hyp, 1).  With a prior, hypothesis 0 IS the prior: one solution, no sample.  Every other hypothesis h
 *   samples with its own h.  counts[h][s] = inliers of solution s over all valid rows.
 * Winner.  Most inliers; ties go to the lower (hypothesis, solution).  Chosen on the device; the first linearisation follows on the
 *   stream without a host round trip.  Fewer than 4 valid rows: MOCAP_RESECT_TOO_FEW.  No candidate with >= min_inliers inliers:
 *   MOCAP_RESECT_NO_MODEL.  In both cases R, t come back as the prior if there is one, else NaN, and nothing is refined.
 * Refinement.  Unknowns: a left rotation increment w (R <- exp([w]x) R) and dt (t <- t + dt).  Per inlier row, with a0 = fx / x2,
 *   b1 = fy / x2, a2 = -(a0 xn), b2 = -(b1 yn)  (D = d(du, dv)/dx has the rows (a0, 0, a2), (0, b1, b2)):
 *   Ju = (a2 P1, a0 P2 - a2 P0, -(a0 P1), a0, 0, a2),  Jv = (b2 P1 - b1 P2, -(b2 P0), b1 P0, 0, b1, b2)      = [-D [R X]x | D]
 *   H_ij = Ju_i Ju_j + Jv_i Jv_j (i <= j),  g_i = Ju_i du + Jv_i dv,  cost = s2;  a row that is not an inlier of the current mask
 *   contributes zero.  Summed through the project's one tree (one lane per valid row, 256 rows per workgroup, lane -> wave by shuffles,
 *   wave -> workgroup through LDS in wave order, one partial per workgroup, one wave folds the partials): no floating-point atomics,
 *   two calls on the same input give the same bytes.  The host takes the step: (H + lam diag H) delta = -g by a dense Cholesky (row by
 *   row, sums left to right); Rodrigues with a = sin th / th, b = (1 - cos th) / th^2 (th < 1e-8: a = 1 - th^2 / 6, b = 1/2 - th^2 / 24),
 *   G = a [w]x + b [w]x^2, E = I + G, R' = E R.  lam_0 = 1e-3 per round.  A trial is ACCEPTED iff the factor exists, its cost is finite
 *   and strictly lower, and every inlier of the mask is still in front of the camera (x2 finite and > 0): lam <- max(lam / 10,
 *   1e-12); otherwise lam <- 10 lam.  STRICTLY LOWER is decided on the cost's change taken from the increment, not on two rounded
 *   sums (which agree to fifteen digits near the minimum: their comparison there is noise, and where the loop stops would be luck).
 *   Per inlier row, at the base pose:  dx_i = ((G_i0 P0 + G_i1 P1) + G_i2 P2) + dt_i;  x2' = x2 + dx2;  dxn = (dx0 - xn dx2) / x2',
 *   dyn = (dx1 - yn dx2) / x2';  ddu = fx dxn, ddv = fy dyn;  delta = ddu (2 du + ddu) + ddv (2 dv + ddv)  (= s2' - s2 exactly);
 *   summed through the same tree:  lower iff the sum is < 0.  A round ends after max_iter accepted steps, after a trial whose step has |w|_inf <= 1e-12 and
 *   |dt|_inf <= 1e-12 (1 + |t|_inf) (taken first if accepted), when lam > 1e12, or at once on an empty mask.
 * Schedule.  Round 1: mask = the classification at the winner, refine.  Round 2: mask = the classification at the refined pose,
 *   refine again.  The mask that comes back is the classification at the FINAL pose.
 * Evaluate only.  max_iter = 0 refines nothing; n_hyp = 0 (which needs a prior) searches nothing.  Both: the prior comes back bit
 *   for bit with its mask, inliers and rms -- the health check of a calibrated rig (a camera against points built without it).
 *
 * mocap_resect_camera: R [9], t [3] out; mask [N] (may be NULL) 1 = inlier at the returned pose, 0 otherwise (skipped rows too);
 *   info [MOCAP_RESECT_INFO] (may be NULL):  [0] valid rows  [1] the winner's inliers  [2] its hypothesis  [3] its solution (-1, -1: no
 *   candidate)  [4] hypotheses without a solution  [5] final inliers  [6] accepted steps  [7] linearisations  [8] rms over the final
 *   inliers at the prior pose (NaN without one)  [9] rms at the winner  [10] rms at the final pose  [11] MOCAP_RESECT_* status.
 *   rms = sqrt(sum s2 / inliers), NaN without an inlier.  min_inliers >= 4, max_iter >= 0, 0 <= n_hyp <= MOCAP_RESECT_MAX_HYP.
 * mocap_resect_camera_dev: the same with X and obs as device pointers, on the context's stream; R, t, mask, info are host pointers
 *   and valid on return.
 * mocap_resect_hypotheses: the candidate table of the same search (n_hyp >= 1), for tests and debugging: sample [H][3] input rows of
 *   each sample (-1 for the prior and for hypotheses without a sample), n_sol [H], poses [H][4][12] (R | t; NaN where there is no
 *   solution), counts [H][4].
 * MOCAP_E_ARG, every output untouched, for: N or n_hyp out of range; min_inliers < 4; max_iter < 0; a K that is not plain; a
 *   threshold that is not finite or not > 0; n_hyp = 0 without a prior; one of prior_R, prior_t without the other; a null X, obs, K,
 *   R or t (or a null output of mocap_resect_hypotheses).
 * Out of scope: a live-loop stage; re-seating from unlabelled multi-marker frames; lens distortion or intrinsics as unknowns;
 *   several cameras jointly (mocap_ba_joint_solve afterwards does that); any change to mocap_initial_poses. */
#define MOCAP_RESECT_MAX_POINTS 131072
#define MOCAP_RESECT_MAX_HYP 4096
#define MOCAP_RESECT_INFO 12 /* doubles */
enum {
  MOCAP_RESECT_OK = 0,
  MOCAP_RESECT_TOO_FEW = 1,  /* fewer than 4 valid rows */
  MOCAP_RESECT_NO_MODEL = 2  /* no candidate pose reaches min_inliers */
};
int mocap_resect_camera(mocap_ctx* ctx, int64_t N, const double* X, const double* obs, const double* K, const double* prior_R,
                        const double* prior_t, double threshold_px, int n_hyp, uint64_t seed, int min_inliers, int max_iter,
                        double* R, double* t, uint8_t* mask, double* info);
int mocap_resect_camera_dev(mocap_ctx* ctx, int64_t N, const double* d_X, const double* d_obs, const double* K,
                            const double* prior_R, const double* prior_t, double threshold_px, int n_hyp, uint64_t seed,
                            int min_inliers, int max_iter, double* R, double* t, uint8_t* mask, double* info);
int mocap_resect_hypotheses(mocap_ctx* ctx, int64_t N, const double* X, const double* obs, const double* K, const double* prior_R,
                            const double* prior_t, double threshold_px, int n_hyp, uint64_t seed, int32_t* sample, int32_t* n_sol,
                            double* poses, int32_t* counts);

/* ---------------------------------------------------------------- lens calibration (the core's own contract)
 * The joint bundle adjustment above with the full lens model: beside the poses and the points, per camera fx, fy, cx, cy, k1, k2, p1,
 * p2 can be unknowns -- intrinsic_matrix and distortion_coef of camera-params.json from the capture-points wand wave alone, where the
 * reference's author needed an OpenCV checkerboard session.  Opt-in and beside mocap_ba_joint_*: with nothing called nothing changes.
 * THE CAPTURE MUST FILL THE IMAGES (markers out to the corners of every camera's picture) and must be taken RAW, with distortion_coef
 * = 0 in mocap_set_image_params: points that cover only the middle of the pictures do not determine a lens.
 *
 * Cameras.  mocap_set_cameras is NOT needed and NOT read: the camera count C, K [C][9] (row-major, plain: [[fx,0,cx],[0,fy,cy],[0,0,1]],
 *   fx, fy finite and > 0, cx, cy finite) and dist [C][5] (OpenCV's order k1 k2 p1 p2 k3, as camera-params.json has it; finite) are
 *   arguments, in and out like the poses R [C][9], t [C][3].  Camera 0's pose is fixed and NEVER written.  k3 is part of the model and
 *   never an unknown.  2 <= C <= MOCAP_BAL_MAX_CAMERAS; obs [N][C][2] with NaN for unseen; 1 <= N <= MOCAP_BAL_MAX_POINTS (the
 *   workspace, two sets of [3 N][NP] doubles and 256 Gram slices, is 0.8 GB at N = 65 536 and NP = 224: the order of the joint
 *   bundle adjustment's at its own limits, whose buffers it shares).
 * Unknowns.  Columns 6 (c - 1) .. + 5 of camera c >= 1 as in the joint bundle adjustment.  flags select pairs of intrinsics, for EVERY
 *   camera (camera 0 included), in this order:
 *     MOCAP_BAL_FOCAL       fx, fy    each with its own scale:  f <- f (1 + delta); the column is the derivative at the current value
 *     MOCAP_BAL_CENTRE      cx, cy    additive, pixels
 *     MOCAP_BAL_RADIAL      k1, k2    additive
 *     MOCAP_BAL_TANGENTIAL  p1, p2    additive
 *   q = 2 x (flags set) <= 8 columns per camera: column 6 (C - 1) + q c + (the parameter's place among the camera's q).  Any flag
 *   needs C >= 3.  n_c = 6 (C - 1) + q C <= 218;  NP = n_c + 1 rounded up to a multiple of 16 (<= 224).  flags = 0: the joint bundle
 *   adjustment with a fixed lens in the model.
 * Points.  Participation is the joint bundle adjustment's, word for word; the DLT start is taken on P_c = K_c [R_c | t_c] of the K as it
 *   came and IGNORES the lens.
 * One view of a point at X, camera (R, t, fx, fy, cx, cy, k1, k2, p1, p2, k3), observation (u, v), huber_px = d:
 *   P_i = (R_i0 X0 + R_i1 X1) + R_i2 X2;  Y_i = P_i + t_i;  USED iff Y2 is finite and > 0.  x = Y0 / Y2, y = Y1 / Y2.
 *   The lens (OpenCV's forward model, operation by operation as mocap_core.synth.distort_pixels):
 *     r2 = x x + y y;  kr = 1 + ((k3 r2 + k2) r2 + k1) r2;
 *     xd = (x kr + ((2 p1) x) y) + p2 (r2 + (2 x) x);   yd = (y kr + p1 (r2 + (2 y) y)) + ((2 p2) x) y
 *   and its Jacobian in (x, y), which is symmetric:  dk = ((3 k3) r2 + 2 k2) r2 + k1,  dk2 = 2 dk,
 *     Jxx = (kr + (dk2 x) x) + ((2 p1) y + (6 p2) x);  Jxy = (dk2 x) y + ((2 p1) x + (2 p2) y);  Jyy = (kr + (dk2 y) y) + ((6 p1) y + (2 p2) x)
 *   ru = (fx xd + cx) - u, rv = (fy yd + cy) - v;  s2, s, the Huber weight w, rho and sw = sqrt(w) as in the joint bundle adjustment.
 *   r = (sw ru, sw rv).  gu = sw (fx / Y2), gv = sw (fy / Y2);  the rows of sw dr/dY, no longer sparse:
 *     du0 = gu Jxx, du1 = gu Jxy, du2 = -(du0 x + du1 y);     dv0 = gv Jxy, dv1 = gv Jyy, dv2 = -(dv0 x + dv1 y)
 *   B = dr/dX:      Bu[j] = (du0 R_0j + du1 R_1j) + du2 R_2j,   Bv[j] likewise from dv
 *   A = dr/d(w, t): Au = (du2 P1 - du1 P2,  du0 P2 - du2 P0,  du1 P0 - du0 P1,  du0, du1, du2),   Av likewise from dv
 *   intrinsics, sfx = sw fx, sfy = sw fy, xr = x r2, yr = y r2, xy2 = (2 x) y   (Au, Av):
 *     fx (sfx xd, 0)   fy (0, sfy yd)   cx (sw, 0)   cy (0, sw)   k1 (sfx xr, sfy yr)   k2 (sfx (xr r2), sfy (yr r2))
 *     p1 (sfx xy2, sfy (r2 + (2 y) y))   p2 (sfx (r2 + (2 x) x), sfy xy2)
 *   A camera's 14 parameters in this order: w 3, t 3, fx, fy, cx, cy, k1, k2, p1, p2.
 * One linearisation, one iteration, the Marquardt rule, the trial linearised at lam' = max(lam / 10, 1e-12), ACCEPTED / REJECTED,
 *   lam_0 = 1e-3, the stops, the gauge and the statuses: the joint bundle adjustment's, with 14 parameters per
 *   camera where it has 7.  Additions:  a trial in which any fx or fy would not be > 0 is REJECTED before it is linearised;  the
 *   updates are f <- f (1 + delta), every other intrinsic p <- p + delta;  on return K and dist hold the current values of what was an
 *   unknown, every other entry (k3 always) is not written.  mocap_set_ba_progress is not honoured.
 *   The gauge multiplies every t and X by |t_1 in| / |t_1 out|: |t_1| comes back as it came to a few ulp (a norm of three rounded
 *   products), camera 0's pose bit for bit.  With MOCAP_BAL_ST_CAMERA_UNSEEN or MOCAP_BAL_ST_NO_POINTS the call returns 0 with R, t,
 *   K and dist untouched; X_out IS written: the start (the DLT points of the points that take part, NaN for the others).
 * Sums.  sum E^T E and sum E^T z through the Gram of mocap_ba_normal_eq as in the joint bundle adjustment (NP up to 224).  A camera's
 *   block U (upper triangle of 14 x 14) and g_c are 119 sums: the triangle is cut into four ROW BANDS, rows 0-1, 2-4, 5-8 and 9-13 (the
 *   last also carries the cost and the counters), grid ceil(N / 256) x C x 4, every band recomputing the view; each band goes
 *   through the project's one tree (one lane per point, lane -> wave by shuffles, wave -> workgroup through LDS in wave order, one
 *   partial per workgroup, one wave per camera and band folds the slab): the order of every sum is a function of N alone.  No
 *   floating-point atomics anywhere: two calls on the same input give the same bytes.  All arithmetic is IEEE double, no fused
 *   operation.  A pass is 6 launches and one host round trip, as in the joint bundle adjustment.
 *
 * mocap_ba_lens_normal_eq: ONE linearisation at the given cameras and the given points X [N][3] (NaN rows do not take part), at
 *   damping `lambda`: S [n_c][n_c], rhs [n_c], *cost (may be NULL), info (may be NULL) as mocap_ba_joint_normal_eq fills them.
 * mocap_ba_lens_solve: the loop.  X_out [N][3] (may be NULL).  info [MOCAP_BAL_INFO] (may be NULL): the layout of mocap_ba_joint_solve,
 *   [8] MOCAP_BAL_ST_* (the values of MOCAP_BAJ_ST_*).
 * MOCAP_E_ARG, every output untouched, for: C or N out of range; a K that is not plain or whose fx, fy are not finite and > 0; a
 *   cx, cy or distortion coefficient that is not finite; any flag with C = 2; unknown flag bits; huber_px, ftol or lambda negative or
 *   not finite; max_iter < 1; a null obs, R, t, K, dist, X, S or rhs.
 *
 * mocap_undistort_points: raw pixels in [N][C][2] -> ideal pinhole pixels out [N][C][2] under K [C][9], dist [C][5] (checked as
 *   above; 1 <= C <= MOCAP_BAL_MAX_CAMERAS, 1 <= N <= MOCAP_UNDISTORT_MAX_POINTS), one lane per observation: the same raw capture feeds
 *   mocap_determine_scale, mocap_acquire_floor, mocap_ba_joint_solve and mocap_resect_camera once the lenses are known.
 *   x0 = (u - cx) / fx, y0 = (v - cy) / fy;  from (x, y) = (x0, y0), MOCAP_UNDISTORT_NEWTON times:  the lens and its Jacobian at
 *   (x, y);  ex = xd - x0, ey = yd - y0;  det = Jxx Jyy - Jxy Jxy;  x <- x - (Jyy ex - Jxy ey) / det,  y <- y - (Jxx ey - Jxy ex) / det
 *   (both from the old x, y).  out = (fx x + cx, fy y + cy).  A NaN in either coordinate gives NaN in both; a camera whose five
 *   coefficients are all zero has its pixels copied bit for bit.  in and out may be the same buffer.
 * mocap_undistort_points_dev: the same with in and out as device pointers, on the context's stream; K and dist are host pointers.
 * Out of scope: k3 and higher-order terms as unknowns, a known-length wand constraint, priors on the intrinsics, skew, more than 16
 *   cameras, fusing the launches. */
#define MOCAP_BAL_MAX_CAMERAS 16
#define MOCAP_BAL_MAX_POINTS 65536
#define MOCAP_BAL_INFO 12 /* doubles */
#define MOCAP_UNDISTORT_MAX_POINTS 1048576
#define MOCAP_UNDISTORT_NEWTON 8
#define MOCAP_BAL_FOCAL 1u      /* flags: fx, fy of every camera are unknowns */
#define MOCAP_BAL_CENTRE 2u     /* ... cx, cy */
#define MOCAP_BAL_RADIAL 4u     /* ... k1, k2 */
#define MOCAP_BAL_TANGENTIAL 8u /* ... p1, p2 */
enum {
  MOCAP_BAL_ST_CAMERA_UNSEEN = 1,   /* a camera has no observation on a participating point: nothing was changed */
  MOCAP_BAL_ST_NO_POINTS = 2,       /* no point takes part: nothing was changed */
  MOCAP_BAL_ST_SINGULAR = 4,        /* the reduced system had no Cholesky factor in some pass (that trial was rejected) */
  MOCAP_BAL_ST_POINT_SINGULAR = 8,  /* some point's V_lambda had no Cholesky factor in some linearisation (the point did not move) */
  MOCAP_BAL_ST_LAMBDA = 16,         /* stopped because lam > 1e12 */
  MOCAP_BAL_ST_MAX_ITER = 32,       /* stopped after max_iter passes */
  MOCAP_BAL_ST_BAD_DEPTH = 64       /* mocap_ba_lens_normal_eq: a view was not used (depth not finite or <= 0) */
};
int mocap_ba_lens_normal_eq(mocap_ctx* ctx, int C, int64_t N, const double* obs, const double* R, const double* t, const double* K,
                            const double* dist, const double* X, uint32_t flags, double huber_px, double lambda, double* S,
                            double* rhs, double* cost, double* info);
int mocap_ba_lens_solve(mocap_ctx* ctx, int C, int64_t N, const double* obs, double* R, double* t, double* K, double* dist,
                        double* X_out, uint32_t flags, double huber_px, double ftol, int max_iter, double* info);
int mocap_undistort_points(mocap_ctx* ctx, int C, int64_t N, const double* in, const double* K, const double* dist, double* out);
int mocap_undistort_points_dev(mocap_ctx* ctx, int C, int64_t N, const double* d_in, const double* K, const double* dist,
                               double* d_out);

/* ---------------------------------------------------------------- predicted precision (the core's own contract)
 * How well, in the caller's length unit, the rig CAN know a point.  Every quality number above is a reprojection error in px^2; this
 * stage answers in metres: with independent pixel noise of standard deviation sigma_px in every view, the triangulated point's
 * first-order covariance is sigma_px^2 H^-1, H = sum over the views of J^T J -- the normal matrix "point refinement" forms, evaluated
 * at a given point with no observation and no iteration.  Opt-in and stateless: nothing is stored in the context, no other entry
 * point changes a byte.  Three forms: named points, the points of a frame batch, and a voxel grid (the capture-volume map).
 *
 * Camera table.  P_c = K_c [R_c | t_c] of "point refinement", each camera with its own K, as built at mocap_set_cameras (MOCAP_E_NOCAMS
 *   without).
 * Caller's coordinates.  `frame`: 12 doubles, the row-major 3 x 4 matrix [A | a], or NULL for the identity: camera-0 coordinates are
 *   X = A x + a for the caller's x.  The host folds it into a per-call table  P'_c = P_c [[A, a], [0, 1]]:
 *     P'[r][j] = (P[r][0] A[0][j] + P[r][1] A[1][j]) + P[r][2] A[2][j]  (j < 3),
 *     P'[r][3] = ((P[r][0] a[0] + P[r][1] a[1]) + P[r][2] a[2]) + P[r][3];      frame == NULL: P' = P byte for byte.
 *   The kernels see P' and x alone: every result is in the caller's coordinates and no inverse of A is taken anywhere.  Every entry
 *   of frame must be finite.
 * One view at x = (X, Y, Z), camera table row P = P'_c (the expressions of "point refinement"):
 *     a = P00 X + P01 Y + P02 Z + P03, b and w likewise from rows 1 and 2, each summed left to right;  pu = a / w, pv = b / w;
 *     Ju[k] = (P0k - pu P2k) / w,  Jv[k] = (P1k - pv P2k) / w,  k < 3   (eight divisions per view).
 *   The six entries of H (00 01 02 11 12 22) start at 0 and take, per view in ascending camera order,  H_ij = H_ij + Ju[i] Ju[j],  then
 *   H_ij = H_ij + Jv[i] Jv[j].  There is no observation: no residual, no g, no cost.
 * Which cameras are views.
 *     named        bit c of seen[i] (uint64), c < C; higher bits are ignored.
 *     frame path   corr[f][k][c] >= 0; the index itself is not read.
 *     visibility   (seen == NULL, and always in the map)  camera c is a view iff  w is finite and w > 0,  w >= near and w <= far,
 *                  0 <= pu and pu < width,  0 <= pv and pv < height -- comparisons of doubles (width, height converted), a NaN fails.
 *                  near >= 0 and finite, far > near (far may be +inf), width, height >= 1;  read only in this form.
 *   n_views = the number of views;  a named or frame-path view whose w is not finite or <= 0 still counts and sets MOCAP_PM_BAD_VIEW.
 * Decomposition.  A = H as a full symmetric 3 x 3, V = identity; cyclic Jacobi by the rule "body trajectories" item 1 spells out
 *   for Horn's matrix, with the index running 0 .. 2: at most MOCAP_PM_SWEEPS sweeps; a sweep begins with
 *   off = (|A01| + |A02|) + |A12| and ends the iteration when off == 0; the pairs in the order 01, 02, 12; the skip rule, the g rule
 *   from the fifth sweep, theta, t, cs, sn and the updates of A and V word for word.  lam = (A00, A11, A22) is then sorted ascending by
 *   the network  (0,1) (1,2) (0,1):  a step (i, j) swaps lam_i, lam_j and columns i, j of V iff lam_i > lam_j.
 * Outputs, per point / slot / voxel:
 *     info      MOCAP_PM_OK, or the reasons below (0 only for a slot that holds no point)
 *     n_views
 *     sig[3]    ascending: sigma_px / sqrt(lam_2), sigma_px / sqrt(lam_1), sigma_px / sqrt(lam_0): the principal standard deviations
 *     axis[3]   column 0 of V (the direction of sig[2]) as the iteration left it, not renormalised; negated when its component of
 *               largest magnitude (the first among equals) is negative
 *     cov[6]    packed like H:  s2 = sigma_px sigma_px, d_k = s2 / lam_k,
 *               cov_ij = ((V_i0 V_j0) d_0 + (V_i1 V_j1) d_1) + (V_i2 V_j2) d_2
 *   When info is not MOCAP_PM_OK every double is a quiet NaN.  Reasons (the first three are found in the one pass over the cameras and
 *   may come together; DEGENERATE comes alone, the decomposition is made only without them):
 *     MOCAP_PM_BAD_POINT    a coordinate of x is not finite
 *     MOCAP_PM_BAD_VIEW     a named or frame-path view whose w is not finite or <= 0
 *     MOCAP_PM_FEW_VIEWS    fewer than 2 views
 *     MOCAP_PM_DEGENERATE   an eigenvalue that is not finite, or lam_0 <= lam_2 * 2^-40 (a point on the baseline of its only two
 *                           cameras; a point at 1e200)
 * All arithmetic is IEEE double, nothing fused, `/` and sqrt IEEE, in the order written.  Every output byte is written; the host form,
 * the _dev form, a second call and a second stream give the same bits; no floating-point atomics.  The _dev forms enqueue on the
 * context's stream and do not wait (frame, origin and e0 .. e2 are HOST pointers in both forms, read before the call returns).
 *
 * mocap_point_precision / _dev: N points xyz [N][3] (1 <= N <= MOCAP_PM_MAX_POINTS), seen [N] uint64 or NULL (by visibility; width,
 *   height, near, far are read only then) -> cov [N][6] (may be NULL), sig [N][3], axis [N][3] (may be NULL), n_views [N] i32,
 *   info [N] i32.
 * mocap_frame_precision / _dev: xyz [F][K_max][3], corr [F][K_max][C], n_pts [F], status [F] (may be NULL) exactly as the frame path
 *   wrote them (with a world transform set, pass its inverse as `frame`) -> the same outputs per slot [F][K_max].  The refinement's
 *   skip rule: a frame with status & (MOCAP_ST_ROOT_OVERFLOW | MOCAP_ST_CAND_OVERFLOW | MOCAP_ST_HIT_OVERFLOW) or n_pts outside
 *   0 .. K_max, and every slot >= n_pts[f], gets info = 0, n_views = 0 and NaN.  n_frames >= 0, K_max >= 1,
 *   n_frames K_max <= MOCAP_PM_MAX_POINTS; n_frames == 0 returns 0 and touches nothing.
 * mocap_coverage_map / _dev: voxel (i, j, k), i < nx fastest, sits at  x_d = ((origin_d + i e0_d) + j e1_d) + k e2_d  per component
 *   (i, j, k converted to double); 1 <= nx, ny, nz <= MOCAP_PM_MAX_DIM, nx ny nz <= MOCAP_PM_MAX_VOXELS; views by visibility.
 *     n_views [nz][ny][nx] u8    the visibility count, whatever the info
 *     sig_max [nz][ny][nx] f32   sig[2] rounded to the nearest float32; NaN unless info is OK
 *     seen    [nz][ny][nx] u64   the views' bits; may be NULL
 *     summary [MOCAP_PM_SUMMARY] i64:  [0 .. 64] the number of voxels seen by exactly v cameras;  [65] the number of GOOD voxels -- OK,
 *       n_views >= min_views and the double sig[2] <= max_sigma (min_views >= 0; max_sigma may be +inf, not NaN);  [66 .. 71] imin, imax,
 *       jmin, jmax, kmin, kmax over the GOOD voxels, with none: every min the dimension, every max -1.  Integers only (per-workgroup
 *       reduction, then integer atomics): independent of any order.
 * mocap_precision_limits: MOCAP_PM_MAX_POINTS, MOCAP_PM_MAX_VOXELS, MOCAP_PM_SUMMARY (any pointer may be NULL).
 * MOCAP_E_ARG, every output untouched, for: sigma_px not finite or <= 0; a frame entry that is not finite; N, n_frames, K_max, nx, ny,
 *   nz or their product out of range; width, height, near, far against the rule above where they are read; min_views < 0; max_sigma
 *   NaN; a null required buffer.
 * Out of scope: lens distortion in the visibility test or the Jacobian, occlusion, per-blob pixel noise, the covariance of the
 *   calibration itself, using the covariances as weights in the later stages. */
#define MOCAP_PM_MAX_POINTS 16777216
#define MOCAP_PM_MAX_VOXELS 134217728
#define MOCAP_PM_MAX_DIM 1024
#define MOCAP_PM_SUMMARY 72 /* int64 */
#define MOCAP_PM_SWEEPS 16
enum {
  MOCAP_PM_OK = 1,          /* sig, axis and cov are the stage's */
  MOCAP_PM_BAD_POINT = 2,   /* NaN: a coordinate that is not finite */
  MOCAP_PM_BAD_VIEW = 4,    /* NaN: a named or frame-path view with a depth that is not finite or <= 0 */
  MOCAP_PM_FEW_VIEWS = 8,   /* NaN: fewer than 2 views */
  MOCAP_PM_DEGENERATE = 16  /* NaN: H has no usable inverse */
};
void mocap_precision_limits(int* max_points, int64_t* max_voxels, int* summary_len);
int mocap_point_precision(mocap_ctx* ctx, int64_t N, const double* xyz, const uint64_t* seen, int width, int height, double near,
                          double far, double sigma_px, const double* frame, double* cov, double* sig, double* axis, int32_t* n_views,
                          int32_t* info);
int mocap_point_precision_dev(mocap_ctx* ctx, int64_t N, const double* d_xyz, const uint64_t* d_seen, int width, int height, double near,
                              double far, double sigma_px, const double* frame, double* d_cov, double* d_sig, double* d_axis,
                              int32_t* d_n_views, int32_t* d_info);
int mocap_frame_precision(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int16_t* corr, const int32_t* n_pts,
                          const int32_t* status, double sigma_px, const double* frame, double* cov, double* sig, double* axis,
                          int32_t* n_views, int32_t* info);
int mocap_frame_precision_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int16_t* d_corr,
                              const int32_t* d_n_pts, const int32_t* d_status, double sigma_px, const double* frame, double* d_cov,
                              double* d_sig, double* d_axis, int32_t* d_n_views, int32_t* d_info);
int mocap_coverage_map(mocap_ctx* ctx, int nx, int ny, int nz, const double* origin, const double* e0, const double* e1,
                       const double* e2, int width, int height, double near, double far, double sigma_px, const double* frame,
                       int min_views, double max_sigma, uint8_t* n_views, float* sig_max, uint64_t* seen, int64_t* summary);
int mocap_coverage_map_dev(mocap_ctx* ctx, int nx, int ny, int nz, const double* origin, const double* e0, const double* e1,
                           const double* e2, int width, int height, double near, double far, double sigma_px, const double* frame,
                           int min_views, double max_sigma, uint8_t* d_n_views, float* d_sig_max, uint64_t* d_seen, int64_t* d_summary);

#ifdef __cplusplus
}
#endif
#endif /* MOCAP_CORE_H */
