// ctx.hpp -- the opaque context behind `mocap_ctx*` (include/mocap_core.h).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "io_fields.hpp"
#include "kernels.hpp"

#define HIP_TRY(ctx, expr)                                     \
  do {                                                         \
    hipError_t e__ = (expr);                                   \
    if (e__ != hipSuccess) return (ctx)->hip_fail(e__, #expr); \
  } while (0)

// device memory, pinned host memory and events belong to the context member that holds them (freed with it, never copied)
struct Owned {
  Owned() = default;
  Owned(const Owned&) = delete;
};

struct DevBuf : Owned {
  void* ptr = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes);  // grow-only; 0 on success
  ~DevBuf() { if (ptr) (void)hipFree(ptr); }
};

struct PinBuf : Owned {  // hipHostMalloc
  void* ptr = nullptr;
  size_t cap = 0;
  // grow-only: more than `cap` bytes needed = the buffer is replaced by one of `want` bytes (the growth rule is the caller's)
  hipError_t reserve(size_t need, size_t want, unsigned flags);
  ~PinBuf() { if (ptr) (void)hipHostFree(ptr); }
};

struct Event : Owned {
  hipEvent_t ev = nullptr;
  hipError_t ready() { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }  // created by its first user
  ~Event() { if (ev) (void)hipEventDestroy(ev); }
};

struct mocap_ctx {
  int device = 0;
  int num_cus = 256;
  int frame_threads = 0;    // workgroup size of the frame kernel, 0 = automatic (MOCAP_FRAME_THREADS=64|128|256)
  int heavy_threshold = -1; // -1 = automatic; 0 = never split heavy frames (MOCAP_HEAVY_THRESHOLD)
  int slice_size = 0;       // 0 = automatic (MOCAP_SLICE_SIZE)
  int hit_cap = 32;         // wide frames: hits kept per (root, camera) (mocap_set_frame_limits)
  int force_wide = 0;       // route every frame batch through the wide (HBM workspace) variant
  int32_t frame_gen = 0;    // generation of the last frame-path launch (tags the slices it publishes)
  int frame_q_cap[2] = {0, 0};  // W_cap the work-queue buffer was laid out for ([0] a batch's own pass, [1] the re-submit's second pass:
                            // two buffers, so that neither pass finds the other's layout and clears the queue again -- six fills per call)
  const char* last_frame_kernel = "none";  // which kernel the last frame batch went to (mocap_last_frame_kernel)
  bool frame_q_clean[2] = {false, false};  // the queue counters were left at zero by the one-launch schedule
  void frame_q_dirty() { frame_q_clean[0] = frame_q_clean[1] = false; }
  int frame_launches = 1;   // 1: one persistent launch per batch (MODE_ALL); 3: main / slice / merge launches
  int prune = 1;            // stop a candidate group's reprojection once it cannot beat its root's best (exact)
  int exhaustive = 0;       // MOCAP_OPT_EXHAUSTIVE_WALK: no branch and bound, no cut-offs (verification mode)
  int eval_bb = 1;          // branch-and-bound selection (csrc/frame_bb.hip) wherever it applies; 0: always the exhaustive walk
  int bb_pl = 16;           // ... candidates per block: a root stops opening digits here at the latest (MOCAP_BB_PL: at least this many, as before round 10)
  int bb_pl_min = 16;       // ... a root opens digits while its blocks hold fewer candidates than this,
  int bb_nb_max = 1;        // ... or fewer than bb_pl while it still has more blocks than this (frame_bb.hip, phase C).  16 / 1 = one size for
                            // every root: every finer setting of the round-10 sweep was slower (profiles/r10_block_size_ab.txt)
  int bb_min_g = 0;         // ... frames with fewer candidates queue every block untested (swept: 0-512 equal, 2048 +13 %)
  int bb_flush = 0;         // ... queued candidates that trigger their evaluation (0 = one per lane)
  int eigcut = 1;           // ... and drop it before the null vector / the reprojection on an eigenvalue bound (EigCut)
  double eig_c0[3] = {0, 0, 0};  // ... origin for the branch-and-bound's bounds: the point closest to all optical axes
  double p3max2c = 0.0;     // ... and the constant in that frame
  double p3max2 = 0.0;      // EigCut constant of the current camera set (0: intrinsics not of the form the bound needs)
  hipStream_t own_stream = nullptr, stream = nullptr;
  // stream hand-over (mocap_set_stream): every "_dev" entry point records this event behind what it enqueued; a new
  // stream is ordered behind it with hipStreamWaitEvent -- the previous stream's handle (the caller's: it may be gone)
  // is never touched again and the host never blocks
  Event handover_event;
  bool dev_outstanding = false;
  int mark_enqueued();
  std::mutex mu;            // one context = one serialised caller (include/mocap_core.h)
  std::string err;          // guarded by err_mu (written by a failing call, copied out by mocap_last_error)
  std::mutex err_mu;
  uint32_t flags = 1u;      // MOCAP_OPT_F32_ROUNDING on by default
  int C = 0;
  std::vector<double> hK, hR, ht, hF;  // host copies (intrinsics are reused by bundle adjustment)
  DevBuf tables;            // Pq | RT | K4 | F | K9
  const double* d_K9 = nullptr;
  const double* d_Pown = nullptr;  // [C][12]: K_c [R_c|t_c], each camera's own K (point refinement)
  mocap::CamView cv{};
  // bundle adjustment: pinned host staging (async copies that really are async) and the event the
  // LM loop spin-waits on (hipStreamSynchronize may sleep on an interrupt: +50..400 us per wait)
  PinBuf ba_pin;
  Event ba_event;
  PinBuf ba_stage;          // pinned staging of a solve's inputs (observations | valid list): no pageable copies
  void (*ba_progress)(const double* x, int n, void* user) = nullptr;  // mocap_set_ba_progress
  void* ba_progress_user = nullptr;
  DevBuf ba_fused;          // one-launch linearisation: chunk partial tiles | chunk costs | counters | (Jaug dump)
  double ba_stamp = 0.0;    // completion stamp of the last fused launch (monotonic per context)
  PinBuf live_pin;          // zero-copy staging of the live (few frames per call) host entry point
  Event live_event;
  DevBuf world;             // 16 doubles: the to-world matrix of the fused epilogue
  bool world_on = false;
  // blob extraction (mocap_set_image_params): frame geometry, undistortion maps, mask workspace
  int img_C = 0, img_rows = 0, img_cols = 0, img_S = 0, img_ay = 0;
  DevBuf img_map, img_rot, img_mask, img_stage, img_tiles, img_lens, img_fix, img_fixidx, img_act, img_box, img_zero;
  int img_n_lt = 0;           // (lens, rotation) x tiles: entries of the fix-up index
  int blob_skip_dark = 1;     // exact early-out for tiles whose source bytes span a range <= 2 (mocap_set_blob_options)
  int centroid_mode = 0;      // MOCAP_CENTROID_* (mocap_set_centroid_mode): 0 = the reference's int() polygon centroid
  DevBuf img_grey, img_bbox;  // weighted mode only: grey plane [images][S][S], slot windows [images][M_max][4] int16
  DevBuf compact_ws;        // block totals of the track-compaction scan
  DevBuf frame_ws;          // wide-frame workspace: [workgroup][hit lists | group columns | ...]
  DevBuf bb_ws;             // search kernels (csrc/frame_bb.hip): the winners' records, [num_cus * kBBMaxWgPerCu][frame_bb_ws_bytes] -- one size for the
                            // context's life, a buffer of its own: no other launch's reserve() ever frees it behind a queued search pass
  DevBuf live_stage;        // mocap_track_frame: device copy of a wide frame's blobs (narrow frames are read from pinned host memory in place)
  DevBuf resub;             // device-side re-submit: counters | frame list | gathered inputs | second-pass outputs
  DevBuf resub_ctr;         // ... its two alternating counters (never re-allocated while a call is in flight)
  DevBuf resub_q;           // ... the second pass's work queues (frame_q_cap[1])
  DevBuf heavy_recs;        // ... heavy roots exported by the second pass (csrc/heavy_bb.hip)
  DevBuf heavy_ws;          // ... the search's frontier workspace
  DevBuf heavy_enum;        // ... queue + per-workgroup winners of the roots enumerated over the whole GPU (heavy_enum_kernel)
  uint32_t resub_calls = 0; // ... parity selects the counter of the current call
  DevBuf scratch[4];        // [0] host-API staging, [1..3] bundle adjustment workspace
  // object filter (mocap_set_object_filter): num_objects == 0 = off
  int objf_D = 0, objf_B = 0;
  float objf_q = 0.f, objf_r = 0.f;
  DevBuf objf_state;        // ObjFilterState | h [B] | low-pass history [2][D][4][B] (a call reads one half and writes the other)
  DevBuf objf_ws;           // per call: samples [D][4][F] | slots [F][D][2] | samples appended [D]
  uint32_t objf_calls = 0;  // ... parity selects the half that holds the history
  // marker tracker (mocap_set_marker_tracker, csrc/marker_track_capi.hip): mt_T == 0 = off
  int mt_T = 0, mt_max_missed = 0;
  double mt_g2 = 0.0, mt_alpha = 0.0;
  DevBuf mt_state;          // MarkerTrackState: the track slots and next_id
  int consolidate = 0;      // MOCAP_CONSOLIDATE_* (mocap_set_point_consolidation): the live loop's points compacted to one per blob, off by default
  int refine_iters = 0;     // mocap_set_point_refinement: Levenberg-Marquardt steps on the live loop's points, 0 = off (the default)
  DevBuf calib_ws;          // calibration tail: one partial per workgroup (pair sums | floor factors), csrc/calib_tail.hip
  // preview-stream JPEG encoder (csrc/jpeg_capi.hip): header and divisors of the last (H, T * W, quality), workspace of a chunk
  int jpeg_key[3] = {0, 0, 0};
  mocap::JpegParams jpeg_params{};
  DevBuf jpeg_ws;           // per image of a chunk: coefficients | AC bits | bit offsets | total bits | unstuffed scan
  DevBuf jpeg_stage;        // host-buffer entry points: frames in, [F][capacity] streams, sizes and status out
  uint32_t preview_overlay = 0;  // MOCAP_OVERLAY_* bits (mocap_set_preview_overlay): drawings on the processed frames, off by default
  DevBuf overlay_stage;     // mocap_draw_epilines: pictures | blobs | counts | corr | n_pts | status
  // rigid bodies (mocap_set_rigid_bodies, csrc/rigid_body_capi.hip): rb_B == 0 = none registered
  int rb_B = 0;
  double rb_tol = 0.0, rb_max_rms = 0.0;
  long long rb_work_cap = 0;
  DevBuf rb_models;         // RigidBodyModel [rb_B]: markers, pair distances and the posability mask of every body
  // body tracker (mocap_set_body_tracker, csrc/body_track_capi.hip): bt_on == 0 = off
  int bt_on = 0, bt_max_missed = 0;
  double bt_g2 = 0.0, bt_alpha = 0.0;
  DevBuf bt_state;          // BodyTrackState: one slot per registered body
  DevBuf bt_search;         // mocap_track_bodies*: the per-frame search's outputs, which the tracker reads
  // joint bundle adjustment (csrc/ba_joint_capi.hip): two sets of (poses, points, E, L), the Gram slices and the camera slab;
  // pinned: G and the camera blocks down, the poses and delta up
  DevBuf baj_ws;
  PinBuf baj_pin;
  // camera resection (csrc/resect_capi.hip): rows, candidate table, mask and slab; pinned: the record of a linearisation, poses up
  DevBuf rs_ws;
  PinBuf rs_pin;
  // predicted precision (csrc/precision_capi.hip): the host copy of the table behind d_Pown, and the per-call table P' on the device
  std::vector<double> hPown;
  DevBuf pm_tab;

  int fail(int code, const char* fmt, ...);
  int hip_fail(hipError_t e, const char* what);
};

// Wait for everything queued on the context's stream by polling an event: a live call and the LM loop (twice per
// iteration) wait on ~0.1 ms of GPU work, and a sleeping wait (hipStreamSynchronize may sleep on an interrupt:
// +50..400 us) costs more than the work itself.
int spin_wait(mocap_ctx* ctx, Event& event);

// internal entry points shared between the translation units of the C ABI (context lock held by the caller)
int mocap_blob_stage_locked(mocap_ctx* ctx, int64_t n_frames, const uint8_t* d_images, int M_max, float* d_blobs,
                            int32_t* d_counts, int32_t* d_status, uint8_t* d_processed = nullptr, int32_t* d_n_contours = nullptr);
// JPEG encoder on device pointers (jpeg_capi.hip): arguments checked, kernels enqueued on the context's stream
int jpeg_dev_locked(mocap_ctx* ctx, const char* who, int64_t n_images, int T, int H, int W, const uint8_t* d_bgr, int quality,
                    uint8_t* d_jpeg, int64_t capacity, int64_t* d_sizes, int32_t* d_status, int64_t out_stride = 0);
// preview overlays (overlay_capi.hip): contours and centre marks over the blob stage's outputs (n_images pictures of edge S, the
// mask in ctx->img_mask), and the epipolar lines of a frame batch's points; `flags` = the bits the calling entry point read
int overlay_blobs_locked(mocap_ctx* ctx, uint32_t flags, int64_t n_images, int S, int M_max, const float* d_blobs,
                         const int32_t* d_counts, const int32_t* d_status, uint8_t* d_bgr);
int epilines_dev_locked(mocap_ctx* ctx, const char* who, int64_t n_frames, int S, uint8_t* d_bgr, int M_max, const float* d_blobs,
                        const int32_t* d_counts, int K_max, const int16_t* d_corr, const int32_t* d_n_pts, const int32_t* d_status);
// the preview stream of the chained live call (mocap_track_frame_images_jpeg)
struct JpegOut {
  int quality;
  uint8_t* jpeg;      // [F][capacity]
  int64_t capacity;
  int64_t* size;      // [F]
};
int locate_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const double* d_err,
                      const int32_t* d_n_pts, int O_max, double* d_pos, double* d_heading, double* d_oerr,
                      int32_t* d_drone, int32_t* d_lead, int32_t* d_n_obj);
// the optional stages of the live loop (io_fields.hpp); `who` names the entry point in a check's message
int filter_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int O_max, const FilterIO& io);
int filter_dev_locked(mocap_ctx* ctx, int64_t n_frames, int O_max, const double* d_pos, const double* d_heading,
                      const int32_t* d_drone, const int32_t* d_n_obj, const FilterIO& io);
int bodies_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int K_max, const BodiesIO& io);
int bodies_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts, const BodiesIO& io);
int markers_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int K_max, const MarkersIO& io);
int markers_times_check(mocap_ctx* ctx, const char* who, int64_t n_frames, const double* t);  // host time stamps: all finite
int markers_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts, const MarkersIO& io);
// body tracker (body_track_capi.hip): behind the rigid-body stage, whose found / assign arrays of the same frames it reads
int tracked_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int K_max, int B_max, const TrackedIO& io);
int tracked_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts, int B_max,
                       const int32_t* d_rb_found, const int8_t* d_rb_assign, const TrackedIO& io);
int tracked_clear_locked(mocap_ctx* ctx);  // all slots cleared, on the stream; nothing with the tracker off
// point consolidation (point_consolidate_capi.hip): the stage of the live loop between the re-submit and everything that reads the points
int consolidate_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int K_max);
int consolidate_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, double* d_xyz, double* d_err, int16_t* d_corr, int32_t* d_n_pts,
                           const int32_t* d_status, int32_t* d_src, int32_t* d_n_in);
// point refinement (point_refine_capi.hip): the stage of the live loop between the re-submit and the consolidation
int refine_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int M_max, int K_max, int iters);
int refine_dev_locked(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs, const int32_t* d_counts, int K_max, int iters,
                      double* d_xyz, double* d_err, const int16_t* d_corr, const int32_t* d_n_pts, const int32_t* d_status,
                      int32_t* d_info);

// copier for copy_fields (io_fields.hpp) on the context's stream
struct StreamCopy {
  mocap_ctx* ctx;
  hipMemcpyKind kind;
  int operator()(void* dst, const void* src, size_t bytes) const {
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
    return 0;
  }
};
