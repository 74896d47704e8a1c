// frame_capi.hip -- C ABI of the frame path (include/mocap_core.h): which kernel a batch takes (plan_frame), the
// launch (match_dev_locked), the device-side re-submit of frames that hit a cap (resubmit_dev_locked), the host and
// "_dev" entry points built from them, and the live loop in one call (mocap_track_*): track_locked behind the host forms,
// track_dev_locked behind the device forms, the optional stages handed to both as one TrackStages and laid out, staged and
// copied back through their field lists (io_fields.hpp).  Host runtime only.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "../../include/mocap_core.h"
#include "ctx.hpp"
#include "jpeg_tables.hpp"

using namespace mocap;

namespace {

// what every frame-path function is handed: the batch ...
struct FrameBatch {
  int64_t n_frames;
  int M_max;
  const float* blobs;     // [n_frames][C][M_max][2]
  const int32_t* counts;  // [n_frames][C]
  double gate_px;
};
// ... and where its results go (n_cand may be null)
struct FrameOut {
  double* xyz;
  double* err;
  int16_t* corr;
  int32_t* n_out;
  int32_t* status;
  int32_t* n_cand;
};

// the sizes plan_frame and frame_shape_fits decide on
constexpr size_t kLdsBytes = 160 * 1024;
bool must_go_wide(const mocap_ctx* ctx, int M_max) { return ctx->force_wide != 0 || (M_max > 255 && ctx->cv.uniformK); }
size_t frame_lds(const mocap_ctx* ctx, int M_max, int K_max, int T, int hit_cap, bool wide) {
  return frame_lds_bytes(ctx->C, M_max, K_max, T, hit_cap, wide, !wide && ctx->cv.uniformK != 0);
}

// which kernel a frame batch of this shape takes (the decision is per launch and never changes a result)
struct FramePlan {
  int T = 256, hit_cap = 1;
  bool wide = false, use_bb = false;
  size_t lds = 0;
};
FramePlan plan_frame(const mocap_ctx* ctx, int M_max, int K_max, int hit_cap_override) {
  FramePlan pl;
  // automatic workgroup size: tiny frames (4 x 4: a handful of candidates) are latency-bound, one wave
  // per frame keeps 4x more frames in flight per CU; everything else wants 256 lanes per frame
  pl.T = ctx->frame_threads ? ctx->frame_threads : (ctx->C * M_max <= 32 ? 64 : 256);
  const int cap = hit_cap_override > 0 ? hit_cap_override : ctx->hit_cap;
  pl.hit_cap = cap < 1 ? 1 : (cap > M_max ? M_max : cap);
  // (a narrow frame with identical intrinsics keeps blob indices in one byte with 0xFF = none: 256 slots go wide)
  pl.wide = must_go_wide(ctx, M_max);
  // The realistic rigs go to their own kernel (csrc/frame_bb.hip: exact branch and bound): plain intrinsics, identical or one
  // matrix per camera (the eigenvalue bounds need every K = [[fx,0,cx],[0,fy,cy],[0,0,1]]: p3max2 > 0 says so), <= 16 cameras, <= 64 blobs per camera, <= 255 roots,
  // frames big enough for a 256-lane workgroup (or 256 lanes asked for: MOCAP_FRAME_THREADS / mocap_set_tuning).  Everything
  // else -- and MOCAP_EVAL_BB=0 -- takes the exhaustive walk.  (Decided before narrow / wide: its layout has no odometer columns and fits where the general narrow one does not.)
  pl.use_bb = ctx->eval_bb && !ctx->exhaustive && !pl.wide && ctx->prune && ctx->eigcut && ctx->p3max2 > 0.0 && ctx->p3max2c > 0.0 &&
              (ctx->frame_threads == 256 || (ctx->frame_threads == 0 && ctx->C * M_max > 32)) && ctx->frame_launches != 3 &&
              frame_bb_fits(ctx->C, M_max, K_max);
  if (pl.use_bb) {
    pl.T = 256;
    pl.lds = frame_bb_lds_bytes(ctx->C, M_max, K_max);
  } else if (!pl.wide) {
    pl.lds = frame_lds(ctx, M_max, K_max, pl.T, pl.hit_cap, false);
    while (pl.lds > kLdsBytes && pl.T > 64) {
      pl.T /= 2;
      pl.lds = frame_lds(ctx, M_max, K_max, pl.T, pl.hit_cap, false);
    }
    pl.wide = pl.lds > kLdsBytes;  // the frame state does not fit LDS: big tables go to an HBM workspace
  }
  if (pl.wide) {
    pl.T = kWideThreads;
    pl.lds = frame_lds(ctx, M_max, K_max, pl.T, pl.hit_cap, true);
    // Round 6: 512 lanes per frame and TWO frames per CU wherever the LDS holds two frame states (64 cameras x 256 blobs:
    // up to ~400 roots).  The same 16 waves per CU and 128 VGPRs, no arithmetic changed -- but two independent frames in
    // different phases (the matching's scalar-heavy pre-test loop, the geometry's FP64) share the SIMDs' issue slots, and
    // every barrier waits for 8 waves instead of 16: 33.3 -> 28.9 ms per 12 500 stress frames.  MOCAP_WIDE_THREADS=1024 = the old plan.
    const char* wt = getenv("MOCAP_WIDE_THREADS");
    const size_t l2 = frame_lds(ctx, M_max, K_max, 512, pl.hit_cap, true);
    if (!(wt && atoi(wt) == 1024) && 2 * l2 <= kLdsBytes && ctx->frame_launches != 3) {
      pl.T = 512;
      pl.lds = l2;
    }
  }
  return pl;
}

// does a frame batch with these sizes fit one of the frame kernels?  The sizes plan_frame decides on, with the hit
// lists uncapped (M_max, whatever the context's cap) and at the smallest workgroup plan_frame would come down to
// (whatever frame_threads asks for).
bool frame_shape_fits(const mocap_ctx* ctx, int M_max, int K) {
  if (frame_bb_fits(ctx->C, M_max, K) && (ctx->cv.uniformK || ctx->p3max2 > 0.0) && !ctx->force_wide && M_max <= 255) return true;  // (one K per camera: the search takes them when all are plain)
  if (!must_go_wide(ctx, M_max) && frame_lds(ctx, M_max, K, 64, M_max, false) <= kLdsBytes) return true;
  return frame_lds(ctx, M_max, K, kWideThreads, M_max, true) <= kLdsBytes;
}

// heavy: null, or the export buffer of the heavy-root search (re-submit pass, wide variant only): roots over G_cap are
// exported instead of flagging their frames (FrameArgs::heavy_bb)
struct HeavyHook {
  int32_t* count;
  unsigned char* recs;
  int cap;
};

// match_dev_locked, part 1: the kernel's arguments from the call, the context and the plan (workspace and work queues:
// filled in by the parts below)
FrameArgs frame_args(const mocap_ctx* ctx, const FrameBatch& b, int K_max, int64_t G_cap, const FrameOut& o,
                     const FramePlan& pl, const int32_t* n_frames_dev, const HeavyHook* heavy) {
  const int M_max = b.M_max;
  FrameArgs a;
  a.cv = ctx->cv;
  a.n_frames = b.n_frames;
  a.n_frames_dev = n_frames_dev;
  a.M = M_max;
  a.K_max = K_max;
  a.gate_px = b.gate_px;
  a.G_cap = G_cap;
  a.blobs = b.blobs;
  a.counts = b.counts;
  a.xyz = o.xyz;
  a.err = o.err;
  a.corr = o.corr;
  a.n_out = o.n_out;
  a.status = o.status;
  a.n_cand = o.n_cand;
  a.world = ctx->world_on ? (const double*)ctx->world.ptr : nullptr;
  a.H = pl.hit_cap;
  a.wide = pl.wide ? 1 : 0;
  if (pl.wide) {  // A/B and tests: MOCAP_WIDE_SPEC=0 = the chain over the cameras strictly camera by camera (frame_kernel.hip spec_begin)
    const char* sp = getenv("MOCAP_WIDE_SPEC");
    if (sp && atoi(sp) == 0) a.wide = 2;
  }
  a.prune = ctx->prune && !ctx->exhaustive;
  a.p3max2 = a.prune && ctx->eigcut ? ctx->p3max2 : 0.0;
  if (!pl.wide && ctx->frame_threads == 0 && pl.T == 64) a.p3max2 = 0.0;  // tiny frames (a handful of candidates): the cut-offs cost more than they save
  a.eval_bb = pl.use_bb ? 1 : 0;
  a.bb_pl = ctx->bb_pl;
  a.bb_nb_max = ctx->bb_nb_max;
  for (int i = 0; i < 3; i++) a.bb_c0[i] = ctx->eig_c0[i];
  a.p3max2c = ctx->p3max2c;
  a.bb_flush = ctx->bb_flush > 0 ? ctx->bb_flush : 256;
  a.bb_min_g = ctx->bb_min_g;
  while (a.bb_pl > 1 && (size_t)a.bb_pl * M_max * 2 * 256 >= ((size_t)1 << 22)) a.bb_pl /= 2;  // expanded-list counter: 22 bits
  a.bb_pl_min = ctx->bb_pl_min < a.bb_pl ? ctx->bb_pl_min : a.bb_pl;
  a.ws = nullptr;
  a.ws_stride = 0;
  const bool hv = heavy && pl.wide;
  a.heavy_bb = hv ? 1 : 0;
  a.heavy_cap = hv ? heavy->cap : 0;
  a.heavy_count = hv ? heavy->count : nullptr;
  a.heavy_recs = hv ? heavy->recs : nullptr;
  a.heavy_stride = hv ? heavy_rec_bytes(ctx->C, pl.hit_cap) : 0;
  return a;
}

// the work queues' buffer: counters | slice -> heavy-list slot | slice generation | heavy-frame list | slice partials
size_t lay_queues(FrameQueues& q, void* base, int K_max) {
  Carver c(base);
  q.counters = c.take<int32_t>(QC_COUNT);
  q.slice_heavy = c.take<int32_t>(q.W_cap);
  q.slice_gen = c.take<int32_t>(q.W_cap);
  q.heavy = c.take<int32_t>(4 * (size_t)q.H_cap);
  q.part_e = c.take<double>((size_t)q.W_cap * K_max);
  q.part_g = c.take<uint32_t>((size_t)q.W_cap * K_max);
  q.part_x = c.take<double>(3 * (size_t)q.W_cap * K_max);
  return c.off;
}

// match_dev_locked, part 2: work queues -- heavy-frame list + slice partials (scheduling note in frame_kernel.hip) --
// sized, laid out and, where the launch cannot rely on what the previous one left, cleared
int prepare_queues(mocap_ctx* ctx, FrameArgs& a, const FramePlan& pl, int64_t full_grid, bool one_launch) {
  const int64_t n_frames = a.n_frames;
  const bool batch = n_frames >= 2 * full_grid;
  FrameQueues& q = a.q;
  q.heavy_threshold = ctx->heavy_threshold >= 0 ? (uint32_t)ctx->heavy_threshold : (batch ? 32768u : 16u * pl.T);  // batch: swept under the single-launch schedule (16 k: 13.45, 24-32 k: 13.32, 48 k: 13.50, 64 k: 13.72 ms per 100 k frames); live calls: swept, p50 0.129 -> 0.117 ms vs 2T, same p99
  // (wide frames: every slice re-does the frame's matching, ~2/3 of an average frame's time, so the slices are three times as long --
  // swept at the stress shape on two streams in round 6: 8 192 -> 24 576 candidates: 26.97 -> 25.65 and 24.82 -> 24.56 ms per
  // 12 500 frames; 16 384 / 20 480 / 28 672 / 32 768 in between or worse, 65 536: 30.5)
  q.slice_size = ctx->slice_size > 0 ? (uint32_t)ctx->slice_size : (batch ? (pl.wide ? 24576u : 8192u) : 4u * pl.T);
  if (a.heavy_bb) q.heavy_threshold = 0;  // (a sliced frame would be matched, and its heavy roots exported, once per slice)
  // small frames: amortise the queue atomic over a chunk (keeps >= 64 chunks per workgroup for balance);
  // frames with real work keep the finest granularity, their candidate counts are heavy-tailed
  q.frame_chunk = 1;
  if (ctx->C * a.M <= 32) {
    int64_t ch = n_frames / (full_grid * 64);
    q.frame_chunk = (int)(ch < 1 ? 1 : (ch > 16 ? 16 : ch));
  }
  int64_t H = n_frames / 8;
  if (H < 64) H = 64;
  if (H > n_frames) H = n_frames;
  q.H_cap = (int)H;
  q.W_cap = (int)(H * 8 < 64 ? 64 : H * 8);
  const int qs = a.n_frames_dev ? 1 : 0;  // the re-submit's second pass keeps queues of its own
  DevBuf& wq = qs ? ctx->resub_q : ctx->scratch[3];
  const void* wq_before = wq.ptr;
  if (wq.reserve(lay_queues(q, nullptr, a.K_max))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(frame work queues) failed");
  lay_queues(q, wq.ptr, a.K_max);
  // one-launch schedule: the kernel leaves the counters at zero and slices carry a launch generation, so the queue
  // needs clearing only when the buffer is new, the layout moved, or the other schedule used it last
  const bool fresh = wq.ptr != wq_before || ctx->frame_q_cap[qs] != q.W_cap || !ctx->frame_q_clean[qs];
  q.gen = ++ctx->frame_gen;
  if (ctx->frame_gen == 0x7fffffff) {  // generation wrap: start over from a cleared queue
    ctx->frame_gen = 0;
    ctx->frame_q_dirty();
  }
  if ((!one_launch && !pl.use_bb) || fresh) {
    const size_t b_slice = Carver::padded<int32_t>(q.W_cap);
    HIP_TRY(ctx, hipMemsetAsync(q.counters, 0, Carver::padded<int32_t>(QC_COUNT), ctx->stream));
    if (q.heavy_threshold) HIP_TRY(ctx, hipMemsetAsync(q.slice_heavy, 0xFF, b_slice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(q.slice_gen, 0, b_slice, ctx->stream));
  }
  ctx->frame_q_cap[qs] = q.W_cap;
  ctx->frame_q_clean[qs] = false;  // until the launch is known to be queued
  return MOCAP_OK;
}

// match_dev_locked, part 3: one of five launches
int launch_frames(mocap_ctx* ctx, const FrameArgs& a, const FramePlan& pl, int64_t full_grid, bool one_launch) {
  const FrameQueues& q = a.q;
  const int qs = a.n_frames_dev ? 1 : 0, T = pl.T;
  const int64_t grid = full_grid < a.n_frames ? full_grid : a.n_frames;
  if (pl.use_bb) {
    // frames only: a frame's cost follows its surviving blocks, not its candidate count -- no heavy list, no slices
    ctx->last_frame_kernel = ctx->cv.uniformK ? (ctx->C <= 8 ? "frame_bb_kernel<CW=1>" : "frame_bb_kernel<CW=2>")
                                              : (ctx->C <= 8 ? "frame_bb_kernel<CW=1, per-camera K>" : "frame_bb_kernel<CW=2, per-camera K>");
    HIP_TRY(ctx, launch_frame_bb(a, (int)grid, ctx->stream));
    ctx->frame_q_clean[qs] = true;
    return MOCAP_OK;
  }
  ctx->last_frame_kernel = pl.wide ? (T == 512 ? "frame_kernel<512, wide>" : "frame_kernel<1024, wide>") : (T == 64 ? "frame_kernel<64>" : (T == 128 ? "frame_kernel<128>" : "frame_kernel<256>"));
  if (one_launch) {
    // one launch: frames, then slices of the heavy frames, merged by the workgroup that finishes a frame's last slice.
    // Few frames (live calls): still enough workgroups for a heavy frame's slices to run side by side.
    int64_t g1 = a.n_frames + (q.heavy_threshold ? 64 : 0);
    if (g1 > full_grid) g1 = full_grid;
    HIP_TRY(ctx, launch_frame_kernel(a, MODE_ALL, T, (int)g1, ctx->stream));
    ctx->frame_q_clean[qs] = true;
    return MOCAP_OK;
  }
  HIP_TRY(ctx, launch_frame_kernel(a, MODE_MAIN, T, (int)grid, ctx->stream));
  if (q.heavy_threshold) {
    HIP_TRY(ctx, launch_frame_kernel(a, MODE_SLICE, T, (int)(full_grid < q.W_cap ? full_grid : q.W_cap), ctx->stream));
    HIP_TRY(ctx, launch_frame_kernel(a, MODE_MERGE, T, (int)(full_grid < q.H_cap ? full_grid : q.H_cap), ctx->stream));
  }
  return MOCAP_OK;
}

// hit_cap_override > 0: the hit-list cap of THIS launch (the re-submit pass keeps every gated hit) -- an argument, never a
// change of the context's state.  n_frames_dev != null: the batch is min(*n_frames_dev, n_frames) frames long.
int match_dev_locked(mocap_ctx* ctx, const FrameBatch& b, int K_max, int64_t G_cap, const FrameOut& o,
                     int hit_cap_override = 0, const int32_t* n_frames_dev = nullptr, const HeavyHook* heavy = nullptr) {
  const int M_max = b.M_max;
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
  if (b.n_frames < 0 || M_max < 1 || K_max < 1 || G_cap < 1)
    return ctx->fail(MOCAP_E_ARG, "mocap_match_triangulate: bad size argument");
  if (b.n_frames == 0) return MOCAP_OK;
  if (!b.blobs || !b.counts || !o.xyz || !o.err || !o.corr || !o.n_out || !o.status)
    return ctx->fail(MOCAP_E_ARG, "mocap_match_triangulate: null buffer");
  if (M_max > kMaxBlobs) return ctx->fail(MOCAP_E_LIMIT, "M_max=%d exceeds %d", M_max, kMaxBlobs);
  if (G_cap > (1ll << 24)) G_cap = 1ll << 24;  // 32-bit candidate offsets per frame
  const FramePlan pl = plan_frame(ctx, M_max, K_max, hit_cap_override);
  if (pl.wide && pl.lds > kLdsBytes)
    return ctx->fail(MOCAP_E_LIMIT, "frame state needs %zu B of LDS (C=%d, M_max=%d, K_max=%d): lower K_max",
                     pl.lds, ctx->C, M_max, K_max);
  FrameArgs a = frame_args(ctx, b, K_max, G_cap, o, pl, n_frames_dev, heavy);
  // persistent grid: enough workgroups to fill every CU at the LDS-limited occupancy
  int per_cu = (int)(kLdsBytes / pl.lds);
  const int wave_cap = pl.use_bb ? frame_bb_wg_per_cu_cap(ctx->C, M_max, K_max) : (16 / (pl.T / 64) > 0 ? 16 / (pl.T / 64) : 1);  // 128 VGPRs -> 16 waves per CU (the headline kernel: its instantiation's own budget)
  if (per_cu > wave_cap) per_cu = wave_cap;
  if (per_cu < 1) per_cu = 1;
  const int64_t full_grid = (int64_t)ctx->num_cus * per_cu;
  if (pl.use_bb) {
    // the winners' records, in a buffer of their own (not the wide variant's frame_ws: a wide second pass behind a search first
    // pass would grow that one, and DevBuf::reserve frees what it replaces): one size whatever the layout and the grid of this
    // call (num_cus * kBBMaxWgPerCu >= full_grid), allocated by the context's first search pass and never again -- nothing is
    // ever freed behind a launch that is still queued on it (the re-submit's second pass follows the first at once)
    a.ws_stride = frame_bb_ws_bytes(ctx->C);
    const size_t ws_bytes = (size_t)ctx->num_cus * kBBMaxWgPerCu * a.ws_stride;
    if (ctx->bb_ws.reserve(ws_bytes)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(search workspace, %zu B) failed", ws_bytes);
    a.ws = (unsigned char*)ctx->bb_ws.ptr;
  }
  if (pl.wide) {
    a.ws_stride = frame_ws_bytes(ctx->C, M_max, K_max, pl.T, pl.hit_cap, true, false);
    if (ctx->frame_ws.reserve((size_t)full_grid * a.ws_stride))
      return ctx->fail(MOCAP_E_HIP, "hipMalloc(wide-frame workspace, %zu B) failed", (size_t)full_grid * a.ws_stride);
    a.ws = (unsigned char*)ctx->frame_ws.ptr;
  }
  // Big batches of tiny frames (one-wave workgroups: 4 x 4) are bound by how many frames are in flight, and the lean
  // kernel of the three-launch schedule keeps twice the waves of the all-in-one kernel resident (measured on 1 M frames
  // of 4 x 4: 4.8 vs 8.2 ms); everything else takes the one persistent launch
  const bool tiny_batch = !pl.wide && ctx->frame_threads == 0 && pl.T == 64 && b.n_frames >= 4096;
  const bool one_launch = ctx->frame_launches != 3 && !(tiny_batch && !getenv("MOCAP_FRAME_LAUNCHES"));
  const int rc = prepare_queues(ctx, a, pl, full_grid, one_launch);
  return rc ? rc : launch_frames(ctx, a, pl, full_grid, one_launch);
}

// ------------------------------------------------------------------ re-submit on the device (uncapped enumeration)
// The reference enumerates the full Cartesian product whatever its size (helpers.py:394-400); the frame path works under
// caps (K_max roots, G_cap groups per root, hit_cap hits per pair of the wide variant) and reports per frame when one was
// hit.  Behind a first pass that is already queued: the flagged frames are gathered, on the device, into a scratch batch
// whose length stays on the device; the frame kernel runs on it with the largest caps the core has (root capacity C *
// M_max as far as a kernel's LDS holds it, G_cap = 2^24 groups per root, every gated hit of a (root, camera) pair kept);
// results that fit the caller's K_max slots are scattered back, the others report ROOT_OVERFLOW and the slots they need.
// Nothing here waits for the GPU: three enqueues behind the first pass (an empty list costs ~15 us of GPU time).
// d_info: null, or [2] device-accessible: {frames flagged, frames re-run}.

// the re-submit's scratch: frame list | gathered inputs | second-pass outputs, for a scratch batch of F2 frames
size_t lay_resubmit(ResubmitArgs& ra, FrameOut& o2, void* base, size_t F2, int C, int M_max, int K_big) {
  Carver c(base);
  ra.list = c.take<int32_t>(F2);
  ra.b2 = c.take<float>(F2 * C * M_max * 2);
  ra.c2 = c.take<int32_t>(F2 * C);
  ra.x2 = o2.xyz = c.take<double>(F2 * K_big * 3);
  ra.e2 = o2.err = c.take<double>(F2 * K_big);
  ra.r2 = o2.corr = c.take<int16_t>(F2 * K_big * C);
  ra.n2 = o2.n_out = c.take<int32_t>(F2 + 2);
  ra.s2 = o2.status = c.take<int32_t>(F2 + 2);  // (+ 2 slots: the self-check builds count in status[n_frames .. n_frames + 1])
  ra.g2 = o2.n_cand = c.take<int32_t>(F2 + 2);
  return c.off;
}

// the heavy-root enumeration's workspace: queue (list | slice | done | bounds) + per-workgroup winners
size_t lay_heavy_enum(HeavyArgs& ha, void* base, int enum_grid) {
  Carver c(base, 4);
  ha.enum_list = c.take<int32_t>(kHeavyEnumMax);
  ha.enum_slice = c.take<int32_t>(kHeavyEnumMax);
  ha.enum_done = c.take<int32_t>(kHeavyEnumMax);
  c.align_to(64);
  ha.enum_bound = c.take<unsigned long long>(kHeavyEnumMax);
  ha.enum_part = c.take<unsigned char>((size_t)kHeavyEnumMax * enum_grid * kHeavyEnumPartBytes);
  return c.off;
}

int resubmit_dev_locked(mocap_ctx* ctx, const FrameBatch& b, int K_max, const FrameOut& o, int32_t* d_info) {
  const int64_t n_frames = b.n_frames;
  const int M_max = b.M_max;
  if (n_frames <= 0) return MOCAP_OK;
  const int C = ctx->C;
  // worst-case root capacity: every blob its own root (never less than the caller asked for) ...
  int K_big = C * M_max < 1024 ? C * M_max : 1024;
  if (K_big < K_max) K_big = K_max;
  if (!frame_shape_fits(ctx, M_max, K_big)) {
    // ... as far as the frame state fits a kernel (64 cameras x 256 blobs: the per-root tables of the wide variant end at
    // a few hundred roots); a frame with more roots than that keeps its root-overflow status
    int lo = K_max, hi = K_big;  // largest K in [K_max, K_big) that fits (K_max itself ran above)
    while (lo < hi) {
      const int mid = (lo + hi + 1) / 2;
      if (frame_shape_fits(ctx, M_max, mid)) lo = mid; else hi = mid - 1;
    }
    K_big = lo;
  }
  const size_t per_frame = sizeof(float) * C * M_max * 2 + sizeof(int32_t) * C + (size_t)K_big * (32 + 2 * C) + 16;
  // the scratch batch holds every frame of the caller's batch unless that takes more than MOCAP_RESUBMIT_SCRATCH_MB
  // (default 8192); beyond it, flagged frames keep their status (d_info[0] > d_info[1] says so: call again)
  size_t budget = (size_t)8192 << 20;
  if (const char* e = getenv("MOCAP_RESUBMIT_SCRATCH_MB")) budget = (size_t)(atol(e) > 0 ? atol(e) : 1) << 20;
  // The scratch batch is sized for the flagged share one expects, not for the whole batch (round-5 advice: a full copy of a
  // 100 k-frame batch was reserved up front although no frame might be flagged): the whole batch while that costs at most
  // 256 MB (a caller's tiny G_cap may flag every frame of a small batch), else one frame in eight, at least 1 024 and at least
  // what 256 MB hold.  More
  // flagged frames than that keep their status without MOCAP_ST_FINAL and d_info says so; mocap_resubmit_dev (and the
  // host-buffer entry points, in a loop) continue with them.  An allocation that fails is retried at half the size down to
  // one frame: the first pass has succeeded by now, a missing scratch must not fail the call.
  int64_t cap = n_frames / 8 < 1024 ? 1024 : n_frames / 8;
  if (cap < (int64_t)(((size_t)256 << 20) / per_frame)) cap = (int64_t)(((size_t)256 << 20) / per_frame);
  if (const char* e = getenv("MOCAP_RESUBMIT_SCRATCH_FRAMES")) cap = atol(e) > 0 ? atol(e) : 1;  // (tests: a scratch smaller than the flagged set)
  if (cap > n_frames) cap = n_frames;
  if ((size_t)cap * per_frame > budget) cap = (int64_t)(budget / per_frame);
  if (cap < 1) cap = 1;
  ResubmitArgs ra;
  FrameOut o2;  // the second pass's outputs
  for (;;) {
    const size_t bytes = lay_resubmit(ra, o2, nullptr, (size_t)cap, C, M_max, K_big);
    if (!ctx->resub.reserve(bytes)) break;
    (void)hipGetLastError();  // (the failed hipMalloc's sticky error)
    if (cap == 1) return ctx->fail(MOCAP_E_HIP, "hipMalloc(re-submit scratch, %zu B for ONE frame) failed", bytes);
    cap = (cap + 1) / 2;
  }
  if (!ctx->resub_ctr.ptr) {
    if (ctx->resub_ctr.reserve(256)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(re-submit counters) failed");
    HIP_TRY(ctx, hipMemsetAsync(ctx->resub_ctr.ptr, 0, 256, ctx->stream));
  }
  lay_resubmit(ra, o2, ctx->resub.ptr, (size_t)cap, C, M_max, K_big);
  ra.n_frames = n_frames;
  ra.cap = cap;
  ra.C = C;
  ra.M = M_max;
  ra.K_max = K_max;
  ra.K_big = K_big;
  ra.status = o.status;
  ra.blobs = b.blobs;
  ra.counts = b.counts;
  // two counters, 128 bytes apart, alternate between calls: this call's is zero (the previous call's gather cleared it)
  // (the parity advances only once the gather -- which zeroes the OTHER counter for the next call -- is known to be queued:
  // a failure before that leaves this call's counter untouched and still zero)
  int32_t* ctr = (int32_t*)ctx->resub_ctr.ptr;
  const uint32_t par = ctx->resub_calls & 1u;
  ra.count = ctr + 32 * par;
  ra.count_next = ctr + 32 * (par ^ 1u);
  ra.xyz = o.xyz;
  ra.err = o.err;
  ra.corr = o.corr;
  ra.n_out = o.n_out;
  ra.status_out = o.status;
  ra.n_cand = o.n_cand;
  ra.info = d_info;
  // Roots whose product no enumeration reaches (two markers behind each other from the root's camera: 2^60 groups at 64
  // cameras) go to the heavy-root search (csrc/heavy_bb.hip) where the second pass runs the wide variant on cameras of the
  // form EigCut needs -- every intrinsic matrix plain, one for all cameras or one per camera (p3max2c > 0 says so; the kernels
  // take their variant from CamView::uniformK, which travels in HeavyArgs::cv) --: the pass enumerates up to
  // MOCAP_RESUBMIT_G_CAP groups per root (default 4096) and exports the roots above it; elsewhere (a skewed matrix, the
  // exhaustive walk, MOCAP_NO_HEAVY_BB) it enumerates up to 2^24 per root and flags what is larger, as before.
  const FramePlan pl2 = plan_frame(ctx, M_max, K_big, M_max);
  const bool heavy_ok = pl2.wide && (ctx->cv.uniformK || ctx->p3max2c > 0.0) && ctx->prune && ctx->eigcut && ctx->p3max2 > 0.0 && !ctx->exhaustive && !getenv("MOCAP_NO_HEAVY_BB");
  int64_t G2 = (int64_t)1 << 24;
  HeavyHook hk{nullptr, nullptr, 0};
  HeavyArgs ha;
  int ncap = 4096;  // (swept on the stress stream: 16 384 and 65 536 solve 1-3 more of ~30 hard roots per 12 500 frames and double the step)
  const int hv_grid = 64;
  const int enum_grid = ctx->num_cus * 3;  // heavy_enum_kernel: 256-lane workgroups (168 VGPRs: three waves per SIMD), the whole GPU on one root at a time
  if (const char* e = getenv("MOCAP_HEAVY_NCAP")) ncap = atoi(e) >= 1 ? atoi(e) : 1;  // (tests: 1 = the search gives up at the first level that keeps two nodes)
  if (heavy_ok) {
    G2 = 4096;
    if (const char* e = getenv("MOCAP_RESUBMIT_G_CAP")) G2 = atol(e) > 0 ? atol(e) : 1;
    hk.cap = 2048;
    if (ctx->heavy_recs.reserve((size_t)hk.cap * heavy_rec_bytes(C, M_max)) || ctx->heavy_ws.reserve((size_t)hv_grid * heavy_bb_ws_bytes(ncap)) ||
        ctx->heavy_enum.reserve(lay_heavy_enum(ha, nullptr, enum_grid) + 64))  // (+ 64: the slack this size has always had)
      return ctx->fail(MOCAP_E_HIP, "hipMalloc(heavy-root search buffers) failed");
    hk.recs = (unsigned char*)ctx->heavy_recs.ptr;
    hk.count = ctr + 16;  // (its own word of the counter block; the gather kernel zeroes it)
    ra.heavy_count = hk.count;
    ra.enum_count = ctr + 17;
  } else {
    ra.heavy_count = nullptr;
    ra.enum_count = nullptr;
  }
  HIP_TRY(ctx, launch_resubmit_gather(ra, ctx->stream));
  ctx->resub_calls++;
  const char* batch_kernel = ctx->last_frame_kernel;  // mocap_last_frame_kernel() keeps naming the pass that did the batch, not the repair of its flagged frames
  const int rc = match_dev_locked(ctx, FrameBatch{cap, M_max, ra.b2, ra.c2, b.gate_px}, K_big, G2, o2,
                                  /*hit_cap_override=*/M_max, /*n_frames_dev=*/ra.count, heavy_ok ? &hk : nullptr);
  if (std::strcmp(batch_kernel, "none") != 0) ctx->last_frame_kernel = batch_kernel;
  if (rc) return rc;
  if (heavy_ok) {
    ha.cv = ctx->cv;
    ha.M = M_max;
    ha.K_big = K_big;
    for (int i = 0; i < 3; i++) ha.bb_c0[i] = ctx->eig_c0[i];
    ha.p3max2c = ctx->p3max2c;
    ha.p3max2 = ctx->p3max2;
    ha.blobs = ra.b2;
    ha.heavy_count = hk.count;
    ha.recs = hk.recs;
    ha.cap = hk.cap;
    ha.stride = heavy_rec_bytes(C, M_max);
    ha.xyz = o2.xyz;
    ha.err = o2.err;
    ha.corr = o2.corr;
    ha.n_out = o2.n_out;
    ha.status = o2.status;
    ha.world = ctx->world_on ? (const double*)ctx->world.ptr : nullptr;
    ha.ws = (unsigned char*)ctx->heavy_ws.ptr;
    ha.ws_stride = heavy_bb_ws_bytes(ncap);
    ha.ncap = ncap;
    ha.enum_cap = (int64_t)1 << 16;  // (2^20 in place costs tens of ms on one CU: the first pass, which slices such roots over 64 workgroups, is the place for them)
    if (const char* e = getenv("MOCAP_HEAVY_ENUM_CAP")) ha.enum_cap = atol(e) >= 0 ? atol(e) : 0;
    ha.debug = getenv("MOCAP_HEAVY_DEBUG") ? 1 : 0;
    // roots the search gives up on with at most 2^24 groups are enumerated by the whole GPU behind it (heavy_enum_kernel):
    // the pass stays exact up to 2^24 groups per root, like the enumeration it replaces (round-5 advice)
    ha.enum_max = (getenv("MOCAP_NO_HEAVY_ENUM") || (ctx->flags & MOCAP_OPT_BOUNDED_RESUBMIT)) ? 0 : kHeavyEnumMax;
    ha.enum_grid = enum_grid;
    ha.enum_count = ctr + 17;
    lay_heavy_enum(ha, ctx->heavy_enum.ptr, enum_grid);
    HIP_TRY(ctx, launch_heavy_bb(ha, hv_grid, ctx->stream));
    HIP_TRY(ctx, launch_heavy_enum(ha, ctx->stream));
  }
  HIP_TRY(ctx, launch_resubmit_scatter(ra, ctx->stream));
  return MOCAP_OK;
}

}  // namespace

extern "C" int mocap_match_triangulate_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs,
                                           const int32_t* d_counts, double gate_px, int K_max, int64_t G_cap,
                                           double* d_xyz, double* d_err, int16_t* d_corr, int32_t* d_n_out,
                                           int32_t* d_status, int32_t* d_n_cand) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = match_dev_locked(ctx, FrameBatch{n_frames, M_max, d_blobs, d_counts, gate_px}, K_max, G_cap,
                                  FrameOut{d_xyz, d_err, d_corr, d_n_out, d_status, d_n_cand});
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_resubmit_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs, const int32_t* d_counts,
                                  double gate_px, int K_max, double* d_xyz, double* d_err, int16_t* d_corr, int32_t* d_n_out,
                                  int32_t* d_status, int32_t* d_n_cand, int32_t* d_resubmitted) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
  if (n_frames < 0 || M_max < 1 || K_max < 1) return ctx->fail(MOCAP_E_ARG, "mocap_resubmit_dev: bad size argument");
  if (n_frames > 0 && (!d_blobs || !d_counts || !d_xyz || !d_err || !d_corr || !d_n_out || !d_status))
    return ctx->fail(MOCAP_E_ARG, "mocap_resubmit_dev: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = resubmit_dev_locked(ctx, FrameBatch{n_frames, M_max, d_blobs, d_counts, gate_px}, K_max,
                                     FrameOut{d_xyz, d_err, d_corr, d_n_out, d_status, d_n_cand}, d_resubmitted);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_match_triangulate_dev_auto(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs,
                                                const int32_t* d_counts, double gate_px, int K_max, int64_t G_cap,
                                                double* d_xyz, double* d_err, int16_t* d_corr, int32_t* d_n_out,
                                                int32_t* d_status, int32_t* d_n_cand, int32_t* d_resubmitted) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const FrameBatch b{n_frames, M_max, d_blobs, d_counts, gate_px};
  const FrameOut o{d_xyz, d_err, d_corr, d_n_out, d_status, d_n_cand};
  int rc = match_dev_locked(ctx, b, K_max, G_cap, o);
  if (rc) return rc;
  rc = resubmit_dev_locked(ctx, b, K_max, o, d_resubmitted);
  return rc ? rc : ctx->mark_enqueued();
}

namespace {

// The host entry points' re-submit: rounds of the device-side second pass until no flagged frame is left behind (more
// than one round only when the scratch batch was smaller than the flagged set).  d_info: the two words
// resubmit_dev_locked reports in; h_info: where the host reads them -- the same words when they are in pinned host
// memory, else a copy precedes the synchronise.  *total: frames re-run.
int resubmit_rounds(mocap_ctx* ctx, const FrameBatch& b, int K_max, const FrameOut& o, int32_t* d_info, int32_t* h_info,
                    int* total) {
  *total = 0;
  for (;;) {
    const int rc = resubmit_dev_locked(ctx, b, K_max, o, d_info);
    if (rc) return rc;
    if (h_info != d_info) HIP_TRY(ctx, hipMemcpyAsync(h_info, d_info, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *total += h_info[1];
    if (h_info[0] <= h_info[1] || h_info[1] <= 0) return MOCAP_OK;
  }
}

// a batch's results from pinned staging `h` to the caller's `o` (corr, n_cand: optional): only the slots the kernel
// wrote (n_out per frame) carry data; the caller's buffers keep their fill beyond
void copy_valid_slots(size_t F, int C, int K_max, const FrameOut& h, const FrameOut& o) {
  memcpy(o.n_out, h.n_out, sizeof(int32_t) * F);
  memcpy(o.status, h.status, sizeof(int32_t) * F);
  if (o.n_cand) memcpy(o.n_cand, h.n_cand, sizeof(int32_t) * F);
  for (size_t f = 0; f < F; f++) {
    const size_t k = (size_t)((h.n_out[f] < 0 || h.n_out[f] > K_max) ? 0 : h.n_out[f]);  // > K_max: needs more slots, nothing written
    memcpy(o.xyz + f * K_max * 3, h.xyz + f * K_max * 3, sizeof(double) * 3 * k);
    memcpy(o.err + f * K_max, h.err + f * K_max, sizeof(double) * k);
    if (o.corr) memcpy(o.corr + f * K_max * C, h.corr + f * K_max * C, sizeof(int16_t) * C * k);
  }
}

// host buffers in, host buffers out; resubmit: frames that hit a cap take the device-side second pass before the results
// travel back (one lock, one synchronisation)
int match_host_locked(mocap_ctx* ctx, const FrameBatch& b, int K_max, int64_t G_cap, const FrameOut& o, bool resubmit,
                      int32_t* n_resubmitted) {
  const int M_max = b.M_max;
  if (n_resubmitted) *n_resubmitted = 0;
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
  if (b.n_frames < 0 || M_max < 1 || K_max < 1) return ctx->fail(MOCAP_E_ARG, "mocap_match_triangulate: bad size argument");
  if (b.n_frames == 0) return MOCAP_OK;
  if (!b.blobs || !b.counts || !o.xyz || !o.err || !o.corr || !o.n_out || !o.status)
    return ctx->fail(MOCAP_E_ARG, "mocap_match_triangulate: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int C = ctx->C;
  const size_t F = (size_t)b.n_frames;
  const size_t b_blobs = sizeof(float) * F * C * M_max * 2, b_counts = sizeof(int32_t) * F * C,
               b_xyz = sizeof(double) * F * K_max * 3, b_err = sizeof(double) * F * K_max,
               b_corr = sizeof(int16_t) * F * K_max * C, b_i = sizeof(int32_t) * F;
  // staging (pinned host or device memory): outputs | inputs | per-frame words | the re-submit's two info words
  float* s_blobs;
  int32_t *s_counts, *info;
  FrameOut s;
  auto lay = [&](void* base) {
    Carver c(base);
    s.xyz = c.take<double>(F * K_max * 3);
    s.err = c.take<double>(F * K_max);
    s_blobs = c.take<float>(F * C * M_max * 2);
    s_counts = c.take<int32_t>(F * C);
    s.corr = c.take<int16_t>(F * K_max * C);
    s.n_out = c.take<int32_t>(F);
    s.status = c.take<int32_t>(F);
    s.n_cand = c.take<int32_t>(F);
    info = c.take<int32_t>(2);
    return c.off;
  };
  const size_t total = lay(nullptr);
  int n_rerun = 0;
  // Live tracking (one or a few frames per call, helpers.py:94): zero-copy through pinned host memory.
  // The kernels read the blobs from, and write the points to, device-visible host memory; eight small
  // copy-engine transfers and a sleeping stream synchronise cost several times the kernels themselves.
  // Not for frames that go to the wide variant: it reads the blobs IN PLACE for every root batch and candidate view,
  // which over PCIe from uncached host memory costs far more than one staged copy.
  if (total <= (size_t)256 * 1024 && !plan_frame(ctx, M_max, K_max, 0).wide) {
    HIP_TRY(ctx, ctx->live_pin.reserve(total, (size_t)256 * 1024, hipHostMallocDefault));
    lay(ctx->live_pin.ptr);
    info[0] = info[1] = 0;
    memcpy(s_blobs, b.blobs, b_blobs);
    memcpy(s_counts, b.counts, b_counts);
    const FrameBatch in{b.n_frames, M_max, s_blobs, s_counts, b.gate_px};
    int rc = match_dev_locked(ctx, in, K_max, G_cap, s);
    if (rc) return rc;
    rc = spin_wait(ctx, ctx->live_event);
    if (rc) return rc;
    bool flagged = false;
    for (size_t f = 0; f < F && resubmit; f++) flagged |= s.status[f] != 0;
    if (flagged) {  // rare: the second pass is queued only when the first one, already back, asks for it
      rc = resubmit_rounds(ctx, in, K_max, s, info, info, &n_rerun);
      if (rc) return rc;
    }
    copy_valid_slots(F, C, K_max, s, o);
    if (n_resubmitted) *n_resubmitted = n_rerun;
    return MOCAP_OK;
  }
  DevBuf& dev = ctx->scratch[0];
  if (dev.reserve(total)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%zu) failed", total);
  lay(dev.ptr);
  HIP_TRY(ctx, hipMemcpyAsync(s_blobs, b.blobs, b_blobs, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(s_counts, b.counts, b_counts, hipMemcpyHostToDevice, ctx->stream));
  const FrameBatch in{b.n_frames, M_max, s_blobs, s_counts, b.gate_px};
  int rc = match_dev_locked(ctx, in, K_max, G_cap, s);
  if (rc) return rc;
  if (resubmit) {
    int32_t h_info[2] = {0, 0};
    rc = resubmit_rounds(ctx, in, K_max, s, info, h_info, &n_rerun);
    if (rc) return rc;
  }
  HIP_TRY(ctx, hipMemcpyAsync(o.xyz, s.xyz, b_xyz, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(o.err, s.err, b_err, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(o.corr, s.corr, b_corr, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(o.n_out, s.n_out, b_i, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(o.status, s.status, b_i, hipMemcpyDeviceToHost, ctx->stream));
  if (o.n_cand) HIP_TRY(ctx, hipMemcpyAsync(o.n_cand, s.n_cand, b_i, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (n_resubmitted) *n_resubmitted = n_rerun;
  return MOCAP_OK;
}

}  // namespace

extern "C" int mocap_match_triangulate(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs,
                                       const int32_t* counts, double gate_px, int K_max, int64_t G_cap,
                                       double* xyz, double* err, int16_t* corr, int32_t* n_out,
                                       int32_t* status, int32_t* n_cand) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return match_host_locked(ctx, FrameBatch{n_frames, M_max, blobs, counts, gate_px}, K_max, G_cap,
                           FrameOut{xyz, err, corr, n_out, status, n_cand}, false, nullptr);
}

// ------------------------------------------------------------------ C-level re-submit (uncapped enumeration)
// mocap_match_triangulate_auto gives every caller of the C ABI what mocap_core/capi.py used to do in Python: frames whose
// status is non-zero are re-submitted, on the GPU, with the largest caps the core has -- under ONE acquisition of the
// context lock, with the hit-list cap of the second pass an argument of its launch (round 4 flipped ctx->hit_cap between
// two locked calls: a concurrent mocap_set_frame_limits was overwritten, a concurrent frame call ran under the foreign cap).
extern "C" int mocap_match_triangulate_auto(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs,
                                            const int32_t* counts, double gate_px, int K_max, int64_t G_cap,
                                            double* xyz, double* err, int16_t* corr, int32_t* n_out, int32_t* status,
                                            int32_t* n_cand, int32_t* n_resubmitted) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return match_host_locked(ctx, FrameBatch{n_frames, M_max, blobs, counts, gate_px}, K_max, G_cap,
                           FrameOut{xyz, err, corr, n_out, status, n_cand}, true, n_resubmitted);
}

// ------------------------------------------------------------------ double-precision centroids at the boundary
// The reference measures on whatever its image_points lists hold (helpers.py:367-373): int64 for _find_dot's int()
// centroids, float64 for anything else.  The kernels carry blob coordinates as float32 (half the LDS / HBM bytes of the
// one array every phase reads).  This entry takes doubles: coordinates float32 can represent -- every integer pixel below
// 2^24, every float32-valued sub-pixel centroid -- go through unchanged, i.e. EXACTLY as the reference would see them;
// anything else is rounded to the nearest float32 (|dx| <= 2^-24 |x|: 2e-5 px at 320 px, far inside north_star's 1e-5
// relative on the points) and the frame is FLAGGED (MOCAP_ST_ROUNDED, informational: the outputs are valid) instead of
// being refused or silently altered.  NaN / inf coordinates are an argument error.
extern "C" int mocap_match_triangulate_f64(mocap_ctx* ctx, int64_t n_frames, int M_max, const double* blobs,
                                           const int32_t* counts, double gate_px, int K_max, int64_t G_cap, double* xyz,
                                           double* err, int16_t* corr, int32_t* n_out, int32_t* status, int32_t* n_cand,
                                           int32_t* n_resubmitted) {
  if (!ctx) return MOCAP_E_ARG;
  int C;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
    if (n_frames < 0 || M_max < 1 || K_max < 1) return ctx->fail(MOCAP_E_ARG, "mocap_match_triangulate_f64: bad size argument");
    if (n_frames > 0 && (!blobs || !counts || !status)) return ctx->fail(MOCAP_E_ARG, "mocap_match_triangulate_f64: null buffer");
    C = ctx->C;
  }
  const size_t per = (size_t)C * M_max * 2;
  std::vector<float> b32;
  std::vector<uint8_t> rounded;
  try {
    b32.resize((size_t)n_frames * per);
    rounded.assign((size_t)n_frames, 0);
  } catch (const std::exception& ex) {
    return ctx->fail(MOCAP_E_HIP, "mocap_match_triangulate_f64: %s", ex.what());
  }
  for (int64_t f = 0; f < n_frames; f++)
    for (int c = 0; c < C; c++) {
      int n = counts[(size_t)f * C + c];
      n = n < 0 ? 0 : (n > M_max ? M_max : n);
      for (int k = 0; k < 2 * n; k++) {
        const size_t o = (size_t)f * per + (size_t)c * M_max * 2 + k;
        const double v = blobs[o];
        if (!(v - v == 0.0)) return ctx->fail(MOCAP_E_ARG, "mocap_match_triangulate_f64: frame %lld camera %d: coordinate is NaN or infinite", (long long)f, c);
        const float r = (float)v;
        b32[o] = r;
        if ((double)r != v) rounded[f] = 1;
      }
    }
  const int rc = mocap_match_triangulate_auto(ctx, n_frames, M_max, b32.data(), counts, gate_px, K_max, G_cap, xyz, err, corr, n_out,
                                              status, n_cand, n_resubmitted);
  if (rc) return rc;
  for (int64_t f = 0; f < n_frames; f++)
    if (rounded[f]) status[f] |= MOCAP_ST_ROUNDED;
  return MOCAP_OK;
}

// ------------------------------------------------------------------ the live loop in one call
// helpers.py:94-133 per frame: find_point_correspondance_and_object_points -> world coordinates -> locate_objects ->
// the `object-points` payload.  One enqueue: [blob stage ->] frame kernel (world epilogue fused in its store) -> one wave
// per frame that runs locate_objects and exports everything into pinned host memory; the host waits for ONE event.
namespace {

struct TrackOut {
  FrameOut pts;  // (corr optional, n_cand unused)
  int O_max; double* pos; double* heading; double* oerr; int32_t* drone; int32_t* n_obj;
  float* blobs = nullptr; int32_t* counts = nullptr; int32_t* blob_status = nullptr;  // (the forms that take raw frames)
};

// the optional stages behind the object search, null = off; an entry point hands over the one it carries
struct TrackStages {
  const FilterIO* filter = nullptr;    // mocap_track_frame_filtered: time stamps in, the object filter's outputs out
  const JpegOut* jpeg = nullptr;       // mocap_track_frame_images_jpeg: the preview stream
  const BodiesIO* bodies = nullptr;    // mocap_track_frame_bodies: the rigid-body locator
  const MarkersIO* markers = nullptr;  // mocap_track_frame_ids: time stamps in, the marker tracker's outputs out
  const TrackedIO* tracked = nullptr;  // mocap_track_frame_bodies_tracked: behind `bodies`, time stamps in, the body tracker's outputs out
  TrackStages() = default;
  TrackStages(const FilterIO& io) : filter(&io) {}
  TrackStages(const JpegOut& io) : jpeg(&io) {}
  TrackStages(const BodiesIO& io) : bodies(&io) {}
  TrackStages(const MarkersIO& io) : markers(&io) {}
  TrackStages(const BodiesIO& rb, const TrackedIO& io) : bodies(&rb), tracked(&io) {}
};

// The opt-in stages on the points themselves, between the re-submit and everything that reads the points, in their order:
// refinement (mocap_set_point_refinement), then consolidation (mocap_set_point_consolidation) -- the consolidation's key, the
// export, the object search and every stage behind see the refined points and errors.  Described here once for the host and the
// device forms; with both modes off nothing is checked and nothing is queued.  `have_corr`: a _dev form got a d_corr.
int point_stages_check(mocap_ctx* ctx, const char* who, const FrameBatch& b, int K_max, bool have_corr) {
  int rc = MOCAP_OK;
  if (ctx->refine_iters) rc = refine_check(ctx, who, b.n_frames, b.M_max, K_max, ctx->refine_iters);
  if (!rc && ctx->refine_iters && b.n_frames > 0 && !have_corr) rc = ctx->fail(MOCAP_E_ARG, "%s: point refinement is on and needs d_corr", who);
  if (!rc && ctx->consolidate) rc = consolidate_check(ctx, who, b.n_frames, K_max);
  if (!rc && ctx->consolidate && b.n_frames > 0 && !have_corr) rc = ctx->fail(MOCAP_E_ARG, "%s: point consolidation is on and needs d_corr", who);
  return rc;
}
// (`in`: the blobs and counts the frame pass read, device-visible; `d`: its outputs)
int point_stages_dev_locked(mocap_ctx* ctx, const FrameBatch& in, int K_max, const FrameOut& d) {
  int rc = MOCAP_OK;
  if (in.n_frames <= 0) return rc;
  if (ctx->refine_iters)
    rc = refine_dev_locked(ctx, in.n_frames, in.M_max, in.blobs, in.counts, K_max, ctx->refine_iters, d.xyz, d.err, d.corr, d.n_out, d.status, nullptr);
  if (!rc && ctx->consolidate) rc = consolidate_dev_locked(ctx, in.n_frames, K_max, d.xyz, d.err, d.corr, d.n_out, d.status, nullptr, nullptr);
  return rc;
}

// images != null: raw frames [F][C][rows][cols][3] (host); else b.blobs / b.counts (host) are the input.  The filter, the
// bodies, the markers and the tracked bodies are described once (io_fields.hpp): their arrays are carved from the same pinned block as the frame's
// outputs, their kernels are queued behind the export and write into that block, their outputs are copied to the caller -- the
// call still waits for one event.  The JPEG stream stays written out here: its slots have a 16-byte stride in the block and only
// the bytes that exist are copied back, which no field list says.
int track_locked(mocap_ctx* ctx, const uint8_t* images, const FrameBatch& b, int K_max, int64_t G_cap, const TrackOut& o,
                 const TrackStages& stages = {}) {
  const JpegOut* jo = stages.jpeg;
  const int64_t n_frames = b.n_frames;
  const int M_max = b.M_max;
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
  if (n_frames < 0 || M_max < 1 || K_max < 1 || G_cap < 1 || o.O_max < 0)
    return ctx->fail(MOCAP_E_ARG, "mocap_track_frame: bad size argument");
  if (n_frames == 0) return MOCAP_OK;
  if ((!images && (!b.blobs || !b.counts)) || !o.pts.xyz || !o.pts.err || !o.pts.n_out || !o.pts.status)
    return ctx->fail(MOCAP_E_ARG, "mocap_track_frame: null buffer");
  if (o.O_max > 0 && (!o.pos || !o.heading || !o.oerr || !o.drone || !o.n_obj))
    return ctx->fail(MOCAP_E_ARG, "mocap_track_frame: null object buffer");
  if (o.O_max > 0 && K_max > 256) return ctx->fail(MOCAP_E_LIMIT, "mocap_track_frame: K_max=%d exceeds 256 with the object search on", K_max);
  if (images && (!ctx->img_C || ctx->img_C != ctx->C))
    return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_image_params has not been called for this camera set");
  if (images && (!o.blobs || !o.counts || !o.blob_status)) return ctx->fail(MOCAP_E_ARG, "mocap_track_frame_images: null blob buffer");
  int rc = MOCAP_OK;
  if (stages.filter) rc = filter_check(ctx, "mocap_track_frame_filtered", n_frames, o.O_max, *stages.filter);
  const char* who_bodies = stages.tracked ? "mocap_track_frame_bodies_tracked" : "mocap_track_frame_bodies";
  if (!rc && stages.tracked) rc = tracked_check(ctx, who_bodies, n_frames, K_max, stages.bodies->B_max, *stages.tracked);
  if (!rc && stages.bodies) rc = bodies_check(ctx, who_bodies, n_frames, K_max, *stages.bodies);
  if (!rc && stages.tracked) rc = markers_times_check(ctx, who_bodies, n_frames, stages.tracked->t);
  if (!rc && stages.markers) rc = markers_check(ctx, "mocap_track_frame_ids", n_frames, K_max, *stages.markers);
  if (!rc && stages.markers) rc = markers_times_check(ctx, "mocap_track_frame_ids", n_frames, stages.markers->t);
  if (!rc) rc = point_stages_check(ctx, "mocap_track_frame", b, K_max, true);  // (the device block always has the rows)
  if (rc) return rc;
  if (jo) {  // the preview stream: the processed frames of the blob stage as one JPEG per frame set
    const char* bad = jpeg::check_args(n_frames, ctx->img_C, ctx->img_S, ctx->img_S, jo->quality, jo->capacity);
    if (bad) return ctx->fail(MOCAP_E_ARG, "mocap_track_frame_images_jpeg: %s", bad);
    if (!jo->jpeg || !jo->size) return ctx->fail(MOCAP_E_ARG, "mocap_track_frame_images_jpeg: null stream buffer");
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int C = ctx->C, O = o.O_max > 0 ? o.O_max : 1;
  const size_t F = (size_t)n_frames;
  const IoDims n{F, (size_t)K_max, stages.bodies ? (size_t)stages.bodies->B_max : 0, (size_t)ctx->objf_D};
  const size_t n_raw = images ? F * C * (size_t)ctx->img_rows * ctx->img_cols * 3 : 0;
  const size_t j_stride = jo ? ((size_t)jo->capacity + 15) / 16 * 16 : 0;  // slots the export kernel copies 16 bytes at a time
  uint8_t* h_jpeg = nullptr;
  int64_t* h_jsize = nullptr;
  // caller-visible side (pinned host memory): inputs | frame outputs | objects | the stages' arrays
  float* h_blobs;
  int32_t *h_counts, *h_bstat, *h_drone, *h_nobj;
  FrameOut h;
  double *h_pos, *h_head, *h_oerr;
  FilterIO hf{};
  BodiesIO hb{(int)n.B};
  MarkersIO hm{};
  TrackedIO ht{};
  auto lay_host = [&](void* base) {
    Carver c(base);
    h_blobs = c.take<float>(F * C * M_max * 2);
    h_counts = c.take<int32_t>(F * C);
    h_bstat = c.take<int32_t>(F * C);
    h.xyz = c.take<double>(F * K_max * 3);
    h.err = c.take<double>(F * K_max);
    h.corr = c.take<int16_t>(F * K_max * C);
    h.n_out = c.take<int32_t>(F);
    h.status = c.take<int32_t>(F);
    h.n_cand = c.take<int32_t>(F);
    h_pos = c.take<double>(F * O * 3);
    h_head = c.take<double>(F * O);
    h_oerr = c.take<double>(F * O);
    h_drone = c.take<int32_t>(F * O);
    h_nobj = c.take<int32_t>(F);
    if (stages.filter) carve(c, hf, n);
    if (jo) {
      h_jpeg = c.take<uint8_t>(F * j_stride);
      h_jsize = c.take<int64_t>(F);
    }
    if (stages.bodies) carve(c, hb, n);
    if (stages.markers) carve(c, hm, n);
    if (stages.tracked) carve(c, ht, n);
    return c.off;
  };
  const size_t host_total = lay_host(nullptr);
  HIP_TRY(ctx, ctx->live_pin.reserve(host_total, host_total < (size_t)256 * 1024 ? (size_t)256 * 1024 : host_total + host_total / 4,
                                     hipHostMallocDefault));
  lay_host(ctx->live_pin.ptr);
  // device side: [raw images | blobs | counts | blob status |] frame outputs
  uint8_t* d_raw = nullptr;
  float* d_blobs = nullptr;
  int32_t *d_counts = nullptr, *d_bstat = nullptr, *d_jstat = nullptr;
  uint8_t *d_proc = nullptr, *d_jpeg = nullptr;
  int64_t* d_jsize = nullptr;
  FrameOut d;
  auto lay_dev = [&](void* base) {
    Carver c(base);
    if (images) {
      d_raw = c.take<uint8_t>(n_raw);
      d_blobs = c.take<float>(F * C * M_max * 2);
      d_counts = c.take<int32_t>(F * C);
      d_bstat = c.take<int32_t>(F * C);
    }
    d.xyz = c.take<double>(F * K_max * 3);
    d.err = c.take<double>(F * K_max);
    d.corr = c.take<int16_t>(F * K_max * C);
    d.n_out = c.take<int32_t>(F);
    d.status = c.take<int32_t>(F);
    d.n_cand = c.take<int32_t>(F);
    if (jo) {
      d_proc = c.take<uint8_t>(F * C * (size_t)ctx->img_S * ctx->img_S * 3);
      d_jpeg = c.take<uint8_t>(F * j_stride);
      d_jsize = c.take<int64_t>(F);
      d_jstat = c.take<int32_t>(F);
    }
    return c.off;
  };
  const size_t dev_total = lay_dev(nullptr);
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(dev_total)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%zu) failed", dev_total);
  lay_dev(s.ptr);

  if (images) {
    HIP_TRY(ctx, hipMemcpyAsync(d_raw, images, n_raw, hipMemcpyHostToDevice, ctx->stream));
    const int rc = mocap_blob_stage_locked(ctx, n_frames, d_raw, M_max, d_blobs, d_counts, d_bstat, d_proc);
    if (rc) return rc;
  } else {
    memcpy(h_blobs, b.blobs, sizeof(float) * F * C * M_max * 2);
    memcpy(h_counts, b.counts, sizeof(int32_t) * F * C);
  }
  LocateArgs la;
  la.n_frames = n_frames;
  la.K_max = K_max;
  la.O_max = O;
  la.xyz = d.xyz;
  la.err = d.err;
  la.n_pts = d.n_out;
  la.obj_pos = h_pos;
  la.obj_heading = h_head;
  la.obj_err = h_oerr;
  la.obj_drone = h_drone;
  la.obj_lead = nullptr;
  la.n_obj = o.O_max > 0 ? h_nobj : nullptr;
  TrackExportArgs ea;
  memset(&ea, 0, sizeof ea);
  ea.C = C;
  ea.M = M_max;
  ea.corr = d.corr;
  ea.status = d.status;
  ea.n_cand = d.n_cand;
  ea.out_xyz = h.xyz;
  ea.out_err = h.err;
  ea.out_corr = o.pts.corr ? h.corr : nullptr;
  ea.out_n_pts = h.n_out;
  ea.out_status = h.status;
  ea.out_n_cand = h.n_cand;
  if (images) {
    ea.blobs = d_blobs;
    ea.counts = d_counts;
    ea.blob_status = d_bstat;
    ea.out_blobs = h_blobs;
    ea.out_counts = h_counts;
    ea.out_blob_status = h_bstat;
  }
  // the frame kernel reads pinned host memory in place (zero-copy) -- except when the shape goes to the wide variant, which
  // re-reads the blobs for every root batch and candidate view: those are staged into device memory once
  FrameBatch in{n_frames, M_max, images ? d_blobs : h_blobs, images ? d_counts : h_counts, b.gate_px};
  if (!images && plan_frame(ctx, M_max, K_max, 0).wide) {
    float* st_blobs;
    int32_t* st_counts;
    auto lay_stage = [&](void* base) {
      Carver c(base);
      st_blobs = c.take<float>(F * C * M_max * 2);
      st_counts = c.take<int32_t>(F * C);
      return c.off;
    };
    DevBuf& st = ctx->live_stage;
    const size_t st_total = lay_stage(nullptr);
    if (st.reserve(st_total)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%zu) failed", st_total);
    lay_stage(st.ptr);
    HIP_TRY(ctx, hipMemcpyAsync(st_blobs, h_blobs, sizeof(float) * F * C * M_max * 2, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(st_counts, h_counts, sizeof(int32_t) * F * C, hipMemcpyHostToDevice, ctx->stream));
    in.blobs = st_blobs;
    in.counts = st_counts;
  }
  {
    rc = match_dev_locked(ctx, in, K_max, G_cap, d);
    if (rc) return rc;
    // frames that hit a cap (candidates, hit lists, roots): re-run, those frames only, with the largest caps the core has --
    // the reference has none (helpers.py:394-400) -- before the export; queued behind the first pass, no host round trip
    rc = resubmit_dev_locked(ctx, in, K_max, d, nullptr);
    if (rc) return rc;
    // opt-in (point_stages_dev_locked): the export and every stage behind it see the refined, consolidated points
    rc = point_stages_dev_locked(ctx, in, K_max, d);
    if (rc) return rc;
    HIP_TRY(ctx, launch_track_export(la, ea, ctx->stream));
    // the stages read the frame's points where the frame path left them (device memory), the filter the export's objects in
    // the pinned block; time stamps travel through that block, every output lands in it
    if (stages.bodies) rc = bodies_dev_locked(ctx, n_frames, K_max, d.xyz, d.n_out, hb);
    if (!rc && stages.tracked) rc = copy_fields<true>(ht, *stages.tracked, n, HostCopy{});
    if (!rc && stages.tracked) rc = tracked_dev_locked(ctx, n_frames, K_max, d.xyz, d.n_out, hb.B_max, hb.found, hb.assign, ht);
    if (!rc && stages.markers) rc = copy_fields<true>(hm, *stages.markers, n, HostCopy{});
    if (!rc && stages.markers) rc = markers_dev_locked(ctx, n_frames, K_max, d.xyz, d.n_out, hm);
    if (!rc && stages.filter) rc = copy_fields<true>(hf, *stages.filter, n, HostCopy{});
    if (!rc && stages.filter) rc = filter_dev_locked(ctx, n_frames, O, h_pos, h_head, h_drone, h_nobj, hf);
    if (rc) return rc;
    if (jo) {  // encoded in device memory, then the bytes that exist travel into the pinned block 16 at a time
      if (ctx->preview_overlay & kOverlayEpilines) {  // the points' epipolar lines, over the blob stage's own drawings
        rc = epilines_dev_locked(ctx, "mocap_track_frame_images_jpeg", n_frames, ctx->img_S, d_proc, M_max, d_blobs, d_counts, K_max,
                                 d.corr, d.n_out, d.status);
        if (rc) return rc;
      }
      rc = jpeg_dev_locked(ctx, "mocap_track_frame_images_jpeg", n_frames, C, ctx->img_S, ctx->img_S, d_proc, jo->quality, d_jpeg,
                           jo->capacity, d_jsize, d_jstat, (int64_t)j_stride);
      if (rc) return rc;
      HIP_TRY(ctx, launch_jpeg_export(n_frames, d_jpeg, (int64_t)j_stride, d_jsize, jo->capacity, h_jpeg, (int64_t)j_stride, h_jsize, ctx->stream));
    }
    rc = spin_wait(ctx, ctx->live_event);
    if (rc) return rc;
  }
  copy_valid_slots(F, C, K_max, h, o.pts);
  for (size_t f = 0; f < F && o.O_max > 0; f++) {
    o.n_obj[f] = h_nobj[f];
    const size_t no = (size_t)(h_nobj[f] < 0 ? 0 : (h_nobj[f] > o.O_max ? o.O_max : h_nobj[f]));
    memcpy(o.pos + f * O * 3, h_pos + f * O * 3, sizeof(double) * 3 * no);
    memcpy(o.heading + f * O, h_head + f * O, sizeof(double) * no);
    memcpy(o.oerr + f * O, h_oerr + f * O, sizeof(double) * no);
    memcpy(o.drone + f * O, h_drone + f * O, sizeof(int32_t) * no);
  }
  if (stages.filter) copy_fields<false>(*stages.filter, hf, n, HostCopy{});
  if (stages.bodies) copy_fields<false>(*stages.bodies, hb, n, HostCopy{});
  if (stages.markers) copy_fields<false>(*stages.markers, hm, n, HostCopy{});
  if (stages.tracked) copy_fields<false>(*stages.tracked, ht, n, HostCopy{});
  for (size_t f = 0; f < F && jo; f++) {
    jo->size[f] = h_jsize[f];
    memcpy(jo->jpeg + f * (size_t)jo->capacity, h_jpeg + f * j_stride, (size_t)(h_jsize[f] < jo->capacity ? h_jsize[f] : jo->capacity));
  }
  if (images) {
    memcpy(o.counts, h_counts, sizeof(int32_t) * F * C);
    memcpy(o.blob_status, h_bstat, sizeof(int32_t) * F * C);
    for (size_t i = 0; i < F * C; i++) {
      const size_t k = (size_t)(h_counts[i] < 0 ? 0 : (h_counts[i] > M_max ? M_max : h_counts[i]));
      memcpy(o.blobs + i * M_max * 2, h_blobs + i * M_max * 2, sizeof(float) * 2 * k);
    }
  }
  return MOCAP_OK;
}

// The device forms (mocap_track_frame*_dev; `who` names the entry point): the stage's own check first, then frame pass ->
// device-side re-submit of the frames that hit a cap -> object search -> the stage, all queued, nothing waited for.  The
// object search is skipped at O_max = 0 -- except in front of the filter, whose check demands O_max >= 1.
int track_dev_locked(mocap_ctx* ctx, const char* who, const FrameBatch& b, int K_max, int64_t G_cap, const TrackOut& o,
                     const TrackStages& stages) {
  int rc = MOCAP_OK;
  if (stages.filter) rc = filter_check(ctx, who, b.n_frames, o.O_max, *stages.filter);
  if (!rc && stages.tracked) rc = tracked_check(ctx, who, b.n_frames, K_max, stages.bodies->B_max, *stages.tracked);
  if (!rc && stages.bodies) rc = bodies_check(ctx, who, b.n_frames, K_max, *stages.bodies);
  if (!rc && stages.markers) rc = markers_check(ctx, who, b.n_frames, K_max, *stages.markers);
  if (!rc) rc = point_stages_check(ctx, who, b, K_max, o.pts.corr != nullptr);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = match_dev_locked(ctx, b, K_max, G_cap, o.pts);
  if (!rc) rc = resubmit_dev_locked(ctx, b, K_max, o.pts, nullptr);
  if (!rc) rc = point_stages_dev_locked(ctx, b, K_max, o.pts);
  if (!rc && (stages.filter || o.O_max > 0))
    rc = locate_dev_locked(ctx, b.n_frames, K_max, o.pts.xyz, o.pts.err, o.pts.n_out, o.O_max, o.pos, o.heading, o.oerr, o.drone, nullptr, o.n_obj);
  if (!rc && stages.bodies) rc = bodies_dev_locked(ctx, b.n_frames, K_max, o.pts.xyz, o.pts.n_out, *stages.bodies);
  if (!rc && stages.tracked)
    rc = tracked_dev_locked(ctx, b.n_frames, K_max, o.pts.xyz, o.pts.n_out, stages.bodies->B_max, stages.bodies->found,
                            stages.bodies->assign, *stages.tracked);
  if (!rc && stages.markers) rc = markers_dev_locked(ctx, b.n_frames, K_max, o.pts.xyz, o.pts.n_out, *stages.markers);
  if (!rc && stages.filter) rc = filter_dev_locked(ctx, b.n_frames, o.O_max, o.pos, o.heading, o.drone, o.n_obj, *stages.filter);
  return rc ? rc : ctx->mark_enqueued();
}

}  // namespace

extern "C" int mocap_track_frame(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts,
                                 double gate_px, int K_max, int64_t G_cap, double* xyz, double* err, int16_t* corr,
                                 int32_t* n_pts, int32_t* status, int O_max, double* pos, double* heading, double* oerr,
                                 int32_t* drone, int32_t* n_obj) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackOut o{{xyz, err, corr, n_pts, status, nullptr}, O_max, pos, heading, oerr, drone, n_obj};
  return track_locked(ctx, nullptr, FrameBatch{n_frames, M_max, blobs, counts, gate_px}, K_max, G_cap, o);
}

extern "C" int mocap_track_frame_images(mocap_ctx* ctx, int64_t n_frames, const uint8_t* images, int M_max, double gate_px,
                                        int K_max, int64_t G_cap, float* blobs, int32_t* counts, int32_t* blob_status,
                                        double* xyz, double* err, int16_t* corr, int32_t* n_pts, int32_t* status, int O_max,
                                        double* pos, double* heading, double* oerr, int32_t* drone, int32_t* n_obj) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!images) return ctx->fail(MOCAP_E_ARG, "mocap_track_frame_images: null image buffer");
  const TrackOut o{{xyz, err, corr, n_pts, status, nullptr}, O_max, pos, heading, oerr, drone, n_obj, blobs, counts, blob_status};
  return track_locked(ctx, images, FrameBatch{n_frames, M_max, nullptr, nullptr, gate_px}, K_max, G_cap, o);
}

extern "C" int mocap_track_frame_images_jpeg(mocap_ctx* ctx, int64_t n_frames, const uint8_t* images, int M_max, double gate_px,
                                             int K_max, int64_t G_cap, float* blobs, int32_t* counts, int32_t* blob_status,
                                             double* xyz, double* err, int16_t* corr, int32_t* n_pts, int32_t* status, int O_max,
                                             double* pos, double* heading, double* oerr, int32_t* drone, int32_t* n_obj,
                                             int quality, uint8_t* jpeg, int64_t capacity, int64_t* jpeg_size) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!images) return ctx->fail(MOCAP_E_ARG, "mocap_track_frame_images_jpeg: null image buffer");
  const TrackOut o{{xyz, err, corr, n_pts, status, nullptr}, O_max, pos, heading, oerr, drone, n_obj, blobs, counts, blob_status};
  const JpegOut io{quality, jpeg, capacity, jpeg_size};
  return track_locked(ctx, images, FrameBatch{n_frames, M_max, nullptr, nullptr, gate_px}, K_max, G_cap, o, io);
}

extern "C" int mocap_track_frame_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs,
                                     const int32_t* d_counts, double gate_px, int K_max, int64_t G_cap, double* d_xyz,
                                     double* d_err, int16_t* d_corr, int32_t* d_n_pts, int32_t* d_status, int O_max,
                                     double* d_pos, double* d_heading, double* d_oerr, int32_t* d_drone, int32_t* d_n_obj) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackOut o{{d_xyz, d_err, d_corr, d_n_pts, d_status, nullptr}, O_max, d_pos, d_heading, d_oerr, d_drone, d_n_obj};
  return track_dev_locked(ctx, "mocap_track_frame_dev", FrameBatch{n_frames, M_max, d_blobs, d_counts, gate_px}, K_max, G_cap, o, TrackStages{});
}

// mocap_track_frame / mocap_track_frame_dev with the rigid-body stage (csrc/rigid_body.hip) behind the object search
extern "C" int mocap_track_frame_bodies(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts,
                                        double gate_px, int K_max, int64_t G_cap, double* xyz, double* err, int16_t* corr,
                                        int32_t* n_pts, int32_t* status, int O_max, double* pos, double* heading, double* oerr,
                                        int32_t* drone, int32_t* n_obj, int B_max, int32_t* rb_found, int32_t* rb_n_used,
                                        int8_t* rb_assign, double* rb_R, double* rb_t, double* rb_rms, double* rb_score,
                                        int32_t* rb_status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackOut o{{xyz, err, corr, n_pts, status, nullptr}, O_max, pos, heading, oerr, drone, n_obj};
  const BodiesIO io{B_max, rb_found, rb_n_used, rb_assign, rb_R, rb_t, rb_rms, rb_score, rb_status};
  return track_locked(ctx, nullptr, FrameBatch{n_frames, M_max, blobs, counts, gate_px}, K_max, G_cap, o, io);
}

extern "C" int mocap_track_frame_bodies_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs,
                                            const int32_t* d_counts, double gate_px, int K_max, int64_t G_cap, double* d_xyz,
                                            double* d_err, int16_t* d_corr, int32_t* d_n_pts, int32_t* d_status, int O_max,
                                            double* d_pos, double* d_heading, double* d_oerr, int32_t* d_drone, int32_t* d_n_obj,
                                            int B_max, int32_t* d_rb_found, int32_t* d_rb_n_used, int8_t* d_rb_assign,
                                            double* d_rb_R, double* d_rb_t, double* d_rb_rms, double* d_rb_score,
                                            int32_t* d_rb_status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackOut o{{d_xyz, d_err, d_corr, d_n_pts, d_status, nullptr}, O_max, d_pos, d_heading, d_oerr, d_drone, d_n_obj};
  const BodiesIO io{B_max, d_rb_found, d_rb_n_used, d_rb_assign, d_rb_R, d_rb_t, d_rb_rms, d_rb_score, d_rb_status};
  return track_dev_locked(ctx, "mocap_track_frame_bodies_dev", FrameBatch{n_frames, M_max, d_blobs, d_counts, gate_px}, K_max, G_cap, o, io);
}

// mocap_track_frame_bodies / _dev with the body tracker (csrc/body_track.hip) behind the rigid-body stage
extern "C" int mocap_track_frame_bodies_tracked(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts,
                                                double gate_px, int K_max, int64_t G_cap, double* xyz, double* err, int16_t* corr,
                                                int32_t* n_pts, int32_t* status, int O_max, double* pos, double* heading, double* oerr,
                                                int32_t* drone, int32_t* n_obj, int B_max, int32_t* rb_found, int32_t* rb_n_used,
                                                int8_t* rb_assign, double* rb_R, double* rb_t, double* rb_rms, double* rb_score,
                                                int32_t* rb_status, const double* t, int32_t* bt_tracked, int32_t* bt_source,
                                                int32_t* bt_n_used, int8_t* bt_assign, double* bt_R, double* bt_t, double* bt_rms,
                                                int32_t* bt_hits, int32_t* bt_missed, int32_t* bt_status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackOut o{{xyz, err, corr, n_pts, status, nullptr}, O_max, pos, heading, oerr, drone, n_obj};
  const BodiesIO rb{B_max, rb_found, rb_n_used, rb_assign, rb_R, rb_t, rb_rms, rb_score, rb_status};
  const TrackedIO io{t, bt_tracked, bt_source, bt_n_used, bt_assign, bt_R, bt_t, bt_rms, bt_hits, bt_missed, bt_status};
  return track_locked(ctx, nullptr, FrameBatch{n_frames, M_max, blobs, counts, gate_px}, K_max, G_cap, o, TrackStages{rb, io});
}

extern "C" int mocap_track_frame_bodies_tracked_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs,
                                                    const int32_t* d_counts, double gate_px, int K_max, int64_t G_cap, double* d_xyz,
                                                    double* d_err, int16_t* d_corr, int32_t* d_n_pts, int32_t* d_status, int O_max,
                                                    double* d_pos, double* d_heading, double* d_oerr, int32_t* d_drone,
                                                    int32_t* d_n_obj, int B_max, int32_t* d_rb_found, int32_t* d_rb_n_used,
                                                    int8_t* d_rb_assign, double* d_rb_R, double* d_rb_t, double* d_rb_rms,
                                                    double* d_rb_score, int32_t* d_rb_status, const double* d_t, int32_t* d_bt_tracked,
                                                    int32_t* d_bt_source, int32_t* d_bt_n_used, int8_t* d_bt_assign, double* d_bt_R,
                                                    double* d_bt_t, double* d_bt_rms, int32_t* d_bt_hits, int32_t* d_bt_missed,
                                                    int32_t* d_bt_status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackOut o{{d_xyz, d_err, d_corr, d_n_pts, d_status, nullptr}, O_max, d_pos, d_heading, d_oerr, d_drone, d_n_obj};
  const BodiesIO rb{B_max, d_rb_found, d_rb_n_used, d_rb_assign, d_rb_R, d_rb_t, d_rb_rms, d_rb_score, d_rb_status};
  const TrackedIO io{d_t, d_bt_tracked, d_bt_source, d_bt_n_used, d_bt_assign, d_bt_R, d_bt_t, d_bt_rms, d_bt_hits, d_bt_missed,
                     d_bt_status};
  return track_dev_locked(ctx, "mocap_track_frame_bodies_tracked_dev", FrameBatch{n_frames, M_max, d_blobs, d_counts, gate_px}, K_max, G_cap,
                          o, TrackStages{rb, io});
}

// mocap_track_frame / mocap_track_frame_dev with the marker tracker (csrc/marker_track.hip) behind the object search
extern "C" int mocap_track_frame_ids(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts,
                                     double gate_px, int K_max, int64_t G_cap, double* xyz, double* err, int16_t* corr,
                                     int32_t* n_pts, int32_t* status, int O_max, double* pos, double* heading, double* oerr,
                                     int32_t* drone, int32_t* n_obj, const double* t, int32_t* mk_id, int32_t* mk_hits,
                                     int32_t* mk_n_tracks, int32_t* mk_status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackOut o{{xyz, err, corr, n_pts, status, nullptr}, O_max, pos, heading, oerr, drone, n_obj};
  const MarkersIO io{t, mk_id, mk_hits, mk_n_tracks, mk_status};
  return track_locked(ctx, nullptr, FrameBatch{n_frames, M_max, blobs, counts, gate_px}, K_max, G_cap, o, io);
}

extern "C" int mocap_track_frame_ids_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs,
                                         const int32_t* d_counts, double gate_px, int K_max, int64_t G_cap, double* d_xyz,
                                         double* d_err, int16_t* d_corr, int32_t* d_n_pts, int32_t* d_status, int O_max,
                                         double* d_pos, double* d_heading, double* d_oerr, int32_t* d_drone, int32_t* d_n_obj,
                                         const double* d_t, int32_t* d_mk_id, int32_t* d_mk_hits, int32_t* d_mk_n_tracks,
                                         int32_t* d_mk_status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackOut o{{d_xyz, d_err, d_corr, d_n_pts, d_status, nullptr}, O_max, d_pos, d_heading, d_oerr, d_drone, d_n_obj};
  const MarkersIO io{d_t, d_mk_id, d_mk_hits, d_mk_n_tracks, d_mk_status};
  return track_dev_locked(ctx, "mocap_track_frame_ids_dev", FrameBatch{n_frames, M_max, d_blobs, d_counts, gate_px}, K_max, G_cap, o, io);
}

extern "C" int mocap_track_frame_filtered(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts,
                                          double gate_px, int K_max, int64_t G_cap, double* xyz, double* err, int16_t* corr,
                                          int32_t* n_pts, int32_t* status, int O_max, double* pos, double* heading, double* oerr,
                                          int32_t* drone, int32_t* n_obj, const double* t, float* fpos, float* fvel,
                                          double* fheading, int32_t* chosen) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackOut o{{xyz, err, corr, n_pts, status, nullptr}, O_max, pos, heading, oerr, drone, n_obj};
  const FilterIO io{t, fpos, fvel, fheading, chosen};
  return track_locked(ctx, nullptr, FrameBatch{n_frames, M_max, blobs, counts, gate_px}, K_max, G_cap, o, io);
}

extern "C" int mocap_track_frame_filtered_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs,
                                              const int32_t* d_counts, double gate_px, int K_max, int64_t G_cap, double* d_xyz,
                                              double* d_err, int16_t* d_corr, int32_t* d_n_pts, int32_t* d_status, int O_max,
                                              double* d_pos, double* d_heading, double* d_oerr, int32_t* d_drone,
                                              int32_t* d_n_obj, const double* d_t, float* d_fpos, float* d_fvel,
                                              double* d_fheading, int32_t* d_chosen) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackOut o{{d_xyz, d_err, d_corr, d_n_pts, d_status, nullptr}, O_max, d_pos, d_heading, d_oerr, d_drone, d_n_obj};
  const FilterIO io{d_t, d_fpos, d_fvel, d_fheading, d_chosen};
  return track_dev_locked(ctx, "mocap_track_frame_filtered_dev", FrameBatch{n_frames, M_max, d_blobs, d_counts, gate_px}, K_max, G_cap, o, io);
}
