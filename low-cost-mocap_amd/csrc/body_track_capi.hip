// body_track_capi.hip -- the "body tracker" section of include/mocap_core.h: set-up, reset, the tracker over a batch's points
// (the per-frame search of rigid_body.hip into context-owned scratch, then the kernel of body_track.hip) and the read-out of
// the slots.  Host runtime only; the one piece of host arithmetic is g2 = gate * gate.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>

#include "../../include/mocap_core.h"
#include "ctx.hpp"

using namespace mocap;

static_assert(BT_SRC_NONE_ == MOCAP_BT_SRC_NONE && BT_SRC_GUIDED_ == MOCAP_BT_SRC_GUIDED && BT_SRC_SEARCH_ == MOCAP_BT_SRC_SEARCH &&
                  BT_SRC_COAST_ == MOCAP_BT_SRC_COAST && BT_ST_BAD_TIME_ == MOCAP_BT_ST_BAD_TIME,
              "kernels.hpp mirrors include/mocap_core.h");

extern "C" int mocap_set_body_tracker(mocap_ctx* ctx, int on, double gate, int max_missed, double vel_alpha) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (on != 0 && on != 1) return ctx->fail(MOCAP_E_ARG, "mocap_set_body_tracker: on=%d is neither 0 nor 1", on);
  if (!on) {  // off: the state and the search scratch are freed once nothing queued reads them any more
    if (ctx->bt_state.ptr || ctx->bt_search.ptr) {
      HIP_TRY(ctx, hipSetDevice(ctx->device));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      for (DevBuf* b : {&ctx->bt_state, &ctx->bt_search}) {
        if (b->ptr) (void)hipFree(b->ptr);
        b->ptr = nullptr;
        b->cap = 0;
      }
    }
    ctx->bt_on = 0;
    return MOCAP_OK;
  }
  if (!std::isfinite(gate) || !(gate > 0.0) || max_missed < 0 || !(vel_alpha >= 0.0 && vel_alpha <= 1.0))
    return ctx->fail(MOCAP_E_ARG, "mocap_set_body_tracker: gate must be finite and > 0, max_missed >= 0, vel_alpha in [0, 1]");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->bt_state.reserve(sizeof(BodyTrackState))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(body tracker state) failed");
  HIP_TRY(ctx, hipMemsetAsync(ctx->bt_state.ptr, 0, sizeof(BodyTrackState), ctx->stream));  // behind everything already queued
  ctx->bt_on = 1;
  ctx->bt_g2 = gate * gate;
  ctx->bt_max_missed = max_missed;
  ctx->bt_alpha = vel_alpha;
  return ctx->mark_enqueued();
}

int tracked_clear_locked(mocap_ctx* ctx) {
  if (!ctx->bt_on) return MOCAP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemsetAsync(ctx->bt_state.ptr, 0, sizeof(BodyTrackState), ctx->stream));
  return ctx->mark_enqueued();
}

extern "C" int mocap_reset_body_tracker(mocap_ctx* ctx) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->bt_on) return ctx->fail(MOCAP_E_ARG, "mocap_reset_body_tracker: mocap_set_body_tracker has not been called");
  return tracked_clear_locked(ctx);
}

int tracked_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int K_max, int B_max, const TrackedIO& io) {
  if (!ctx->bt_on) return ctx->fail(MOCAP_E_ARG, "%s: mocap_set_body_tracker has not been called", who);
  if (n_frames < 0 || K_max < 1 || B_max < 0) return ctx->fail(MOCAP_E_ARG, "%s: bad size argument", who);
  if (K_max > kRbMaxPoints) return ctx->fail(MOCAP_E_ARG, "%s: K_max=%d exceeds the %d points per frame the body tracker takes", who, K_max, kRbMaxPoints);
  if (B_max < ctx->rb_B) return ctx->fail(MOCAP_E_ARG, "%s: B_max=%d is less than the %d registered bodies", who, B_max, ctx->rb_B);
  if (n_frames > 0 && (!io.t || !io.status)) return ctx->fail(MOCAP_E_ARG, "%s: null tracker buffer", who);
  if (n_frames > 0 && B_max > 0 &&
      (!io.tracked || !io.source || !io.n_used || !io.assign || !io.R || !io.p || !io.rms || !io.hits || !io.missed))
    return ctx->fail(MOCAP_E_ARG, "%s: null tracker buffer", who);
  return MOCAP_OK;
}

// (arguments checked by tracked_check; context lock held by the caller; d_rb_*: the search's results for these frames, [F][B_max])
int tracked_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts, int B_max,
                       const int32_t* d_rb_found, const int8_t* d_rb_assign, const TrackedIO& io) {
  if (n_frames == 0) return MOCAP_OK;
  BodyTrackArgs a;
  a.n_frames = n_frames;
  a.K_max = K_max;
  a.B = ctx->rb_B;
  a.B_max = B_max;
  a.max_missed = ctx->bt_max_missed;
  a.g2 = ctx->bt_g2;
  a.vel_alpha = ctx->bt_alpha;
  a.max_rms = ctx->rb_max_rms;
  a.models = (const RigidBodyModel*)ctx->rb_models.ptr;
  a.t = io.t;
  a.xyz = d_xyz;
  a.n_pts = d_n_pts;
  a.rb_found = d_rb_found;
  a.rb_assign = d_rb_assign;
  a.state = (BodyTrackState*)ctx->bt_state.ptr;
  a.tracked = io.tracked;
  a.source = io.source;
  a.n_used = io.n_used;
  a.assign = io.assign;
  a.R = io.R;
  a.p = io.p;
  a.rms = io.rms;
  a.hits = io.hits;
  a.missed = io.missed;
  a.status = io.status;
  HIP_TRY(ctx, launch_body_tracker(a, ctx->stream));
  return MOCAP_OK;
}

namespace {

// the per-frame search into context-owned scratch, then the tracker (both queued on the context's stream)
int search_then_track_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts, int B_max,
                             const TrackedIO& io) {
  const IoDims n{(size_t)n_frames, (size_t)K_max, (size_t)B_max};
  BodiesIO rb{B_max};
  auto lay = [&](void* base) {
    Carver c(base);
    carve(c, rb, n);
    return c.off;
  };
  const size_t need = lay(nullptr);
  if (ctx->bt_search.cap < need) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a grown buffer is a new one: nothing queued may still read the old
    if (ctx->bt_search.reserve(need)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(body tracker search scratch) failed");
  }
  lay(ctx->bt_search.ptr);
  int rc = bodies_dev_locked(ctx, n_frames, K_max, d_xyz, d_n_pts, rb);
  if (!rc) rc = tracked_dev_locked(ctx, n_frames, K_max, d_xyz, d_n_pts, B_max, rb.found, rb.assign, io);
  return rc;
}

}  // namespace

extern "C" int mocap_track_bodies_dev(mocap_ctx* ctx, int64_t n_frames, const double* d_t, int K_max, const double* d_xyz,
                                      const int32_t* d_n_pts, int B_max, int32_t* d_tracked, int32_t* d_source, int32_t* d_n_used,
                                      int8_t* d_assign, double* d_R, double* d_t_pose, double* d_rms, int32_t* d_hits,
                                      int32_t* d_missed, int32_t* d_status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackedIO io{d_t, d_tracked, d_source, d_n_used, d_assign, d_R, d_t_pose, d_rms, d_hits, d_missed, d_status};
  int rc = tracked_check(ctx, "mocap_track_bodies_dev", n_frames, K_max, B_max, io);
  if (rc) return rc;
  if (n_frames == 0) return MOCAP_OK;
  if (!d_xyz || !d_n_pts) return ctx->fail(MOCAP_E_ARG, "mocap_track_bodies_dev: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = search_then_track_locked(ctx, n_frames, K_max, d_xyz, d_n_pts, B_max, io);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_track_bodies(mocap_ctx* ctx, int64_t n_frames, const double* t, int K_max, const double* xyz, const int32_t* n_pts,
                                  int B_max, int32_t* tracked, int32_t* source, int32_t* n_used, int8_t* assign, double* R,
                                  double* t_pose, double* rms, int32_t* hits, int32_t* missed, int32_t* status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const TrackedIO io{t, tracked, source, n_used, assign, R, t_pose, rms, hits, missed, status};
  int rc = tracked_check(ctx, "mocap_track_bodies", n_frames, K_max, B_max, io);
  if (rc) return rc;
  if (n_frames == 0) return MOCAP_OK;
  if (!xyz || !n_pts) return ctx->fail(MOCAP_E_ARG, "mocap_track_bodies: null buffer");
  rc = markers_times_check(ctx, "mocap_track_bodies", n_frames, t);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const IoDims n{(size_t)n_frames, (size_t)K_max, (size_t)B_max};
  double* d_xyz;
  int32_t* d_n;
  TrackedIO d{};
  auto lay = [&](void* base) {
    Carver c(base);
    d_xyz = c.take<double>(n.F * n.K * 3);
    d_n = c.take<int32_t>(n.F);
    carve(c, d, n);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  HIP_TRY(ctx, hipMemcpyAsync(d_xyz, xyz, sizeof(double) * n.F * n.K * 3, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_n, n_pts, sizeof(int32_t) * n.F, hipMemcpyHostToDevice, ctx->stream));
  rc = copy_fields<true>(d, io, n, StreamCopy{ctx, hipMemcpyHostToDevice});
  if (!rc) rc = search_then_track_locked(ctx, n_frames, K_max, d_xyz, d_n, B_max, d);
  if (!rc) rc = copy_fields<false>(io, d, n, StreamCopy{ctx, hipMemcpyDeviceToHost});
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_get_body_tracks(mocap_ctx* ctx, int32_t* live, double* R, double* p, double* v, double* t_seen, int32_t* missed,
                                     int32_t* hits) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->bt_on) return ctx->fail(MOCAP_E_ARG, "mocap_get_body_tracks: mocap_set_body_tracker has not been called");
  if (!live || !R || !p || !v || !t_seen || !missed || !hits) return ctx->fail(MOCAP_E_ARG, "mocap_get_body_tracks: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  BodyTrackState s;
  HIP_TRY(ctx, hipMemcpyAsync(&s, ctx->bt_state.ptr, sizeof s, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int b = 0; b < kRbMaxBodies; b++) {
    live[b] = s.live[b];
    for (int k = 0; k < 9; k++) R[b * 9 + k] = s.R[b][k];
    for (int k = 0; k < 3; k++) {
      p[b * 3 + k] = s.p[b][k];
      v[b * 3 + k] = s.v[b][k];
    }
    t_seen[b] = s.t_seen[b];
    missed[b] = s.missed[b];
    hits[b] = s.hits[b];
  }
  return MOCAP_OK;
}
