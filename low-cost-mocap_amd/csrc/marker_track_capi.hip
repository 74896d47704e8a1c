// marker_track_capi.hip -- the "marker tracker" section of include/mocap_core.h: set-up, reset, the tracker over a batch's
// points and the read-out of the live tracks (kernel: marker_track.hip).  Host runtime only; the one piece of host
// arithmetic is g2 = gate * gate.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>

#include "../../include/mocap_core.h"
#include "ctx.hpp"

using namespace mocap;

static_assert(kMtMaxTracks == MOCAP_MT_MAX_TRACKS && kMtMaxPoints == MOCAP_MT_MAX_POINTS, "kernels.hpp mirrors include/mocap_core.h");
static_assert(MT_ST_FULL_ == MOCAP_MT_ST_FULL && MT_ST_BAD_TIME_ == MOCAP_MT_ST_BAD_TIME, "kernels.hpp mirrors include/mocap_core.h");

extern "C" int mocap_set_marker_tracker(mocap_ctx* ctx, int T_max, double gate, int max_missed, double vel_alpha) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (T_max < 0 || T_max > kMtMaxTracks) return ctx->fail(MOCAP_E_ARG, "mocap_set_marker_tracker: T_max=%d outside 0 .. %d", T_max, kMtMaxTracks);
  if (T_max == 0) {  // off: the state is freed once nothing queued reads it any more
    if (ctx->mt_state.ptr) {
      HIP_TRY(ctx, hipSetDevice(ctx->device));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      (void)hipFree(ctx->mt_state.ptr);
      ctx->mt_state.ptr = nullptr;
      ctx->mt_state.cap = 0;
    }
    ctx->mt_T = 0;
    return MOCAP_OK;
  }
  if (!std::isfinite(gate) || !(gate > 0.0) || max_missed < 0 || !(vel_alpha >= 0.0 && vel_alpha <= 1.0))
    return ctx->fail(MOCAP_E_ARG, "mocap_set_marker_tracker: gate must be finite and > 0, max_missed >= 0, vel_alpha in [0, 1]");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->mt_state.reserve(sizeof(MarkerTrackState))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(marker tracker state) failed");
  HIP_TRY(ctx, hipMemsetAsync(ctx->mt_state.ptr, 0, sizeof(MarkerTrackState), ctx->stream));  // behind everything already queued
  ctx->mt_T = T_max;
  ctx->mt_g2 = gate * gate;
  ctx->mt_max_missed = max_missed;
  ctx->mt_alpha = vel_alpha;
  return ctx->mark_enqueued();
}

extern "C" int mocap_reset_marker_tracker(mocap_ctx* ctx) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->mt_T) return ctx->fail(MOCAP_E_ARG, "mocap_reset_marker_tracker: mocap_set_marker_tracker has not been called");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemsetAsync(ctx->mt_state.ptr, 0, sizeof(MarkerTrackState), ctx->stream));
  return ctx->mark_enqueued();
}

int markers_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int K_max, const MarkersIO& io) {
  if (!ctx->mt_T) return ctx->fail(MOCAP_E_ARG, "%s: mocap_set_marker_tracker has not been called", who);
  if (n_frames < 0 || K_max < 1) return ctx->fail(MOCAP_E_ARG, "%s: bad size argument", who);
  if (K_max > kMtMaxPoints) return ctx->fail(MOCAP_E_ARG, "%s: K_max=%d exceeds the %d points per frame the marker tracker takes", who, K_max, kMtMaxPoints);
  if (n_frames > 0 && (!io.t || !io.id || !io.hits || !io.n_tracks || !io.status)) return ctx->fail(MOCAP_E_ARG, "%s: null marker buffer", who);
  return MOCAP_OK;
}

int markers_times_check(mocap_ctx* ctx, const char* who, int64_t n_frames, const double* t) {
  for (int64_t f = 0; f < n_frames; f++)
    if (!std::isfinite(t[f])) return ctx->fail(MOCAP_E_ARG, "%s: time stamp %lld is not finite", who, (long long)f);
  return MOCAP_OK;
}

// (arguments checked by markers_check; context lock held by the caller)
int markers_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts, const MarkersIO& io) {
  if (n_frames == 0) return MOCAP_OK;
  MarkerTrackArgs a;
  a.n_frames = n_frames;
  a.K_max = K_max;
  a.T_max = ctx->mt_T;
  a.max_missed = ctx->mt_max_missed;
  a.g2 = ctx->mt_g2;
  a.vel_alpha = ctx->mt_alpha;
  a.t = io.t;
  a.xyz = d_xyz;
  a.n_pts = d_n_pts;
  a.state = (MarkerTrackState*)ctx->mt_state.ptr;
  a.id = io.id;
  a.hits = io.hits;
  a.n_tracks = io.n_tracks;
  a.status = io.status;
  HIP_TRY(ctx, launch_marker_tracker(a, ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_track_markers_dev(mocap_ctx* ctx, int64_t n_frames, const double* d_t, int K_max, const double* d_xyz,
                                       const int32_t* d_n_pts, int32_t* d_id, int32_t* d_hits, int32_t* d_n_tracks,
                                       int32_t* d_status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const MarkersIO io{d_t, d_id, d_hits, d_n_tracks, d_status};
  int rc = markers_check(ctx, "mocap_track_markers_dev", n_frames, K_max, io);
  if (rc) return rc;
  if (n_frames == 0) return MOCAP_OK;
  if (!d_xyz || !d_n_pts) return ctx->fail(MOCAP_E_ARG, "mocap_track_markers_dev: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = markers_dev_locked(ctx, n_frames, K_max, d_xyz, d_n_pts, io);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_track_markers(mocap_ctx* ctx, int64_t n_frames, const double* t, int K_max, const double* xyz,
                                   const int32_t* n_pts, int32_t* id, int32_t* hits, int32_t* n_tracks, int32_t* status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const MarkersIO io{t, id, hits, n_tracks, status};
  int rc = markers_check(ctx, "mocap_track_markers", n_frames, K_max, io);
  if (rc) return rc;
  if (n_frames == 0) return MOCAP_OK;
  if (!xyz || !n_pts) return ctx->fail(MOCAP_E_ARG, "mocap_track_markers: null buffer");
  rc = markers_times_check(ctx, "mocap_track_markers", n_frames, t);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const IoDims n{(size_t)n_frames, (size_t)K_max};
  double* d_xyz;
  int32_t* d_n;
  MarkersIO d{};
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
  if (!rc) rc = markers_dev_locked(ctx, n_frames, K_max, d_xyz, d_n, d);
  if (!rc) rc = copy_fields<false>(io, d, n, StreamCopy{ctx, hipMemcpyDeviceToHost});
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_get_marker_tracks(mocap_ctx* ctx, int32_t* n, int32_t* id, double* pos, double* vel, double* t_seen,
                                       int32_t* missed, int32_t* hits) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->mt_T) return ctx->fail(MOCAP_E_ARG, "mocap_get_marker_tracks: mocap_set_marker_tracker has not been called");
  if (!n || !id || !pos || !vel || !t_seen || !missed || !hits) return ctx->fail(MOCAP_E_ARG, "mocap_get_marker_tracks: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  MarkerTrackState s;
  HIP_TRY(ctx, hipMemcpyAsync(&s, ctx->mt_state.ptr, sizeof s, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  int k = 0;
  for (int i = 0; i < ctx->mt_T; i++) {
    if (!s.live[i]) continue;
    id[k] = s.id[i];
    for (int c = 0; c < 3; c++) {
      pos[k * 3 + c] = s.p[i][c];
      vel[k * 3 + c] = s.v[i][c];
    }
    t_seen[k] = s.t_seen[i];
    missed[k] = s.missed[i];
    hits[k] = s.hits[i];
    k++;
  }
  *n = k;
  return MOCAP_OK;
}
