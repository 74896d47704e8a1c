// track_smooth_capi.hip -- the "trajectories" section of include/mocap_core.h: a session's points gathered into one row per marker,
// and the rows smoothed and gap-filled (kernels: track_smooth.hip).  The host forms upload, run and download; the _dev forms read
// the session where it lies.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>

#include "../../include/mocap_core.h"
#include "ctx.hpp"
#include "track_smooth.hpp"

using namespace mocap;

static_assert(kTsMaxRows == MOCAP_TS_MAX_ROWS && kTsMaxHalfWindow == MOCAP_TS_MAX_HALF_WINDOW, "limits");
static_assert(kTsMaxPoints == MOCAP_MT_MAX_POINTS, "K_max is the marker tracker's");

static_assert(kTsSmoothed == MOCAP_TS_SMOOTHED && kTsFilled == MOCAP_TS_FILLED && kTsFew == MOCAP_TS_FEW &&
                  kTsSingular == MOCAP_TS_SINGULAR && kTsBadTime == MOCAP_TS_BAD_TIME,
              "flags");

namespace mocap {

int rows_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int R) {
  if (n_frames < 1) return ctx->fail(MOCAP_E_ARG, "%s: n_frames must be at least 1", who);
  if (R < 1 || R > MOCAP_TS_MAX_ROWS) return ctx->fail(MOCAP_E_ARG, "%s: R must be 1 .. %d", who, MOCAP_TS_MAX_ROWS);
  if (n_frames > ((int64_t)1 << 31) / R) return ctx->fail(MOCAP_E_ARG, "%s: R * n_frames must be at most 2^31", who);
  return MOCAP_OK;
}

int window_check(mocap_ctx* ctx, const char* who, int degree, int W, double span, int n_min, int max_gap) {
  if (degree < 1 || degree > 3) return ctx->fail(MOCAP_E_ARG, "%s: degree must be 1, 2 or 3", who);
  if (W < 1 || W > MOCAP_TS_MAX_HALF_WINDOW) return ctx->fail(MOCAP_E_ARG, "%s: W must be 1 .. %d", who, MOCAP_TS_MAX_HALF_WINDOW);
  if (!(span > 0.0)) return ctx->fail(MOCAP_E_ARG, "%s: span must be > 0 (+inf = none)", who);
  if (n_min < degree + 1 || n_min > 2 * W + 1) return ctx->fail(MOCAP_E_ARG, "%s: n_min must be degree + 1 .. 2 W + 1", who);
  if (max_gap < 0 || max_gap > W) return ctx->fail(MOCAP_E_ARG, "%s: max_gap must be 0 .. W", who);
  return MOCAP_OK;
}

int good_times_locked(mocap_ctx* ctx, const char* ws, int64_t n_frames, const double* t, const uint8_t** good) {
  GoodTimesArgs g{n_frames, t, nullptr, nullptr};
  auto lay = [&](void* base) {
    Carver c(base);
    g.tile_max = c.take<double>((size_t)ts_tiles(n_frames));
    g.good = c.take<uint8_t>((size_t)n_frames);
    return c.off;
  };
  if (ctx->calib_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%s) failed", ws);
  lay(ctx->calib_ws.ptr);
  *good = g.good;
  HIP_TRY(ctx, launch_good_times(g, ctx->stream));
  return MOCAP_OK;
}

}  // namespace mocap

namespace {

int gather_check(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts, const int32_t* id, int n_ids,
                 const int32_t* relabel, int R, const double* traj) {
  const char* who = "mocap_gather_tracks";
  if (int rc = rows_check(ctx, who, n_frames, R)) return rc;
  if (K_max < 1 || K_max > kTsMaxPoints) return ctx->fail(MOCAP_E_ARG, "%s: K_max must be 1 .. 64", who);
  if (n_ids < 1) return ctx->fail(MOCAP_E_ARG, "%s: n_ids must be at least 1", who);
  if (!xyz || !n_pts || !id || !relabel || !traj) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  return MOCAP_OK;
}

int smooth_check(mocap_ctx* ctx, int64_t n_frames, int R, const double* t, const double* traj, int degree, int W, double span,
                 int n_min, int max_gap, const double* pos, const double* vel, const double* acc, const double* res,
                 const int32_t* n_used, const int32_t* flag) {
  const char* who = "mocap_smooth_tracks";
  if (int rc = rows_check(ctx, who, n_frames, R)) return rc;
  if (int rc = window_check(ctx, who, degree, W, span, n_min, max_gap)) return rc;
  if (!t || !traj || !pos || !vel || !acc || !res || !n_used || !flag) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  return MOCAP_OK;
}

// (arguments checked; context lock held by the caller; every pointer device-accessible)
int smooth_dev_locked(mocap_ctx* ctx, SmoothTracksArgs a) {
  if (int rc = good_times_locked(ctx, "trajectory workspace", a.n_frames, a.t, &a.good)) return rc;
  HIP_TRY(ctx, launch_smooth_tracks(a, ctx->stream));
  return MOCAP_OK;
}

}  // namespace

extern "C" int mocap_gather_tracks_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts,
                                       const int32_t* d_id, const int32_t* d_hits, int min_hits, int n_ids, const int32_t* d_relabel,
                                       int R, double* d_traj) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = gather_check(ctx, n_frames, K_max, d_xyz, d_n_pts, d_id, n_ids, d_relabel, R, d_traj)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const GatherTracksArgs a{n_frames, K_max, min_hits, n_ids, R, d_xyz, d_n_pts, d_id, d_hits, d_relabel, d_traj};
  HIP_TRY(ctx, launch_gather_tracks(a, ctx->stream));
  return ctx->mark_enqueued();
}

extern "C" int mocap_gather_tracks(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts,
                                   const int32_t* id, const int32_t* hits, int min_hits, int n_ids, const int32_t* relabel, int R,
                                   double* traj) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = gather_check(ctx, n_frames, K_max, xyz, n_pts, id, n_ids, relabel, R, traj)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, K = (size_t)K_max;
  GatherTracksArgs a{n_frames, K_max, min_hits, n_ids, R, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  auto lay = [&](void* base) {
    Carver c(base);
    a.xyz = c.take<double>(F * K * 3);
    a.n_pts = c.take<int32_t>(F);
    a.id = c.take<int32_t>(F * K);
    a.hits = c.take<int32_t>(F * K);
    a.relabel = c.take<int32_t>((size_t)n_ids);
    a.traj = c.take<double>((size_t)R * F * 3);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  const StreamCopy up{ctx, hipMemcpyHostToDevice};
  if (up((void*)a.xyz, xyz, sizeof(double) * F * K * 3) || up((void*)a.n_pts, n_pts, sizeof(int32_t) * F) ||
      up((void*)a.id, id, sizeof(int32_t) * F * K) || (hits && up((void*)a.hits, hits, sizeof(int32_t) * F * K)) ||
      up((void*)a.relabel, relabel, sizeof(int32_t) * (size_t)n_ids))
    return MOCAP_E_HIP;
  if (!hits) a.hits = nullptr;
  HIP_TRY(ctx, launch_gather_tracks(a, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(traj, a.traj, sizeof(double) * (size_t)R * F * 3, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_smooth_tracks_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_t, const double* d_traj, int degree,
                                       int W, double span, int n_min, int max_gap, double* d_pos, double* d_vel, double* d_acc,
                                       double* d_res, int32_t* d_n_used, int32_t* d_flag) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = smooth_check(ctx, n_frames, R, d_t, d_traj, degree, W, span, n_min, max_gap, d_pos, d_vel, d_acc, d_res, d_n_used, d_flag))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const SmoothTracksArgs a{n_frames, R, degree, W, n_min, max_gap, span, d_t, d_traj, nullptr,
                           d_pos, d_vel, d_acc, d_res, d_n_used, d_flag};
  const int rc = smooth_dev_locked(ctx, a);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_smooth_tracks(mocap_ctx* ctx, int64_t n_frames, int R, const double* t, const double* traj, int degree, int W,
                                   double span, int n_min, int max_gap, double* pos, double* vel, double* acc, double* res,
                                   int32_t* n_used, int32_t* flag) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = smooth_check(ctx, n_frames, R, t, traj, degree, W, span, n_min, max_gap, pos, vel, acc, res, n_used, flag)) return rc;
  bool any_finite = false;
  for (int64_t f = 0; f < n_frames && !any_finite; f++) any_finite = std::isfinite(t[f]);
  if (!any_finite) return ctx->fail(MOCAP_E_ARG, "mocap_smooth_tracks: t has no finite entry");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, N = (size_t)R * F;
  SmoothTracksArgs a{n_frames, R, degree, W, n_min, max_gap, span};
  double *d_t, *d_traj;
  auto lay = [&](void* base) {
    Carver c(base);
    d_t = c.take<double>(F);
    d_traj = c.take<double>(N * 3);
    a.pos = c.take<double>(N * 3);
    a.vel = c.take<double>(N * 3);
    a.acc = c.take<double>(N * 3);
    a.res = c.take<double>(N);
    a.n_used = c.take<int32_t>(N);
    a.flag = c.take<int32_t>(N);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  a.t = d_t;
  a.traj = d_traj;
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if (up(d_t, t, sizeof(double) * F) || up(d_traj, traj, sizeof(double) * N * 3)) return MOCAP_E_HIP;
  if (int rc = smooth_dev_locked(ctx, a)) return rc;
  if (down(pos, a.pos, sizeof(double) * N * 3) || down(vel, a.vel, sizeof(double) * N * 3) || down(acc, a.acc, sizeof(double) * N * 3) ||
      down(res, a.res, sizeof(double) * N) || down(n_used, a.n_used, sizeof(int32_t) * N) || down(flag, a.flag, sizeof(int32_t) * N))
    return MOCAP_E_HIP;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
