// precision_capi.hip -- the "predicted precision" section of include/mocap_core.h: point covariances at given points, at the points
// of a frame batch, and the capture-volume map, with their host forms (kernels: precision.hip).  The argument rules and the fold of
// the caller's coordinates into the per-call table P' are precision_host.hpp's (plain C++, checked under the host sanitizers); the
// table reaches the device as kernel arguments, so a _dev call copies nothing from host memory and never waits.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "../../include/mocap_core.h"
#include "ctx.hpp"
#include "precision.hpp"

using namespace mocap;

static_assert(kPmMaxPoints == MOCAP_PM_MAX_POINTS && kPmMaxVoxels == MOCAP_PM_MAX_VOXELS && kPmSummary == MOCAP_PM_SUMMARY &&
                  kPmSweeps == MOCAP_PM_SWEEPS && kPmMaxDim == MOCAP_PM_MAX_DIM,
              "precision_host.hpp and precision_math.hpp mirror include/mocap_core.h");
static_assert(kPmOk == MOCAP_PM_OK && kPmBadPoint == MOCAP_PM_BAD_POINT && kPmBadView == MOCAP_PM_BAD_VIEW &&
                  kPmFewViews == MOCAP_PM_FEW_VIEWS && kPmDegenerate == MOCAP_PM_DEGENERATE,
              "precision_math.hpp mirrors include/mocap_core.h");
static_assert(kMaxCameras <= 64, "a view mask is 64 bits, the histogram 65 entries");

namespace {

// the rules every entry shares, before anything is written
int common_check(mocap_ctx* ctx, const char* who, double sigma_px, const double* frame) {
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "%s: mocap_set_cameras has not been called", who);
  if (const char* why = pm_common_check(sigma_px, frame)) return ctx->fail(MOCAP_E_ARG, "%s: %s", who, why);
  return MOCAP_OK;
}

// (arguments checked; context lock held) P' folded on the host and put into ctx->pm_tab behind what is queued
int shared_args(mocap_ctx* ctx, double sigma_px, const double* frame, PmArgs& s) {
  const int C = ctx->C;
  if (ctx->pm_tab.reserve(sizeof(double) * 12 * kMaxCameras)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(precision table) failed");
  std::vector<double> tab((size_t)12 * C);
  pm_fold(C, ctx->hPown.data(), frame, tab.data());
  HIP_TRY(ctx, launch_pm_put_table(tab.data(), C, (double*)ctx->pm_tab.ptr, ctx->stream));
  s.C = C;
  s.tab = (const double*)ctx->pm_tab.ptr;
  s.sigma_px = sigma_px;
  return MOCAP_OK;
}

int points_check(mocap_ctx* ctx, const char* who, int64_t N, const double* xyz, const uint64_t* seen, int width, int height, double near,
                 double far, double sigma_px, const double* frame, const double* sig, const int32_t* n_views, const int32_t* info) {
  if (int rc = common_check(ctx, who, sigma_px, frame)) return rc;
  if (const char* why = pm_points_check(N)) return ctx->fail(MOCAP_E_ARG, "%s: %s", who, why);
  if (!seen)
    if (const char* why = pm_vis_check(width, height, near, far)) return ctx->fail(MOCAP_E_ARG, "%s: %s", who, why);
  if (!xyz || !sig || !n_views || !info) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  return MOCAP_OK;
}

int points_dev_locked(mocap_ctx* ctx, int64_t N, const double* d_xyz, const uint64_t* d_seen, int width, int height, double near, double far,
                      double sigma_px, const double* frame, double* d_cov, double* d_sig, double* d_axis, int32_t* d_n_views,
                      int32_t* d_info) {
  PmPointArgs a{};
  if (int rc = shared_args(ctx, sigma_px, frame, a.s)) return rc;
  if (!d_seen) a.s.vis = PmVis{(double)width, (double)height, near, far};
  a.s.cov = d_cov;
  a.s.sig = d_sig;
  a.s.axis = d_axis;
  a.s.n_views = d_n_views;
  a.s.info = d_info;
  a.N = N;
  a.xyz = d_xyz;
  a.seen = d_seen;
  HIP_TRY(ctx, launch_pm_points(a, ctx->stream));
  return MOCAP_OK;
}

int frames_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int K_max, const double* xyz, const int16_t* corr, const int32_t* n_pts,
                 double sigma_px, const double* frame, const double* sig, const int32_t* n_views, const int32_t* info) {
  if (int rc = common_check(ctx, who, sigma_px, frame)) return rc;
  if (const char* why = pm_frames_check(n_frames, K_max)) return ctx->fail(MOCAP_E_ARG, "%s: %s", who, why);
  if (n_frames && (!xyz || !corr || !n_pts || !sig || !n_views || !info)) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  return MOCAP_OK;
}

int frames_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int16_t* d_corr, const int32_t* d_n_pts,
                      const int32_t* d_status, double sigma_px, const double* frame, double* d_cov, double* d_sig, double* d_axis,
                      int32_t* d_n_views, int32_t* d_info) {
  PmFrameArgs a{};
  if (int rc = shared_args(ctx, sigma_px, frame, a.s)) return rc;
  a.s.cov = d_cov;
  a.s.sig = d_sig;
  a.s.axis = d_axis;
  a.s.n_views = d_n_views;
  a.s.info = d_info;
  a.n_frames = n_frames;
  a.K_max = K_max;
  a.xyz = d_xyz;
  a.corr = d_corr;
  a.n_pts = d_n_pts;
  a.status = d_status;
  HIP_TRY(ctx, launch_pm_frames(a, ctx->stream));
  return MOCAP_OK;
}

int map_check(mocap_ctx* ctx, const char* who, int nx, int ny, int nz, const double* origin, const double* e0, const double* e1,
              const double* e2, int width, int height, double near, double far, double sigma_px, const double* frame, int min_views,
              double max_sigma, const uint8_t* n_views, const float* sig_max, const int64_t* summary) {
  if (int rc = common_check(ctx, who, sigma_px, frame)) return rc;
  if (const char* why = pm_map_check(nx, ny, nz, min_views, max_sigma)) return ctx->fail(MOCAP_E_ARG, "%s: %s", who, why);
  if (const char* why = pm_vis_check(width, height, near, far)) return ctx->fail(MOCAP_E_ARG, "%s: %s", who, why);
  if (!origin || !e0 || !e1 || !e2 || !n_views || !sig_max || !summary) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  return MOCAP_OK;
}

int map_dev_locked(mocap_ctx* ctx, int nx, int ny, int nz, const double* origin, const double* e0, const double* e1, const double* e2,
                   int width, int height, double near, double far, double sigma_px, const double* frame, int min_views, double max_sigma,
                   uint8_t* d_n_views, float* d_sig_max, uint64_t* d_seen, int64_t* d_summary) {
  PmMapArgs a{};
  if (int rc = shared_args(ctx, sigma_px, frame, a.s)) return rc;
  a.s.vis = PmVis{(double)width, (double)height, near, far};
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  for (int d = 0; d < 3; d++) {
    a.origin[d] = origin[d];
    a.e0[d] = e0[d];
    a.e1[d] = e1[d];
    a.e2[d] = e2[d];
  }
  a.min_views = min_views;
  a.max_sigma = max_sigma;
  a.n_views = d_n_views;
  a.sig_max = d_sig_max;
  a.seen = d_seen;
  a.summary = (unsigned long long*)d_summary;
  HIP_TRY(ctx, launch_pm_map(a, ctx->stream));
  return MOCAP_OK;
}

}  // namespace

extern "C" void mocap_precision_limits(int* max_points, int64_t* max_voxels, int* summary_len) {
  if (max_points) *max_points = kPmMaxPoints;
  if (max_voxels) *max_voxels = kPmMaxVoxels;
  if (summary_len) *summary_len = kPmSummary;
}

extern "C" int mocap_point_precision_dev(mocap_ctx* ctx, int64_t N, const double* d_xyz, const uint64_t* d_seen, int width, int height,
                                         double near, double far, double sigma_px, const double* frame, double* d_cov, double* d_sig,
                                         double* d_axis, int32_t* d_n_views, int32_t* d_info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = points_check(ctx, "mocap_point_precision_dev", N, d_xyz, d_seen, width, height, near, far, sigma_px, frame, d_sig, d_n_views,
                            d_info))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = points_dev_locked(ctx, N, d_xyz, d_seen, width, height, near, far, sigma_px, frame, d_cov, d_sig, d_axis, d_n_views, d_info);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_point_precision(mocap_ctx* ctx, int64_t N, const double* xyz, const uint64_t* seen, int width, int height, double near,
                                     double far, double sigma_px, const double* frame, double* cov, double* sig, double* axis,
                                     int32_t* n_views, int32_t* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = points_check(ctx, "mocap_point_precision", N, xyz, seen, width, height, near, far, sigma_px, frame, sig, n_views, info))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)N;
  double *d_xyz, *d_cov, *d_sig, *d_axis;
  uint64_t* d_seen;
  int32_t *d_nv, *d_info;
  auto lay = [&](void* base) {
    Carver c(base);
    d_xyz = c.take<double>(n * 3);
    d_cov = c.take<double>(n * 6);
    d_sig = c.take<double>(n * 3);
    d_axis = c.take<double>(n * 3);
    d_seen = c.take<uint64_t>(n);
    d_nv = c.take<int32_t>(n);
    d_info = c.take<int32_t>(n);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  int rc;
  if ((rc = up(d_xyz, xyz, sizeof(double) * n * 3))) return rc;
  if (seen && (rc = up(d_seen, seen, sizeof(uint64_t) * n))) return rc;
  rc = points_dev_locked(ctx, N, d_xyz, seen ? d_seen : nullptr, width, height, near, far, sigma_px, frame, cov ? d_cov : nullptr, d_sig,
                         axis ? d_axis : nullptr, d_nv, d_info);
  if (rc) return rc;
  if (cov && (rc = down(cov, d_cov, sizeof(double) * n * 6))) return rc;
  if (axis && (rc = down(axis, d_axis, sizeof(double) * n * 3))) return rc;
  if ((rc = down(sig, d_sig, sizeof(double) * n * 3)) || (rc = down(n_views, d_nv, sizeof(int32_t) * n)) ||
      (rc = down(info, d_info, sizeof(int32_t) * n)))
    return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_frame_precision_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int16_t* d_corr,
                                         const int32_t* d_n_pts, const int32_t* d_status, double sigma_px, const double* frame,
                                         double* d_cov, double* d_sig, double* d_axis, int32_t* d_n_views, int32_t* d_info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = frames_check(ctx, "mocap_frame_precision_dev", n_frames, K_max, d_xyz, d_corr, d_n_pts, sigma_px, frame, d_sig, d_n_views,
                            d_info))
    return rc;
  if (n_frames == 0) return MOCAP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = frames_dev_locked(ctx, n_frames, K_max, d_xyz, d_corr, d_n_pts, d_status, sigma_px, frame, d_cov, d_sig, d_axis, d_n_views,
                                   d_info);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_frame_precision(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int16_t* corr,
                                     const int32_t* n_pts, const int32_t* status, double sigma_px, const double* frame, double* cov,
                                     double* sig, double* axis, int32_t* n_views, int32_t* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = frames_check(ctx, "mocap_frame_precision", n_frames, K_max, xyz, corr, n_pts, sigma_px, frame, sig, n_views, info)) return rc;
  if (n_frames == 0) return MOCAP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, n = F * (size_t)K_max, C = (size_t)ctx->C;
  double *d_xyz, *d_cov, *d_sig, *d_axis;
  int16_t* d_corr;
  int32_t *d_n, *d_st, *d_nv, *d_info;
  auto lay = [&](void* base) {
    Carver c(base);
    d_xyz = c.take<double>(n * 3);
    d_cov = c.take<double>(n * 6);
    d_sig = c.take<double>(n * 3);
    d_axis = c.take<double>(n * 3);
    d_corr = c.take<int16_t>(n * C);
    d_n = c.take<int32_t>(F);
    d_st = c.take<int32_t>(F);
    d_nv = c.take<int32_t>(n);
    d_info = c.take<int32_t>(n);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  int rc;
  if ((rc = up(d_xyz, xyz, sizeof(double) * n * 3)) || (rc = up(d_corr, corr, sizeof(int16_t) * n * C)) ||
      (rc = up(d_n, n_pts, sizeof(int32_t) * F)))
    return rc;
  if (status && (rc = up(d_st, status, sizeof(int32_t) * F))) return rc;
  rc = frames_dev_locked(ctx, n_frames, K_max, d_xyz, d_corr, d_n, status ? d_st : nullptr, sigma_px, frame, cov ? d_cov : nullptr, d_sig,
                         axis ? d_axis : nullptr, d_nv, d_info);
  if (rc) return rc;
  if (cov && (rc = down(cov, d_cov, sizeof(double) * n * 6))) return rc;
  if (axis && (rc = down(axis, d_axis, sizeof(double) * n * 3))) return rc;
  if ((rc = down(sig, d_sig, sizeof(double) * n * 3)) || (rc = down(n_views, d_nv, sizeof(int32_t) * n)) ||
      (rc = down(info, d_info, sizeof(int32_t) * n)))
    return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_coverage_map_dev(mocap_ctx* ctx, int nx, int ny, int nz, const double* origin, const double* e0, const double* e1,
                                      const double* e2, int width, int height, double near, double far, double sigma_px,
                                      const double* frame, int min_views, double max_sigma, uint8_t* d_n_views, float* d_sig_max,
                                      uint64_t* d_seen, int64_t* d_summary) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = map_check(ctx, "mocap_coverage_map_dev", nx, ny, nz, origin, e0, e1, e2, width, height, near, far, sigma_px, frame, min_views,
                         max_sigma, d_n_views, d_sig_max, d_summary))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = map_dev_locked(ctx, nx, ny, nz, origin, e0, e1, e2, width, height, near, far, sigma_px, frame, min_views, max_sigma,
                                d_n_views, d_sig_max, d_seen, d_summary);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_coverage_map(mocap_ctx* ctx, int nx, int ny, int nz, const double* origin, const double* e0, const double* e1,
                                  const double* e2, int width, int height, double near, double far, double sigma_px, const double* frame,
                                  int min_views, double max_sigma, uint8_t* n_views, float* sig_max, uint64_t* seen, int64_t* summary) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = map_check(ctx, "mocap_coverage_map", nx, ny, nz, origin, e0, e1, e2, width, height, near, far, sigma_px, frame, min_views,
                         max_sigma, n_views, sig_max, summary))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)nx * ny * nz;
  uint8_t* d_nv;
  float* d_sm;
  uint64_t* d_seen;
  int64_t* d_sum;
  auto lay = [&](void* base) {
    Carver c(base);
    d_seen = c.take<uint64_t>(seen ? n : 0);
    d_sum = c.take<int64_t>(kPmSummary);
    d_sm = c.take<float>(n);
    d_nv = c.take<uint8_t>(n);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  const StreamCopy down{ctx, hipMemcpyDeviceToHost};
  int rc = map_dev_locked(ctx, nx, ny, nz, origin, e0, e1, e2, width, height, near, far, sigma_px, frame, min_views, max_sigma, d_nv, d_sm,
                          seen ? d_seen : nullptr, d_sum);
  if (rc) return rc;
  if ((rc = down(n_views, d_nv, n)) || (rc = down(sig_max, d_sm, sizeof(float) * n)) ||
      (rc = down(summary, d_sum, sizeof(int64_t) * kPmSummary)))
    return rc;
  if (seen && (rc = down(seen, d_seen, sizeof(uint64_t) * n))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
