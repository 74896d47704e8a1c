// point_refine_capi.hip -- the "point refinement" section of include/mocap_core.h: the mode of the live loop, the staged call on
// the frame path's arrays, the observation form, and their host forms (kernel: point_refine.hip).  Host runtime only, no arithmetic.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/mocap_core.h"
#include "ctx.hpp"
#include "refine_lm.hpp"

using namespace mocap;

static_assert(kRefineMaxIters == MOCAP_REFINE_MAX_ITERS, "refine_lm.hpp mirrors include/mocap_core.h");
static_assert(kRfRefined == MOCAP_RF_REFINED && kRfFewViews == MOCAP_RF_FEW_VIEWS && kRfBadIndex == MOCAP_RF_BAD_INDEX &&
                  kRfBadObs == MOCAP_RF_BAD_OBS && kRfBadStart == MOCAP_RF_BAD_START && kRfStepsShift == MOCAP_RF_STEPS_SHIFT,
              "refine_lm.hpp mirrors include/mocap_core.h");

extern "C" int mocap_set_point_refinement(mocap_ctx* ctx, int iters) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (iters < 0 || iters > kRefineMaxIters)
    return ctx->fail(MOCAP_E_ARG, "mocap_set_point_refinement: iters=%d outside 0 .. %d", iters, kRefineMaxIters);
  ctx->refine_iters = iters;
  return MOCAP_OK;
}

int refine_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int M_max, int K_max, int iters) {
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "%s: mocap_set_cameras has not been called", who);
  if (n_frames < 0 || n_frames > 0x7fffffffll || M_max < 1 || K_max < 1) return ctx->fail(MOCAP_E_ARG, "%s: bad size argument", who);
  if (iters < 1 || iters > kRefineMaxIters) return ctx->fail(MOCAP_E_ARG, "%s: iters=%d outside 1 .. %d", who, iters, kRefineMaxIters);
  return MOCAP_OK;
}

static RefineArgs refine_args(mocap_ctx* ctx, int iters) {
  RefineArgs a{};
  a.cv = ctx->cv;
  a.P = ctx->d_Pown;
  a.iters = iters;
  return a;
}

// (arguments checked by refine_check, the arrays non-null; context lock held by the caller)
int refine_dev_locked(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs, const int32_t* d_counts, int K_max, int iters,
                      double* d_xyz, double* d_err, const int16_t* d_corr, const int32_t* d_n_pts, const int32_t* d_status,
                      int32_t* d_info) {
  if (n_frames == 0) return MOCAP_OK;
  RefineArgs a = refine_args(ctx, iters);
  a.n_frames = n_frames;
  a.M = M_max;
  a.K_max = K_max;
  a.blobs = d_blobs;
  a.counts = d_counts;
  a.corr = d_corr;
  a.n_pts = d_n_pts;
  a.status = d_status;
  a.world = ctx->world_on ? (const double*)ctx->world.ptr : nullptr;
  a.xyz = d_xyz;
  a.err = d_err;
  a.info = d_info;
  HIP_TRY(ctx, launch_point_refine(a, ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_refine_points_dev(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* d_blobs, const int32_t* d_counts,
                                       int K_max, int iters, double* d_xyz, double* d_err, const int16_t* d_corr,
                                       const int32_t* d_n_pts, const int32_t* d_status, int32_t* d_info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = refine_check(ctx, "mocap_refine_points_dev", n_frames, M_max, K_max, iters);
  if (rc) return rc;
  if (n_frames == 0) return MOCAP_OK;
  if (!d_blobs || !d_counts || !d_xyz || !d_err || !d_corr || !d_n_pts) return ctx->fail(MOCAP_E_ARG, "mocap_refine_points_dev: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = refine_dev_locked(ctx, n_frames, M_max, d_blobs, d_counts, K_max, iters, d_xyz, d_err, d_corr, d_n_pts, d_status, d_info);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_refine_points(mocap_ctx* ctx, int64_t n_frames, int M_max, const float* blobs, const int32_t* counts, int K_max,
                                   int iters, double* xyz, double* err, const int16_t* corr, const int32_t* n_pts,
                                   const int32_t* status, int32_t* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = refine_check(ctx, "mocap_refine_points", n_frames, M_max, K_max, iters);
  if (rc) return rc;
  if (n_frames == 0) return MOCAP_OK;
  if (!blobs || !counts || !xyz || !err || !corr || !n_pts) return ctx->fail(MOCAP_E_ARG, "mocap_refine_points: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, K = (size_t)K_max, C = (size_t)ctx->C, M = (size_t)M_max;
  float* d_blobs;
  double *d_xyz, *d_err;
  int16_t* d_corr;
  int32_t *d_counts, *d_n, *d_st, *d_info;
  auto lay = [&](void* base) {
    Carver c(base);
    d_xyz = c.take<double>(F * K * 3);
    d_err = c.take<double>(F * K);
    d_blobs = c.take<float>(F * C * M * 2);
    d_corr = c.take<int16_t>(F * K * C);
    d_counts = c.take<int32_t>(F * C);
    d_n = c.take<int32_t>(F);
    d_st = c.take<int32_t>(F);
    d_info = c.take<int32_t>(F * K);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  // xyz and err travel both ways whole: what the kernel leaves alone comes back as it went
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if ((rc = up(d_xyz, xyz, sizeof(double) * F * K * 3)) || (rc = up(d_err, err, sizeof(double) * F * K)) ||
      (rc = up(d_blobs, blobs, sizeof(float) * F * C * M * 2)) || (rc = up(d_corr, corr, sizeof(int16_t) * F * K * C)) ||
      (rc = up(d_counts, counts, sizeof(int32_t) * F * C)) || (rc = up(d_n, n_pts, sizeof(int32_t) * F)))
    return rc;
  if (status && (rc = up(d_st, status, sizeof(int32_t) * F))) return rc;
  rc = refine_dev_locked(ctx, n_frames, M_max, d_blobs, d_counts, K_max, iters, d_xyz, d_err, d_corr, d_n, status ? d_st : nullptr,
                         info ? d_info : nullptr);
  if (rc) return rc;
  if ((rc = down(xyz, d_xyz, sizeof(double) * F * K * 3)) || (rc = down(err, d_err, sizeof(double) * F * K))) return rc;
  if (info && (rc = down(info, d_info, sizeof(int32_t) * F * K))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

static int triangulate_refined_check(mocap_ctx* ctx, const char* who, int64_t N, int iters) {
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "%s: mocap_set_cameras has not been called", who);
  if (N < 0) return ctx->fail(MOCAP_E_ARG, "%s: bad size argument", who);
  if (iters < 1 || iters > kRefineMaxIters) return ctx->fail(MOCAP_E_ARG, "%s: iters=%d outside 1 .. %d", who, iters, kRefineMaxIters);
  return MOCAP_OK;
}

static int triangulate_refined_dev_locked(mocap_ctx* ctx, int64_t N, const double* d_obs, int iters, double* d_xyz, double* d_err,
                                          int32_t* d_info) {
  RefineArgs a = refine_args(ctx, iters);
  a.N = N;
  a.obs = d_obs;
  a.xyz = d_xyz;
  a.err = d_err;
  a.info = d_info;
  HIP_TRY(ctx, launch_point_refine(a, ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_triangulate_refined_dev(mocap_ctx* ctx, int64_t N, const double* d_obs, int iters, double* d_xyz, double* d_err,
                                             int32_t* d_info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = triangulate_refined_check(ctx, "mocap_triangulate_refined_dev", N, iters);
  if (rc) return rc;
  if (N == 0) return MOCAP_OK;
  if (!d_obs || !d_xyz) return ctx->fail(MOCAP_E_ARG, "mocap_triangulate_refined_dev: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = triangulate_refined_dev_locked(ctx, N, d_obs, iters, d_xyz, d_err, d_info);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_triangulate_refined(mocap_ctx* ctx, int64_t N, const double* obs, int iters, double* xyz, double* err,
                                         int32_t* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = triangulate_refined_check(ctx, "mocap_triangulate_refined", N, iters);
  if (rc) return rc;
  if (N == 0) return MOCAP_OK;
  if (!obs || !xyz) return ctx->fail(MOCAP_E_ARG, "mocap_triangulate_refined: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)N, C = (size_t)ctx->C;
  double *d_obs, *d_xyz, *d_err;
  int32_t* d_info;
  auto lay = [&](void* base) {
    Carver c(base);
    d_obs = c.take<double>(n * C * 2);
    d_xyz = c.take<double>(n * 3);
    d_err = c.take<double>(n);
    d_info = c.take<int32_t>(n);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if ((rc = up(d_obs, obs, sizeof(double) * n * C * 2))) return rc;
  rc = triangulate_refined_dev_locked(ctx, N, d_obs, iters, d_xyz, err ? d_err : nullptr, info ? d_info : nullptr);
  if (rc) return rc;
  if ((rc = down(xyz, d_xyz, sizeof(double) * n * 3))) return rc;
  if (err && (rc = down(err, d_err, sizeof(double) * n))) return rc;
  if (info && (rc = down(info, d_info, sizeof(int32_t) * n))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
