// point_consolidate_capi.hip -- the "point consolidation" section of include/mocap_core.h: the mode of the live loop, the staged
// call on device arrays and its host form (kernel: point_consolidate.hip).  Host runtime only, no arithmetic.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/mocap_core.h"
#include "ctx.hpp"

using namespace mocap;

static_assert(kPcMaxPoints == MOCAP_PC_MAX_POINTS, "kernels.hpp mirrors include/mocap_core.h");
static_assert(kPcStatusSkip == (MOCAP_ST_ROOT_OVERFLOW | MOCAP_ST_CAND_OVERFLOW | MOCAP_ST_HIT_OVERFLOW), "kernels.hpp mirrors include/mocap_core.h");

extern "C" int mocap_set_point_consolidation(mocap_ctx* ctx, int mode) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (mode != MOCAP_CONSOLIDATE_OFF && mode != MOCAP_CONSOLIDATE_BLOBS)
    return ctx->fail(MOCAP_E_ARG, "mocap_set_point_consolidation: unknown mode %d", mode);
  ctx->consolidate = mode;
  return MOCAP_OK;
}

int consolidate_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int K_max) {
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "%s: mocap_set_cameras has not been called", who);
  if (n_frames < 0 || n_frames > 0x7fffffffll || K_max < 1) return ctx->fail(MOCAP_E_ARG, "%s: bad size argument", who);
  if (K_max > kPcMaxPoints) return ctx->fail(MOCAP_E_LIMIT, "%s: K_max=%d exceeds the %d points per frame the consolidation takes", who, K_max, kPcMaxPoints);
  return MOCAP_OK;
}

// (arguments checked by consolidate_check, the arrays non-null; context lock held by the caller)
int consolidate_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, double* d_xyz, double* d_err, int16_t* d_corr, int32_t* d_n_pts,
                           const int32_t* d_status, int32_t* d_src, int32_t* d_n_in) {
  if (n_frames == 0) return MOCAP_OK;
  ConsolidateArgs a;
  a.n_frames = n_frames;
  a.C = ctx->C;
  a.K_max = K_max;
  a.xyz = d_xyz;
  a.err = d_err;
  a.corr = d_corr;
  a.n_pts = d_n_pts;
  a.status = d_status;
  a.src = d_src;
  a.n_in = d_n_in;
  HIP_TRY(ctx, launch_point_consolidate(a, ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_consolidate_points_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, double* d_xyz, double* d_err, int16_t* d_corr,
                                            int32_t* d_n_pts, const int32_t* d_status, int32_t* d_src, int32_t* d_n_in) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = consolidate_check(ctx, "mocap_consolidate_points_dev", n_frames, K_max);
  if (rc) return rc;
  if (n_frames == 0) return MOCAP_OK;
  if (!d_xyz || !d_err || !d_corr || !d_n_pts) return ctx->fail(MOCAP_E_ARG, "mocap_consolidate_points_dev: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = consolidate_dev_locked(ctx, n_frames, K_max, d_xyz, d_err, d_corr, d_n_pts, d_status, d_src, d_n_in);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_consolidate_points(mocap_ctx* ctx, int64_t n_frames, int K_max, double* xyz, double* err, int16_t* corr,
                                        int32_t* n_pts, const int32_t* status, int32_t* src, int32_t* n_in) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = consolidate_check(ctx, "mocap_consolidate_points", n_frames, K_max);
  if (rc) return rc;
  if (n_frames == 0) return MOCAP_OK;
  if (!xyz || !err || !corr || !n_pts) return ctx->fail(MOCAP_E_ARG, "mocap_consolidate_points: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, K = (size_t)K_max, C = (size_t)ctx->C;
  double *d_xyz, *d_err;
  int16_t* d_corr;
  int32_t *d_n, *d_st, *d_src, *d_nin;
  auto lay = [&](void* base) {
    Carver c(base);
    d_xyz = c.take<double>(F * K * 3);
    d_err = c.take<double>(F * K);
    d_corr = c.take<int16_t>(F * K * C);
    d_n = c.take<int32_t>(F);
    d_st = c.take<int32_t>(F);
    d_src = c.take<int32_t>(F * K);
    d_nin = c.take<int32_t>(F);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  // every array travels both ways whole: what the kernel leaves alone (unprocessed frames, the slots from the new count on) comes
  // back as it went
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if ((rc = up(d_xyz, xyz, sizeof(double) * F * K * 3)) || (rc = up(d_err, err, sizeof(double) * F * K)) ||
      (rc = up(d_corr, corr, sizeof(int16_t) * F * K * C)) || (rc = up(d_n, n_pts, sizeof(int32_t) * F)))
    return rc;
  if (status && (rc = up(d_st, status, sizeof(int32_t) * F))) return rc;
  if (src && (rc = up(d_src, src, sizeof(int32_t) * F * K))) return rc;
  rc = consolidate_dev_locked(ctx, n_frames, K_max, d_xyz, d_err, d_corr, d_n, status ? d_st : nullptr, src ? d_src : nullptr,
                              n_in ? d_nin : nullptr);
  if (rc) return rc;
  if ((rc = down(xyz, d_xyz, sizeof(double) * F * K * 3)) || (rc = down(err, d_err, sizeof(double) * F * K)) ||
      (rc = down(corr, d_corr, sizeof(int16_t) * F * K * C)) || (rc = down(n_pts, d_n, sizeof(int32_t) * F)))
    return rc;
  if (src && (rc = down(src, d_src, sizeof(int32_t) * F * K))) return rc;
  if (n_in && (rc = down(n_in, d_nin, sizeof(int32_t) * F))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
