// body_learn_capi.hip -- the "rigid-body learning" section of include/mocap_core.h: a body's marker set averaged over a capture
// (kernels: body_learn.hip).  The host form uploads, runs and downloads; the _dev form reads the capture where it lies.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/mocap_core.h"
#include "body_learn.hpp"
#include "ctx.hpp"

using namespace mocap;

static_assert(kLbResult == MOCAP_LB_RESULT, "result layout");

namespace {

int learn_check(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts, const int32_t* id, int N,
                const int32_t* sel, int64_t ref_frame, int iters, double max_rms, const double* result) {
  const char* who = "mocap_learn_rigid_body";
  if (n_frames < 1) return ctx->fail(MOCAP_E_ARG, "%s: n_frames must be at least 1", who);
  if (K_max < 1 || K_max > MOCAP_RB_MAX_POINTS) return ctx->fail(MOCAP_E_ARG, "%s: K_max must be 1 .. 64", who);
  if (N < 3 || N > MOCAP_RB_MAX_MARKERS) return ctx->fail(MOCAP_E_ARG, "%s: a body has 3 .. 8 markers", who);
  if (!xyz || !n_pts || !id || !sel || !result) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  for (int m = 0; m < N; m++) {
    if (sel[m] < 0) return ctx->fail(MOCAP_E_ARG, "%s: sel[%d] is negative", who, m);
    for (int k = 0; k < m; k++)
      if (sel[k] == sel[m]) return ctx->fail(MOCAP_E_ARG, "%s: sel[%d] repeats sel[%d]", who, m, k);
  }
  if (iters < 1 || iters > 16) return ctx->fail(MOCAP_E_ARG, "%s: iters must be 1 .. 16", who);
  if (!(max_rms > 0.0)) return ctx->fail(MOCAP_E_ARG, "%s: max_rms must be > 0 (+inf = no gate)", who);
  if (ref_frame < -1 || ref_frame >= n_frames) return ctx->fail(MOCAP_E_ARG, "%s: ref_frame must be -1 or a frame of the capture", who);
  if (n_frames > ((int64_t)1 << 27)) return ctx->fail(MOCAP_E_LIMIT, "%s: more than 2^27 frames in one call", who);
  return MOCAP_OK;
}

// (arguments checked by learn_check; context lock held by the caller; every pointer but sel device-accessible)
int learn_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts, const int32_t* d_id,
                     const int32_t* d_status, int N, const int32_t* sel, int64_t ref_frame, int iters, double max_rms,
                     double* d_result) {
  BodyLearnArgs a;
  auto lay = [&](void* base) {
    Carver c(base);
    a.slot = c.take<int8_t>((size_t)n_frames * kRbMaxMarkers);
    a.slab = c.take<double>((size_t)calib_partials(n_frames) * kLbSlabDoubles);
    a.state = c.take<BodyLearnState>(1);
    return c.off;
  };
  if (ctx->calib_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(rigid-body learning workspace) failed");
  lay(ctx->calib_ws.ptr);
  a.n_frames = n_frames;
  a.K_max = K_max;
  a.N = N;
  for (int m = 0; m < kRbMaxMarkers; m++) a.sel[m] = m < N ? sel[m] : -1;
  a.ref_frame = ref_frame;
  a.max_rms = max_rms;
  a.xyz = d_xyz;
  a.n_pts = d_n_pts;
  a.id = d_id;
  a.status = d_status;
  a.result = d_result;
  HIP_TRY(ctx, launch_body_learn(a, iters, ctx->stream));
  return MOCAP_OK;
}

}  // namespace

extern "C" int mocap_learn_rigid_body_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts,
                                          const int32_t* d_id, const int32_t* d_status, int N, const int32_t* sel, int64_t ref_frame,
                                          int iters, double max_rms, double* d_result) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = learn_check(ctx, n_frames, K_max, d_xyz, d_n_pts, d_id, N, sel, ref_frame, iters, max_rms, d_result);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = learn_dev_locked(ctx, n_frames, K_max, d_xyz, d_n_pts, d_id, d_status, N, sel, ref_frame, iters, max_rms, d_result);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_learn_rigid_body(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts,
                                      const int32_t* id, const int32_t* status, int N, const int32_t* sel, int64_t ref_frame,
                                      int iters, double max_rms, double* result) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int rc0 = learn_check(ctx, n_frames, K_max, xyz, n_pts, id, N, sel, ref_frame, iters, max_rms, result);
  if (rc0) return rc0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, K = (size_t)K_max;
  double *d_xyz, *d_out;
  int32_t *d_n, *d_id, *d_st;
  auto lay = [&](void* base) {
    Carver c(base);
    d_xyz = c.take<double>(F * K * 3);
    d_n = c.take<int32_t>(F);
    d_id = c.take<int32_t>(F * K);
    d_st = c.take<int32_t>(F);
    d_out = c.take<double>(kLbResult);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  HIP_TRY(ctx, hipMemcpyAsync(d_xyz, xyz, sizeof(double) * F * K * 3, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_n, n_pts, sizeof(int32_t) * F, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_id, id, sizeof(int32_t) * F * K, hipMemcpyHostToDevice, ctx->stream));
  if (status) HIP_TRY(ctx, hipMemcpyAsync(d_st, status, sizeof(int32_t) * F, hipMemcpyHostToDevice, ctx->stream));
  const int rc = learn_dev_locked(ctx, n_frames, K_max, d_xyz, d_n, d_id, status ? d_st : nullptr, N, sel, ref_frame, iters,
                                  max_rms, d_out);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(result, d_out, sizeof(double) * kLbResult, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
