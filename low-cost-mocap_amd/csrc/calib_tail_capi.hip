// calib_tail_capi.hip -- the "calibration tail" section of include/mocap_core.h: determine-scale and acquire-floor over a
// capture's frame-path outputs (kernels: calib_tail.hip), and the two pieces of host arithmetic behind them: the plane and
// the to-world rotation from the reduced factor (index.py:172-192), and set-origin (index.py:200-207).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <mutex>

#include "../../include/mocap_core.h"
#include "ctx.hpp"

using namespace mocap;

namespace {

int tail_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts,
               const void* out) {
  if (n_frames < 0 || K_max < 1) return ctx->fail(MOCAP_E_ARG, "%s: bad size argument", who);
  if (n_frames > ((int64_t)1 << 27)) return ctx->fail(MOCAP_E_LIMIT, "%s: more than 2^27 frames in one call", who);
  if (!out || (n_frames > 0 && (!xyz || !n_pts))) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  return MOCAP_OK;
}

// (arguments checked by tail_check; context lock held by the caller; every pointer device-accessible)
int tail_dev_locked(mocap_ctx* ctx, bool floor, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts,
                    const int32_t* d_status, double actual_distance, double* d_pair_dist, double* d_out) {
  const size_t slab = sizeof(double) * (size_t)calib_partials(n_frames) * (floor ? kFloorSlabDoubles : kPairSlabDoubles);
  if (ctx->calib_ws.reserve(slab + 256)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(calibration tail partials) failed");
  CalibTailArgs a;
  a.n_frames = n_frames;
  a.K_max = K_max;
  a.xyz = d_xyz;
  a.n_pts = d_n_pts;
  a.status = d_status;
  a.pair_dist = floor ? nullptr : d_pair_dist;
  a.slab = (double*)ctx->calib_ws.ptr;
  HIP_TRY(ctx, floor ? launch_floor_factor(a, d_out, ctx->stream) : launch_pair_scale(a, actual_distance, d_out, ctx->stream));
  return MOCAP_OK;
}

// host form of either entry: copy in, run, copy out, wait
int tail_host(mocap_ctx* ctx, bool floor, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts,
              const int32_t* status, double actual_distance, double* pair_dist, double* out, int n_out) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, K = (size_t)K_max;
  double *d_xyz, *d_pair, *d_out;
  int32_t *d_n, *d_st;
  auto lay = [&](void* base) {
    Carver c(base);
    d_xyz = c.take<double>(F * K * 3);
    d_n = c.take<int32_t>(F);
    d_st = c.take<int32_t>(F);
    d_pair = c.take<double>(F);
    d_out = c.take<double>(17);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  if (F) {
    HIP_TRY(ctx, hipMemcpyAsync(d_xyz, xyz, sizeof(double) * F * K * 3, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_n, n_pts, sizeof(int32_t) * F, hipMemcpyHostToDevice, ctx->stream));
    if (status) HIP_TRY(ctx, hipMemcpyAsync(d_st, status, sizeof(int32_t) * F, hipMemcpyHostToDevice, ctx->stream));
  }
  const int rc = tail_dev_locked(ctx, floor, n_frames, K_max, d_xyz, d_n, status ? d_st : nullptr, actual_distance,
                                 pair_dist ? d_pair : nullptr, d_out);
  if (rc) return rc;
  if (F && pair_dist && !floor)
    HIP_TRY(ctx, hipMemcpyAsync(pair_dist, d_pair, sizeof(double) * F, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(out, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

int host_fail(mocap_ctx* ctx, int code, const char* text) { return ctx ? ctx->fail(code, "%s", text) : code; }

}  // namespace

extern "C" int mocap_determine_scale_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz,
                                         const int32_t* d_n_pts, const int32_t* d_status, double actual_distance,
                                         double* d_pair_dist, double* d_result) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = tail_check(ctx, "mocap_determine_scale", n_frames, K_max, d_xyz, d_n_pts, d_result);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = tail_dev_locked(ctx, false, n_frames, K_max, d_xyz, d_n_pts, d_status, actual_distance, d_pair_dist, d_result);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_determine_scale(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts,
                                     const int32_t* status, double actual_distance, double* pair_dist, double* result) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int rc = tail_check(ctx, "mocap_determine_scale", n_frames, K_max, xyz, n_pts, result);
  if (rc) return rc;
  return tail_host(ctx, false, n_frames, K_max, xyz, n_pts, status, actual_distance, pair_dist, result, 4);
}

extern "C" int mocap_floor_factor_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts,
                                      const int32_t* d_status, double* d_factor) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = tail_check(ctx, "mocap_floor_factor", n_frames, K_max, d_xyz, d_n_pts, d_factor);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = tail_dev_locked(ctx, true, n_frames, K_max, d_xyz, d_n_pts, d_status, 0.0, nullptr, d_factor);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_floor_factor(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts,
                                  const int32_t* status, double* factor) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int rc = tail_check(ctx, "mocap_floor_factor", n_frames, K_max, xyz, n_pts, factor);
  if (rc) return rc;
  return tail_host(ctx, true, n_frames, K_max, xyz, n_pts, status, 0.0, nullptr, factor, 17);
}

extern "C" int mocap_floor_from_factor(mocap_ctx* ctx, const double* factor, double* to_world, double* info) {
  // host-only arithmetic on caller-owned buffers (ctx may be NULL; it only receives the error text)
  if (!factor || !to_world) return host_fail(ctx, MOCAP_E_ARG, "mocap_floor_from_factor: null buffer");
  const double* R = factor;
  const double n = factor[16];
  if (!(n >= 3.0)) return host_fail(ctx, MOCAP_E_ARG, "mocap_floor_from_factor: a plane needs at least 3 points");
  const double d0 = std::fabs(R[0]), d1 = std::fabs(R[5]), d2 = std::fabs(R[10]);
  const double dmax = std::fmax(d0, std::fmax(d1, d2));
  const double tiny = n * DBL_EPSILON * dmax;
  if (!(d0 > tiny) || !(d1 > tiny) || !(d2 > tiny))
    return host_fail(ctx, MOCAP_E_ARG, "mocap_floor_from_factor: the points do not span a plane over x, y (collinear or coincident)");
  // least-squares fit z = a x + b y + c: the 3 x 3 triangle against the first three entries of the last column
  const double c = R[11] / R[10];
  const double b = (R[7] - R[6] * c) / R[5];
  const double a = ((R[3] - R[1] * b) - R[2] * c) / R[0];
  // index.py:175-190, expression by expression
  double pn[3] = {a, b, -1.0};
  const double pn_norm = std::sqrt((pn[0] * pn[0] + pn[1] * pn[1]) + pn[2] * pn[2]);
  for (double& v : pn) v /= pn_norm;
  const double up[3] = {0.0, 0.0, (double)1.0f};  // up_normal (float32 in the reference: exact)
  const double dot = (pn[0] * up[0] + pn[1] * up[1]) + pn[2] * up[2];
  const double cr[3] = {pn[1] * up[2] - pn[2] * up[1], pn[2] * up[0] - pn[0] * up[2], pn[0] * up[1] - pn[1] * up[0]};
  const double sn = std::sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
  const double G[3][3] = {{dot, -sn, 0.0}, {sn, dot, 0.0}, {0.0, 0.0, 1.0}};
  double v[3] = {up[0] - dot * pn[0], up[1] - dot * pn[1], up[2] - dot * pn[2]};
  const double v_norm = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  for (double& x : v) x /= v_norm;
  const double w[3] = {up[1] * pn[2] - up[2] * pn[1], up[2] * pn[0] - up[0] * pn[2], up[0] * pn[1] - up[1] * pn[0]};
  double Fm[3][3];  // columns: plane_normal, v, w
  for (int i = 0; i < 3; i++) {
    Fm[i][0] = pn[i];
    Fm[i][1] = v[i];
    Fm[i][2] = w[i];
  }
  // linalg.inv(F) by cofactors
  double Fi[3][3];
  const double det = Fm[0][0] * (Fm[1][1] * Fm[2][2] - Fm[1][2] * Fm[2][1]) - Fm[0][1] * (Fm[1][0] * Fm[2][2] - Fm[1][2] * Fm[2][0]) +
                     Fm[0][2] * (Fm[1][0] * Fm[2][1] - Fm[1][1] * Fm[2][0]);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
      Fi[i][j] = (Fm[r0][c0] * Fm[r1][c1] - Fm[r0][c1] * Fm[r1][c0]) / det;
    }
  double FG[3][3], Rw[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) FG[i][j] = (Fm[i][0] * G[0][j] + Fm[i][1] * G[1][j]) + Fm[i][2] * G[2][j];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Rw[i][j] = (FG[i][0] * Fi[0][j] + FG[i][1] * Fi[1][j]) + FG[i][2] * Fi[2][j];
  for (int i = 0; i < 3; i++) Rw[i][1] = -Rw[i][1];  // R @ diag(1, -1, 1), index.py:190
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) to_world[4 * i + j] = (i < 3 && j < 3) ? Rw[i][j] : (i == j ? 1.0 : 0.0);
  if (info) {
    info[0] = a;
    info[1] = b;
    info[2] = c;
    info[3] = n;
    info[4] = std::fabs(R[15]) / std::sqrt(n);
    info[5] = std::atan(std::sqrt(a * a + b * b));
  }
  if (!(v_norm >= 1e-8))
    return host_fail(ctx, MOCAP_E_NOCONV,
                     "mocap_floor_from_factor: the floor is parallel to the xy-plane, the reference's rotation is noise-determined "
                     "(|up - (up.n) n| < 1e-8); the matrix was written as the arithmetic gives it");
  return MOCAP_OK;
}

extern "C" int mocap_world_set_origin(mocap_ctx* ctx, const double* to_world_in, const double* point, double* to_world_out) {
  if (!to_world_in || !point || !to_world_out) return host_fail(ctx, MOCAP_E_ARG, "mocap_world_set_origin: null buffer");
  double T[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  T[0][3] = -point[0];
  T[1][3] = -point[2];  // index.py:204: y and z of the point swapped
  T[2][3] = -point[1];
  double out[16];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double acc = T[i][0] * to_world_in[j];
      for (int k = 1; k < 4; k++) acc = acc + T[i][k] * to_world_in[4 * k + j];
      out[4 * i + j] = acc;
    }
  std::memcpy(to_world_out, out, sizeof(out));
  return MOCAP_OK;
}
