// body_session_capi.hip -- the "body trajectories" section of include/mocap_core.h: the poses of a session's bodies from their
// labelled rows, the rotations smoothed, and the rows filled rigidly (kernels: body_session.hip).  The host forms upload, run and
// download; the _dev forms read the session where it lies.  The body description (n_markers, rows, markers) is host memory in
// both forms: it is checked and tabulated here, and travels to the device inside kernel arguments.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/mocap_core.h"
#include "body_session.hpp"
#include "ctx.hpp"
#include "span_rule.hpp"

using namespace mocap;

static_assert(kBpMaxBodies == MOCAP_BP_MAX_BODIES && kBpMaxMarkers == MOCAP_RB_MAX_MARKERS, "limits");
static_assert(kBpPosed == MOCAP_BP_POSED && kBpFew == MOCAP_BP_FEW && kBpDegenerate == MOCAP_BP_DEGENERATE && kBpRms == MOCAP_BP_RMS, "flags");
static_assert(kBpSrcNone == MOCAP_BP_SRC_NONE && kBpSrcMeasured == MOCAP_BP_SRC_MEASURED && kBpSrcRigid == MOCAP_BP_SRC_RIGID &&
                  kBpSrcRigidFilled == MOCAP_BP_SRC_RIGID_FILLED,
              "sources");

namespace {

// bit s of the mask: the marker subset s holds a spanning triple (so it has >= 3 markers)
void posable_mask(int n, const double (*q)[3], unsigned long long mask[4]) {
  mask[0] = mask[1] = mask[2] = mask[3] = 0;
  unsigned char triple[kBpMaxMarkers][kBpMaxMarkers][kBpMaxMarkers];
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++)
      for (int k = j + 1; k < n; k++) triple[i][j][k] = triple_spans(q[i], q[j], q[k]) ? 1 : 0;
  for (unsigned s = 0; s < (1u << n); s++) {
    bool ok = false;
    for (int i = 0; i < n && !ok; i++)
      for (int j = i + 1; j < n && !ok; j++)
        for (int k = j + 1; k < n && !ok; k++) ok = (s >> i & 1) && (s >> j & 1) && (s >> k & 1) && triple[i][j][k];
    if (ok) mask[s >> 6] |= 1ull << (s & 63);
  }
}

}  // namespace

// the common body description, checked and tabulated ("joint poses" takes its bodies through it too: body_session.hpp)
int mocap::bodies_table(mocap_ctx* ctx, const char* who, int R, int B, const int32_t* n_markers, const int32_t* rows,
                        const double* markers, std::vector<BpBody>& table) {
  if (B < 1 || B > kBpMaxBodies) return ctx->fail(MOCAP_E_ARG, "%s: B=%d outside 1 .. %d", who, B, kBpMaxBodies);
  if (!n_markers || !rows || !markers) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  table.assign((size_t)B, BpBody{});
  std::vector<unsigned char> taken((size_t)R, 0);
  for (int b = 0; b < B; b++) {
    BpBody& m = table[(size_t)b];
    const int n = n_markers[b];
    if (n < 3 || n > kBpMaxMarkers) return ctx->fail(MOCAP_E_ARG, "%s: body %d has %d markers (3 .. %d)", who, b, n, kBpMaxMarkers);
    m.n = n;
    for (int i = 0; i < kBpMaxMarkers; i++) m.rows[i] = -1;
    for (int i = 0; i < n; i++) {
      const int32_t r = rows[(size_t)b * kBpMaxMarkers + i];
      if (r < 0 || r >= R) return ctx->fail(MOCAP_E_ARG, "%s: body %d, marker %d: row %d outside 0 .. %d", who, b, i, r, R - 1);
      if (taken[(size_t)r]) return ctx->fail(MOCAP_E_ARG, "%s: body %d, marker %d: row %d is used twice", who, b, i, r);
      taken[(size_t)r] = 1;
      m.rows[i] = r;
      for (int k = 0; k < 3; k++) {
        const double v = markers[((size_t)b * kBpMaxMarkers + i) * 3 + k];
        if (!std::isfinite(v)) return ctx->fail(MOCAP_E_ARG, "%s: body %d, marker %d: non-finite coordinate", who, b, i);
        m.q[i][k] = v;
      }
    }
    posable_mask(n, m.q, m.posable);
    const unsigned full = (1u << n) - 1;
    if (!((m.posable[full >> 6] >> (full & 63)) & 1ull))
      return ctx->fail(MOCAP_E_ARG, "%s: body %d is not posable (its markers are collinear)", who, b);
  }
  return MOCAP_OK;
}

namespace {

int pose_check(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, double max_rms, const int32_t* n_used,
               const int32_t* present, const double* quat, const double* Rm, const double* t_pose, const double* rms,
               const int32_t* flag) {
  const char* who = "mocap_pose_rows";
  if (int rc = rows_check(ctx, who, n_frames, R)) return rc;
  if (!(max_rms > 0.0)) return ctx->fail(MOCAP_E_ARG, "%s: max_rms must be > 0 (+inf = any)", who);
  if (!traj || !n_used || !present || !quat || !Rm || !t_pose || !rms || !flag) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  return MOCAP_OK;
}

// (arguments checked; context lock held by the caller; every pointer of `a` device-accessible)
int pose_dev_locked(mocap_ctx* ctx, PoseRowsArgs a, const std::vector<BpBody>& table) {
  const size_t F = (size_t)a.n_frames, B = (size_t)a.B;
  BpBody* d_bodies;
  auto lay = [&](void* base) {
    Carver c(base);
    d_bodies = c.take<BpBody>(B);
    a.tile_i32 = c.take<int32_t>(B * (size_t)ts_tiles(a.n_frames));
    a.parity = c.take<uint8_t>(B * F);
    return c.off;
  };
  if (ctx->calib_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(body trajectories workspace) failed");
  lay(ctx->calib_ws.ptr);
  a.bodies = d_bodies;
  HIP_TRY(ctx, launch_put_bodies(table.data(), a.B, d_bodies, ctx->stream));
  HIP_TRY(ctx, launch_pose_rows(a, ctx->stream));
  return MOCAP_OK;
}

int rot_check(mocap_ctx* ctx, int64_t n_frames, int B, const double* t, const double* quat, int degree, int W, double span, int n_min,
              int max_gap, const double* quat_s, const double* omega, const double* res, const int32_t* n_used, const int32_t* flag) {
  const char* who = "mocap_smooth_rotations";
  if (n_frames < 1) return ctx->fail(MOCAP_E_ARG, "%s: n_frames must be at least 1", who);
  if (B < 1 || B > kBpMaxBodies) return ctx->fail(MOCAP_E_ARG, "%s: B must be 1 .. %d", who, kBpMaxBodies);
  if (n_frames > ((int64_t)1 << 31) / B) return ctx->fail(MOCAP_E_ARG, "%s: B * n_frames must be at most 2^31", who);
  if (int rc = window_check(ctx, who, degree, W, span, n_min, max_gap)) return rc;
  if (!t || !quat || !quat_s || !omega || !res || !n_used || !flag) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  return MOCAP_OK;
}

int rot_dev_locked(mocap_ctx* ctx, SmoothRotationsArgs a) {
  if (int rc = good_times_locked(ctx, "body trajectories workspace", a.n_frames, a.t, &a.good)) return rc;
  HIP_TRY(ctx, launch_smooth_rotations(a, ctx->stream));
  return MOCAP_OK;
}

int fill_check(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, const int32_t* flag, const double* Rm, const double* t_pose,
               const int32_t* flag_s, const double* quat_s, const double* pos_s, const double* filled, const int32_t* src) {
  const char* who = "mocap_fill_rows";
  if (int rc = rows_check(ctx, who, n_frames, R)) return rc;
  if (!traj || !flag || !Rm || !t_pose || !filled || !src) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  const int given = (flag_s ? 1 : 0) + (quat_s ? 1 : 0) + (pos_s ? 1 : 0);
  if (given != 0 && given != 3) return ctx->fail(MOCAP_E_ARG, "%s: flag_s, quat_s and pos_s are given together or not at all", who);
  return MOCAP_OK;
}

int fill_dev_locked(mocap_ctx* ctx, FillRowsArgs a, const std::vector<BpBody>& table) {
  BpBody* d_bodies;
  auto lay = [&](void* base) {
    Carver c(base);
    d_bodies = c.take<BpBody>((size_t)a.B);
    a.row_of = c.take<int32_t>((size_t)a.R);
    return c.off;
  };
  if (ctx->calib_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(body trajectories workspace) failed");
  lay(ctx->calib_ws.ptr);
  a.bodies = d_bodies;
  HIP_TRY(ctx, launch_put_bodies(table.data(), a.B, d_bodies, ctx->stream));
  HIP_TRY(ctx, launch_fill_rows(a, ctx->stream));
  return MOCAP_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ stage 1
extern "C" int mocap_pose_rows_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_traj, int B, const int32_t* n_markers,
                                   const int32_t* rows, const double* markers, double max_rms, int32_t* d_n_used, int32_t* d_present,
                                   double* d_quat, double* d_Rm, double* d_t_pose, double* d_rms, int32_t* d_flag) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = pose_check(ctx, n_frames, R, d_traj, max_rms, d_n_used, d_present, d_quat, d_Rm, d_t_pose, d_rms, d_flag)) return rc;
  std::vector<BpBody> table;
  if (int rc = bodies_table(ctx, "mocap_pose_rows", R, B, n_markers, rows, markers, table)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  PoseRowsArgs a{n_frames, R, B, max_rms, d_traj, nullptr, nullptr, nullptr, d_n_used, d_present, d_flag, d_quat, d_Rm, d_t_pose, d_rms};
  const int rc = pose_dev_locked(ctx, a, table);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_pose_rows(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int B, const int32_t* n_markers,
                               const int32_t* rows, const double* markers, double max_rms, int32_t* n_used, int32_t* present,
                               double* quat, double* Rm, double* t_pose, double* rms, int32_t* flag) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = pose_check(ctx, n_frames, R, traj, max_rms, n_used, present, quat, Rm, t_pose, rms, flag)) return rc;
  std::vector<BpBody> table;
  if (int rc = bodies_table(ctx, "mocap_pose_rows", R, B, n_markers, rows, markers, table)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, N = (size_t)B * F;
  PoseRowsArgs a{n_frames, R, B, max_rms};
  double* d_traj;
  auto lay = [&](void* base) {
    Carver c(base);
    d_traj = c.take<double>((size_t)R * F * 3);
    a.quat = c.take<double>(N * 4);
    a.Rm = c.take<double>(N * 9);
    a.t_pose = c.take<double>(N * 3);
    a.rms = c.take<double>(N);
    a.n_used = c.take<int32_t>(N);
    a.present = c.take<int32_t>(N);
    a.flag = c.take<int32_t>(N);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  a.traj = d_traj;
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if (up(d_traj, traj, sizeof(double) * (size_t)R * F * 3)) return MOCAP_E_HIP;
  if (int rc = pose_dev_locked(ctx, a, table)) return rc;
  if (down(n_used, a.n_used, sizeof(int32_t) * N) || down(present, a.present, sizeof(int32_t) * N) ||
      down(quat, a.quat, sizeof(double) * N * 4) || down(Rm, a.Rm, sizeof(double) * N * 9) ||
      down(t_pose, a.t_pose, sizeof(double) * N * 3) || down(rms, a.rms, sizeof(double) * N) || down(flag, a.flag, sizeof(int32_t) * N))
    return MOCAP_E_HIP;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

// ------------------------------------------------------------------------------------------------------------------ stage 2
extern "C" int mocap_smooth_rotations_dev(mocap_ctx* ctx, int64_t n_frames, int B, const double* d_t, const double* d_quat, int degree,
                                          int W, double span, int n_min, int max_gap, double* d_quat_s, double* d_omega, double* d_res,
                                          int32_t* d_n_used, int32_t* d_flag) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = rot_check(ctx, n_frames, B, d_t, d_quat, degree, W, span, n_min, max_gap, d_quat_s, d_omega, d_res, d_n_used, d_flag))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const SmoothRotationsArgs a{n_frames, B, degree, W, n_min, max_gap, span, d_t, d_quat, nullptr, d_quat_s, d_omega, d_res, d_n_used, d_flag};
  const int rc = rot_dev_locked(ctx, a);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_smooth_rotations(mocap_ctx* ctx, int64_t n_frames, int B, const double* t, const double* quat, int degree, int W,
                                      double span, int n_min, int max_gap, double* quat_s, double* omega, double* res, int32_t* n_used,
                                      int32_t* flag) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = rot_check(ctx, n_frames, B, t, quat, degree, W, span, n_min, max_gap, quat_s, omega, res, n_used, flag)) return rc;
  bool any_finite = false;
  for (int64_t f = 0; f < n_frames && !any_finite; f++) any_finite = std::isfinite(t[f]);
  if (!any_finite) return ctx->fail(MOCAP_E_ARG, "mocap_smooth_rotations: t has no finite entry");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, N = (size_t)B * F;
  SmoothRotationsArgs a{n_frames, B, degree, W, n_min, max_gap, span};
  double *d_t, *d_quat;
  auto lay = [&](void* base) {
    Carver c(base);
    d_t = c.take<double>(F);
    d_quat = c.take<double>(N * 4);
    a.quat_s = c.take<double>(N * 4);
    a.omega = c.take<double>(N * 3);
    a.res = c.take<double>(N);
    a.n_used = c.take<int32_t>(N);
    a.flag = c.take<int32_t>(N);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  a.t = d_t;
  a.quat = d_quat;
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if (up(d_t, t, sizeof(double) * F) || up(d_quat, quat, sizeof(double) * N * 4)) return MOCAP_E_HIP;
  if (int rc = rot_dev_locked(ctx, a)) return rc;
  if (down(quat_s, a.quat_s, sizeof(double) * N * 4) || down(omega, a.omega, sizeof(double) * N * 3) ||
      down(res, a.res, sizeof(double) * N) || down(n_used, a.n_used, sizeof(int32_t) * N) || down(flag, a.flag, sizeof(int32_t) * N))
    return MOCAP_E_HIP;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

// ------------------------------------------------------------------------------------------------------------------ stage 3
extern "C" int mocap_fill_rows_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_traj, int B, const int32_t* n_markers,
                                   const int32_t* rows, const double* markers, const int32_t* d_flag, const double* d_Rm,
                                   const double* d_t_pose, const int32_t* d_flag_s, const double* d_quat_s, const double* d_pos_s,
                                   double* d_filled, int32_t* d_src) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = fill_check(ctx, n_frames, R, d_traj, d_flag, d_Rm, d_t_pose, d_flag_s, d_quat_s, d_pos_s, d_filled, d_src)) return rc;
  std::vector<BpBody> table;
  if (int rc = bodies_table(ctx, "mocap_fill_rows", R, B, n_markers, rows, markers, table)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const FillRowsArgs a{n_frames, R, B, d_traj, nullptr, nullptr, d_flag, d_Rm, d_t_pose, d_flag_s, d_quat_s, d_pos_s, d_filled, d_src};
  const int rc = fill_dev_locked(ctx, a, table);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_fill_rows(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int B, const int32_t* n_markers,
                               const int32_t* rows, const double* markers, const int32_t* flag, const double* Rm, const double* t_pose,
                               const int32_t* flag_s, const double* quat_s, const double* pos_s, double* filled, int32_t* src) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = fill_check(ctx, n_frames, R, traj, flag, Rm, t_pose, flag_s, quat_s, pos_s, filled, src)) return rc;
  std::vector<BpBody> table;
  if (int rc = bodies_table(ctx, "mocap_fill_rows", R, B, n_markers, rows, markers, table)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, N = (size_t)B * F, M = (size_t)R * F;
  FillRowsArgs a{n_frames, R, B};
  double *d_traj, *d_Rm, *d_t_pose, *d_quat_s, *d_pos_s;
  int32_t *d_flag, *d_flag_s;
  auto lay = [&](void* base) {
    Carver c(base);
    d_traj = c.take<double>(M * 3);
    d_Rm = c.take<double>(N * 9);
    d_t_pose = c.take<double>(N * 3);
    d_quat_s = c.take<double>(N * 4);
    d_pos_s = c.take<double>(N * 3);
    a.filled = c.take<double>(M * 3);
    d_flag = c.take<int32_t>(N);
    d_flag_s = c.take<int32_t>(N);
    a.src = c.take<int32_t>(M);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  a.traj = d_traj;
  a.flag = d_flag;
  a.Rm = d_Rm;
  a.t_pose = d_t_pose;
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if (up(d_traj, traj, sizeof(double) * M * 3) || up(d_flag, flag, sizeof(int32_t) * N) || up(d_Rm, Rm, sizeof(double) * N * 9) ||
      up(d_t_pose, t_pose, sizeof(double) * N * 3))
    return MOCAP_E_HIP;
  if (flag_s) {
    if (up(d_flag_s, flag_s, sizeof(int32_t) * N) || up(d_quat_s, quat_s, sizeof(double) * N * 4) ||
        up(d_pos_s, pos_s, sizeof(double) * N * 3))
      return MOCAP_E_HIP;
    a.flag_s = d_flag_s;
    a.quat_s = d_quat_s;
    a.pos_s = d_pos_s;
  }
  if (int rc = fill_dev_locked(ctx, a, table)) return rc;
  if (down(filled, a.filled, sizeof(double) * M * 3) || down(src, a.src, sizeof(int32_t) * M)) return MOCAP_E_HIP;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
