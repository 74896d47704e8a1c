// joints_capi.hip -- the "joints" section of include/mocap_core.h: which bodies of a session are joined, where and how, and a
// joint's motion per frame (kernels: joints.hip).  The host forms upload, run and download; the _dev forms read the poses where
// mocap_pose_rows left them.  The refusals and the joint table are joints_host.hpp's (plain C++, checked under the host sanitizers).
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "../../include/mocap_core.h"
#include "ctx.hpp"
#include "joints.hpp"

using namespace mocap;

static_assert(kJtMaxBodies == MOCAP_BP_MAX_BODIES && kJtMaxFrames == MOCAP_RG_MAX_FRAMES && kJtMaxJoints == MOCAP_JT_MAX_JOINTS, "limits");
static_assert(kJtUnseen == MOCAP_JT_UNSEEN && kJtSingular == MOCAP_JT_SINGULAR && kJtFixed == MOCAP_JT_FIXED &&
                  kJtHinge == MOCAP_JT_HINGE && kJtBall == MOCAP_JT_BALL,
              "kinds");

namespace {

constexpr size_t kSlabBudget = (size_t)192 << 20;  // bytes of the two slabs of one round of launches

int find_check(mocap_ctx* ctx, int64_t n_frames, int B, const int32_t* flag, const double* Rm, const double* t_pose, int min_common,
               double tol_rank, double max_sep, const int32_t* cnt, const int32_t* kind, const int32_t* accepted, const double* lam,
               const double* sep, const double* centre, const double* axis, const int32_t* parent, const int32_t* n_joints) {
  if (const char* why = jt_find_check(n_frames, B, min_common, tol_rank, max_sep)) return ctx->fail(MOCAP_E_ARG, "mocap_find_joints: %s", why);
  if (!flag || !Rm || !t_pose || !cnt || !kind || !accepted || !lam || !sep || !centre || !axis || !parent || !n_joints)
    return ctx->fail(MOCAP_E_ARG, "mocap_find_joints: null buffer");
  return MOCAP_OK;
}

// (arguments checked; context lock held by the caller; every pointer device-accessible)
int find_dev_locked(mocap_ctx* ctx, FindJointsArgs a) {
  const size_t P = (size_t)jt_tiles(a.n_frames), per_pair = P * (kJtSlots * sizeof(double) + kJtPairs * sizeof(int32_t));
  const size_t fit = kSlabBudget / per_pair, pairs = (size_t)jt_block_pairs(a.B);
  a.round_pairs = (int)(fit < 1 ? 1 : fit > pairs ? pairs : fit);
  auto lay = [&](void* base) {
    Carver c(base);
    a.slab = c.take<double>((size_t)a.round_pairs * kJtSlots * P);
    a.sums = c.take<double>((size_t)a.B * a.B * kJtSums);
    a.cslab = c.take<int32_t>((size_t)a.round_pairs * kJtPairs * P);
    return c.off;
  };
  if (ctx->calib_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(joints workspace) failed");
  lay(ctx->calib_ws.ptr);
  HIP_TRY(ctx, launch_find_joints(a, ctx->stream));
  return MOCAP_OK;
}

int series_check(mocap_ctx* ctx, int64_t n_frames, int B, const int32_t* flag, const double* quat, const double* Rm, const double* t_pose,
                 int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind, const double* c_a, const double* c_b,
                 const double* axis_b, const double* q_ref, const int32_t* present, const double* centre, const double* gap,
                 const double* quat_rel, const double* twist, std::vector<JtJoint>& table) {
  if (const char* why = jt_series_check(n_frames, B)) return ctx->fail(MOCAP_E_ARG, "mocap_joint_series: %s", why);
  if (!flag || !quat || !Rm || !t_pose || !present || !centre || !gap || !quat_rel || !twist)
    return ctx->fail(MOCAP_E_ARG, "mocap_joint_series: null buffer");
  if (const char* why = jt_joint_table(B, J, body_a, body_b, kind, c_a, c_b, axis_b, q_ref, table))
    return ctx->fail(MOCAP_E_ARG, "mocap_joint_series: %s", why);
  return MOCAP_OK;
}

int series_dev_locked(mocap_ctx* ctx, JointSeriesArgs a, const std::vector<JtJoint>& table) {
  JtJoint* d_joints;
  auto lay = [&](void* base) {
    Carver c(base);
    d_joints = c.take<JtJoint>((size_t)a.J);
    return c.off;
  };
  if (ctx->calib_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(joints workspace) failed");
  lay(ctx->calib_ws.ptr);
  a.joints = d_joints;
  HIP_TRY(ctx, launch_put_joints(table.data(), a.J, d_joints, ctx->stream));
  HIP_TRY(ctx, launch_joint_series(a, ctx->stream));
  return MOCAP_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ find
extern "C" int mocap_find_joints_dev(mocap_ctx* ctx, int64_t n_frames, int B, const int32_t* d_flag, const double* d_Rm,
                                     const double* d_t_pose, int min_common, double tol_rank, double max_sep, int32_t* d_cnt,
                                     int32_t* d_kind, int32_t* d_accepted, double* d_lam, double* d_sep, double* d_centre,
                                     double* d_axis, int32_t* d_parent, int32_t* d_n_joints) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = find_check(ctx, n_frames, B, d_flag, d_Rm, d_t_pose, min_common, tol_rank, max_sep, d_cnt, d_kind, d_accepted, d_lam,
                          d_sep, d_centre, d_axis, d_parent, d_n_joints))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  FindJointsArgs a{n_frames, B, min_common, tol_rank, max_sep, d_flag, d_Rm, d_t_pose};
  a.cnt = d_cnt;
  a.kind = d_kind;
  a.accepted = d_accepted;
  a.lam = d_lam;
  a.sep = d_sep;
  a.centre = d_centre;
  a.axis = d_axis;
  a.parent = d_parent;
  a.n_joints = d_n_joints;
  const int rc = find_dev_locked(ctx, a);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_find_joints(mocap_ctx* ctx, int64_t n_frames, int B, const int32_t* flag, const double* Rm, const double* t_pose,
                                 int min_common, double tol_rank, double max_sep, int32_t* cnt, int32_t* kind, int32_t* accepted,
                                 double* lam, double* sep, double* centre, double* axis, int32_t* parent, int32_t* n_joints) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = find_check(ctx, n_frames, B, flag, Rm, t_pose, min_common, tol_rank, max_sep, cnt, kind, accepted, lam, sep, centre, axis,
                          parent, n_joints))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)B * (size_t)n_frames, BB = (size_t)B * B;
  FindJointsArgs a{n_frames, B, min_common, tol_rank, max_sep};
  int32_t* d_flag;
  double *d_Rm, *d_t_pose;
  auto lay = [&](void* base) {
    Carver c(base);
    d_Rm = c.take<double>(N * 9);
    d_t_pose = c.take<double>(N * 3);
    a.lam = c.take<double>(BB * 3);
    a.sep = c.take<double>(BB);
    a.centre = c.take<double>(BB * 3);
    a.axis = c.take<double>(BB * 3);
    d_flag = c.take<int32_t>(N);
    a.cnt = c.take<int32_t>(BB);
    a.kind = c.take<int32_t>(BB);
    a.accepted = c.take<int32_t>(BB);
    a.parent = c.take<int32_t>((size_t)B);
    a.n_joints = c.take<int32_t>(1);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  a.flag = d_flag;
  a.Rm = d_Rm;
  a.t_pose = d_t_pose;
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if (up(d_flag, flag, sizeof(int32_t) * N) || up(d_Rm, Rm, sizeof(double) * N * 9) || up(d_t_pose, t_pose, sizeof(double) * N * 3))
    return MOCAP_E_HIP;
  if (int rc = find_dev_locked(ctx, a)) return rc;
  if (down(cnt, a.cnt, sizeof(int32_t) * BB) || down(kind, a.kind, sizeof(int32_t) * BB) ||
      down(accepted, a.accepted, sizeof(int32_t) * BB) || down(lam, a.lam, sizeof(double) * BB * 3) ||
      down(sep, a.sep, sizeof(double) * BB) || down(centre, a.centre, sizeof(double) * BB * 3) ||
      down(axis, a.axis, sizeof(double) * BB * 3) || down(parent, a.parent, sizeof(int32_t) * (size_t)B) ||
      down(n_joints, a.n_joints, sizeof(int32_t)))
    return MOCAP_E_HIP;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

// ------------------------------------------------------------------------------------------------------------------ series
extern "C" int mocap_joint_series_dev(mocap_ctx* ctx, int64_t n_frames, int B, const int32_t* d_flag, const double* d_quat,
                                      const double* d_Rm, const double* d_t_pose, int J, const int32_t* body_a, const int32_t* body_b,
                                      const int32_t* kind, const double* c_a, const double* c_b, const double* axis_b,
                                      const double* q_ref, int32_t* d_present, double* d_centre, double* d_gap, double* d_quat_rel,
                                      double* d_twist) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  std::vector<JtJoint> table;
  if (int rc = series_check(ctx, n_frames, B, d_flag, d_quat, d_Rm, d_t_pose, J, body_a, body_b, kind, c_a, c_b, axis_b, q_ref, d_present,
                            d_centre, d_gap, d_quat_rel, d_twist, table))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const JointSeriesArgs a{n_frames, B, J, d_flag, d_quat, d_Rm, d_t_pose, nullptr, d_present, d_centre, d_gap, d_quat_rel, d_twist};
  const int rc = series_dev_locked(ctx, a, table);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_joint_series(mocap_ctx* ctx, int64_t n_frames, int B, const int32_t* flag, const double* quat, const double* Rm,
                                  const double* t_pose, int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind,
                                  const double* c_a, const double* c_b, const double* axis_b, const double* q_ref, int32_t* present,
                                  double* centre, double* gap, double* quat_rel, double* twist) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  std::vector<JtJoint> table;
  if (int rc = series_check(ctx, n_frames, B, flag, quat, Rm, t_pose, J, body_a, body_b, kind, c_a, c_b, axis_b, q_ref, present, centre,
                            gap, quat_rel, twist, table))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)B * (size_t)n_frames, M = (size_t)J * (size_t)n_frames;
  JointSeriesArgs a{n_frames, B, J};
  int32_t* d_flag;
  double *d_quat, *d_Rm, *d_t_pose;
  auto lay = [&](void* base) {
    Carver c(base);
    d_quat = c.take<double>(N * 4);
    d_Rm = c.take<double>(N * 9);
    d_t_pose = c.take<double>(N * 3);
    a.centre = c.take<double>(M * 3);
    a.gap = c.take<double>(M);
    a.quat_rel = c.take<double>(M * 4);
    a.twist = c.take<double>(M * 2);
    d_flag = c.take<int32_t>(N);
    a.present = c.take<int32_t>(M);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  a.flag = d_flag;
  a.quat = d_quat;
  a.Rm = d_Rm;
  a.t_pose = d_t_pose;
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if (up(d_flag, flag, sizeof(int32_t) * N) || up(d_quat, quat, sizeof(double) * N * 4) || up(d_Rm, Rm, sizeof(double) * N * 9) ||
      up(d_t_pose, t_pose, sizeof(double) * N * 3))
    return MOCAP_E_HIP;
  if (int rc = series_dev_locked(ctx, a, table)) return rc;
  if (down(present, a.present, sizeof(int32_t) * M) || down(centre, a.centre, sizeof(double) * M * 3) ||
      down(gap, a.gap, sizeof(double) * M) || down(quat_rel, a.quat_rel, sizeof(double) * M * 4) ||
      down(twist, a.twist, sizeof(double) * M * 2))
    return MOCAP_E_HIP;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
