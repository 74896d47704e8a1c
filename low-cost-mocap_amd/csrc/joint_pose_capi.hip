// joint_pose_capi.hip -- the "joint poses" section of include/mocap_core.h: the bodies mocap_pose_rows could not pose, posed through
// the skeleton's joints from the bodies it could (kernels: joint_pose.hip).  The host form uploads, runs and downloads; the _dev
// form reads the session and the poses where they lie.  The bodies and the joints are host memory in both forms: the bodies are
// checked and tabulated by "body trajectories"' own function, the joints and the three parameters by joint_pose_host.hpp (plain
// C++, checked under the host sanitizers), and both tables travel to the device inside kernel arguments.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "../../include/mocap_core.h"
#include "ctx.hpp"
#include "joint_pose.hpp"

using namespace mocap;

static_assert(kJpMaxBodies == MOCAP_BP_MAX_BODIES && kJpMaxMarkers == MOCAP_RB_MAX_MARKERS && kJpMaxRounds == MOCAP_JP_MAX_ROUNDS, "limits");
static_assert(kBpJointed == MOCAP_BP_JOINTED && kJpMaxBodies == kBpMaxBodies && kJpMaxMarkers == kBpMaxMarkers, "flags");

namespace {

struct Tables {
  std::vector<BpBody> bodies;
  std::vector<JpDir> dirs;
  int32_t first[kJpMaxBodies + 1];
};

// every refusal of the call, before anything is written
int check(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int B, const int32_t* n_markers, const int32_t* rows,
          const double* markers, const int32_t* flag, const double* quat, const double* Rm, const double* t_pose, int J,
          const int32_t* body_a, const int32_t* body_b, const int32_t* kind, const double* c_a, const double* c_b, const double* axis_a,
          const double* axis_b, double axis_len, double max_rms, int max_rounds, const int32_t* flag_j, const int32_t* hops,
          const int32_t* via, const double* quat_j, const double* Rm_j, const double* t_j, const double* rms_j, Tables& tb) {
  const char* who = "mocap_pose_joints";
  if (int rc = rows_check(ctx, who, n_frames, R)) return rc;
  if (const char* why = jp_args_check(B, J, axis_len, max_rms, max_rounds)) return ctx->fail(MOCAP_E_ARG, "%s: %s", who, why);
  if (!traj || !flag || !quat || !Rm || !t_pose || !flag_j || !hops || !via || !quat_j || !Rm_j || !t_j || !rms_j)
    return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  if (int rc = bodies_table(ctx, who, R, B, n_markers, rows, markers, tb.bodies)) return rc;
  if (const char* why = jp_dir_table(B, n_markers, markers, J, body_a, body_b, kind, c_a, c_b, axis_a, axis_b, axis_len, tb.dirs, tb.first))
    return ctx->fail(MOCAP_E_ARG, "%s: %s", who, why);
  return MOCAP_OK;
}

// (arguments checked; context lock held by the caller; every pointer of `a` device-accessible)
int pose_dev_locked(mocap_ctx* ctx, PoseJointsArgs a, int max_rounds, const Tables& tb) {
  const size_t F = (size_t)a.n_frames, B = (size_t)a.B;
  BpBody* d_bodies;
  JpDir* d_dirs;
  auto lay = [&](void* base) {
    Carver c(base);
    d_bodies = c.take<BpBody>(B);
    d_dirs = c.take<JpDir>(tb.dirs.size());
    a.tile_i32 = c.take<int32_t>(B * (size_t)ts_tiles(a.n_frames));
    a.parity = c.take<uint8_t>(B * F);
    return c.off;
  };
  if (ctx->calib_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(joint poses workspace) failed");
  lay(ctx->calib_ws.ptr);
  a.bodies = d_bodies;
  a.dirs = d_dirs;
  for (int b = 0; b <= a.B; b++) a.first[b] = tb.first[b];
  HIP_TRY(ctx, launch_put_bodies(tb.bodies.data(), a.B, d_bodies, ctx->stream));
  HIP_TRY(ctx, launch_put_dirs(tb.dirs.data(), (int)tb.dirs.size(), d_dirs, ctx->stream));
  HIP_TRY(ctx, launch_pose_joints(a, max_rounds, ctx->stream));
  return MOCAP_OK;
}

}  // namespace

extern "C" int mocap_pose_joints_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_traj, int B, const int32_t* n_markers,
                                     const int32_t* rows, const double* markers, const int32_t* d_flag, const double* d_quat,
                                     const double* d_Rm, const double* d_t_pose, int J, const int32_t* body_a, const int32_t* body_b,
                                     const int32_t* kind, const double* c_a, const double* c_b, const double* axis_a,
                                     const double* axis_b, double axis_len, double max_rms, int max_rounds, int32_t* d_flag_j,
                                     int32_t* d_hops, int32_t* d_via, double* d_quat_j, double* d_Rm_j, double* d_t_j, double* d_rms_j) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Tables tb;
  if (int rc = check(ctx, n_frames, R, d_traj, B, n_markers, rows, markers, d_flag, d_quat, d_Rm, d_t_pose, J, body_a, body_b, kind, c_a,
                     c_b, axis_a, axis_b, axis_len, max_rms, max_rounds, d_flag_j, d_hops, d_via, d_quat_j, d_Rm_j, d_t_j, d_rms_j, tb))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  PoseJointsArgs a{};
  a.n_frames = n_frames;
  a.R = R;
  a.B = B;
  a.axis_len = axis_len;
  a.max_rms = max_rms;
  a.traj = d_traj;
  a.flag = d_flag;
  a.quat = d_quat;
  a.Rm = d_Rm;
  a.t_pose = d_t_pose;
  a.flag_j = d_flag_j;
  a.hops = d_hops;
  a.via = d_via;
  a.quat_j = d_quat_j;
  a.Rm_j = d_Rm_j;
  a.t_j = d_t_j;
  a.rms_j = d_rms_j;
  const int rc = pose_dev_locked(ctx, a, max_rounds, tb);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_pose_joints(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int B, const int32_t* n_markers,
                                 const int32_t* rows, const double* markers, const int32_t* flag, const double* quat, const double* Rm,
                                 const double* t_pose, int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind,
                                 const double* c_a, const double* c_b, const double* axis_a, const double* axis_b, double axis_len,
                                 double max_rms, int max_rounds, int32_t* flag_j, int32_t* hops, int32_t* via, double* quat_j,
                                 double* Rm_j, double* t_j, double* rms_j) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Tables tb;
  if (int rc = check(ctx, n_frames, R, traj, B, n_markers, rows, markers, flag, quat, Rm, t_pose, J, body_a, body_b, kind, c_a, c_b,
                     axis_a, axis_b, axis_len, max_rms, max_rounds, flag_j, hops, via, quat_j, Rm_j, t_j, rms_j, tb))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, N = (size_t)B * F, M = (size_t)R * F;
  PoseJointsArgs a{};
  a.n_frames = n_frames;
  a.R = R;
  a.B = B;
  a.axis_len = axis_len;
  a.max_rms = max_rms;
  double *d_traj, *d_quat, *d_Rm, *d_t_pose;
  int32_t* d_flag;
  auto lay = [&](void* base) {
    Carver c(base);
    d_traj = c.take<double>(M * 3);
    d_quat = c.take<double>(N * 4);
    d_Rm = c.take<double>(N * 9);
    d_t_pose = c.take<double>(N * 3);
    a.quat_j = c.take<double>(N * 4);
    a.Rm_j = c.take<double>(N * 9);
    a.t_j = c.take<double>(N * 3);
    a.rms_j = c.take<double>(N);
    d_flag = c.take<int32_t>(N);
    a.flag_j = c.take<int32_t>(N);
    a.hops = c.take<int32_t>(N);
    a.via = c.take<int32_t>(N);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  a.traj = d_traj;
  a.flag = d_flag;
  a.quat = d_quat;
  a.Rm = d_Rm;
  a.t_pose = d_t_pose;
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if (up(d_traj, traj, sizeof(double) * M * 3) || up(d_flag, flag, sizeof(int32_t) * N) || up(d_quat, quat, sizeof(double) * N * 4) ||
      up(d_Rm, Rm, sizeof(double) * N * 9) || up(d_t_pose, t_pose, sizeof(double) * N * 3))
    return MOCAP_E_HIP;
  if (int rc = pose_dev_locked(ctx, a, max_rounds, tb)) return rc;
  if (down(flag_j, a.flag_j, sizeof(int32_t) * N) || down(hops, a.hops, sizeof(int32_t) * N) || down(via, a.via, sizeof(int32_t) * N) ||
      down(quat_j, a.quat_j, sizeof(double) * N * 4) || down(Rm_j, a.Rm_j, sizeof(double) * N * 9) ||
      down(t_j, a.t_j, sizeof(double) * N * 3) || down(rms_j, a.rms_j, sizeof(double) * N))
    return MOCAP_E_HIP;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
