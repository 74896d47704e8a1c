// skeleton_fit_capi.hip -- the "skeleton fit" section of include/mocap_core.h: every active body of a frame fitted at once, the
// joints as weighted constraints (kernels: skeleton_fit.hip).  The host form uploads, runs and downloads; the _dev form reads the
// session and the poses where they lie.  The bodies and the joints are host memory in both forms: the bodies are checked and
// tabulated by "body trajectories"' own function, the joints by "joint poses"' own check, the parameters and the forest's tables
// by skeleton_fit_host.hpp (plain C++, checked under the host sanitizers).  The frames are taken in rounds of whole tiles under a
// fixed workspace cap; a frame's arithmetic does not know its round.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "../../include/mocap_core.h"
#include "ctx.hpp"
#include "skeleton_fit.hpp"

using namespace mocap;

static_assert(kSkMaxBodies == MOCAP_BP_MAX_BODIES && kSkMaxIters == MOCAP_SK_MAX_ITERS && kSkMaxBodies == kBpMaxBodies, "limits");

namespace {

struct Tables {
  std::vector<BpBody> bodies;
  std::vector<SkDir> dirs;
  SkForest fr;
};

// every refusal of the call, before anything is written
int check(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int B, const int32_t* n_markers, const int32_t* rows,
          const double* markers, const int32_t* flag, const double* quat, const double* t_pose, int J, const int32_t* body_a,
          const int32_t* body_b, const int32_t* kind, const double* c_a, const double* c_b, const double* axis_a, const double* axis_b,
          double axis_len, double w_joint, int iters, const double* quat_s, const double* Rm_s, const double* t_s, const double* rms_s,
          const double* cost0, const double* cost, const int32_t* steps, const int32_t* n_act, Tables& tb) {
  const char* who = "mocap_fit_skeleton";
  if (int rc = rows_check(ctx, who, n_frames, R)) return rc;
  if (const char* why = sk_args_check(B, J, axis_len, w_joint, iters)) return ctx->fail(MOCAP_E_ARG, "%s: %s", who, why);
  if (!traj || !flag || !quat || !t_pose || !quat_s || !Rm_s || !t_s || !rms_s || !cost0 || !cost || !steps || !n_act)
    return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  if (int rc = bodies_table(ctx, who, R, B, n_markers, rows, markers, tb.bodies)) return rc;
  if (const char* why = sk_tables(B, J, body_a, body_b, kind, c_a, c_b, axis_a, axis_b, tb.dirs, tb.fr))
    return ctx->fail(MOCAP_E_ARG, "%s: %s", who, why);
  return MOCAP_OK;
}

// (arguments checked; context lock held by the caller; every pointer of `a` device-accessible)
int fit_dev_locked(mocap_ctx* ctx, SkArgs a, int iters, const Tables& tb) {
  const size_t F = (size_t)a.n_frames, B = (size_t)a.B;
  a.cap = sk_round_frames(a.B, a.n_frames);
  const size_t cap = (size_t)a.cap;
  BpBody* d_bodies;
  SkDir* d_dirs;
  auto lay = [&](void* base) {
    Carver c(base);
    d_bodies = c.take<BpBody>(B);
    d_dirs = c.take<SkDir>(tb.dirs.size());
    a.tile_i32 = c.take<int32_t>(B * (size_t)ts_tiles(a.n_frames));
    a.parity = c.take<uint8_t>(B * F);
    a.ws = c.take<double>(B * kSkPlanes * cap);
    a.act = c.take<int32_t>(B * cap);
    a.lam = c.take<double>(cap);
    a.piv = c.take<int32_t>(cap);
    return c.off;
  };
  if (ctx->calib_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(skeleton fit workspace) failed");
  lay(ctx->calib_ws.ptr);
  a.bodies = d_bodies;
  a.dirs = d_dirs;
  a.fr = tb.fr;
  HIP_TRY(ctx, launch_put_bodies(tb.bodies.data(), a.B, d_bodies, ctx->stream));
  HIP_TRY(ctx, launch_put_sk_dirs(tb.dirs.data(), (int)tb.dirs.size(), d_dirs, ctx->stream));
  for (int64_t f0 = 0; f0 < a.n_frames; f0 += a.cap) {
    a.f0 = f0;
    a.nf = (int)(a.n_frames - f0 < a.cap ? a.n_frames - f0 : a.cap);
    HIP_TRY(ctx, launch_fit_skeleton_round(a, iters, ctx->stream));
  }
  HIP_TRY(ctx, launch_fit_skeleton_signs(a, ctx->stream));
  return MOCAP_OK;
}

}  // namespace

extern "C" int mocap_fit_skeleton_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_traj, int B, const int32_t* n_markers,
                                      const int32_t* rows, const double* markers, const int32_t* d_flag, const double* d_quat,
                                      const double* d_t_pose, int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind,
                                      const double* c_a, const double* c_b, const double* axis_a, const double* axis_b,
                                      double axis_len, double w_joint, int iters, double* d_quat_s, double* d_Rm_s, double* d_t_s,
                                      double* d_rms_s, double* d_cost0, double* d_cost, int32_t* d_steps, int32_t* d_n_act) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Tables tb;
  if (int rc = check(ctx, n_frames, R, d_traj, B, n_markers, rows, markers, d_flag, d_quat, d_t_pose, J, body_a, body_b, kind, c_a, c_b,
                     axis_a, axis_b, axis_len, w_joint, iters, d_quat_s, d_Rm_s, d_t_s, d_rms_s, d_cost0, d_cost, d_steps, d_n_act, tb))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  SkArgs a{};
  a.n_frames = n_frames;
  a.R = R;
  a.B = B;
  a.J = J;
  a.axis_len = axis_len;
  a.w_joint = w_joint;
  a.traj = d_traj;
  a.flag = d_flag;
  a.quat = d_quat;
  a.t_pose = d_t_pose;
  a.quat_s = d_quat_s;
  a.Rm_s = d_Rm_s;
  a.t_s = d_t_s;
  a.rms_s = d_rms_s;
  a.cost0 = d_cost0;
  a.cost = d_cost;
  a.steps = d_steps;
  a.n_act = d_n_act;
  const int rc = fit_dev_locked(ctx, a, iters, tb);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_fit_skeleton(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int B, const int32_t* n_markers,
                                  const int32_t* rows, const double* markers, const int32_t* flag, const double* quat,
                                  const double* t_pose, int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind,
                                  const double* c_a, const double* c_b, const double* axis_a, const double* axis_b, double axis_len,
                                  double w_joint, int iters, double* quat_s, double* Rm_s, double* t_s, double* rms_s, double* cost0,
                                  double* cost, int32_t* steps, int32_t* n_act) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  Tables tb;
  if (int rc = check(ctx, n_frames, R, traj, B, n_markers, rows, markers, flag, quat, t_pose, J, body_a, body_b, kind, c_a, c_b, axis_a,
                     axis_b, axis_len, w_joint, iters, quat_s, Rm_s, t_s, rms_s, cost0, cost, steps, n_act, tb))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, N = (size_t)B * F, M = (size_t)R * F;
  SkArgs a{};
  a.n_frames = n_frames;
  a.R = R;
  a.B = B;
  a.J = J;
  a.axis_len = axis_len;
  a.w_joint = w_joint;
  double *d_traj, *d_quat, *d_t_pose;
  int32_t* d_flag;
  auto lay = [&](void* base) {
    Carver c(base);
    d_traj = c.take<double>(M * 3);
    d_quat = c.take<double>(N * 4);
    d_t_pose = c.take<double>(N * 3);
    a.quat_s = c.take<double>(N * 4);
    a.Rm_s = c.take<double>(N * 9);
    a.t_s = c.take<double>(N * 3);
    a.rms_s = c.take<double>(N);
    a.cost0 = c.take<double>(F);
    a.cost = c.take<double>(F);
    d_flag = c.take<int32_t>(N);
    a.steps = c.take<int32_t>(F);
    a.n_act = c.take<int32_t>(F);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  a.traj = d_traj;
  a.flag = d_flag;
  a.quat = d_quat;
  a.t_pose = d_t_pose;
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if (up(d_traj, traj, sizeof(double) * M * 3) || up(d_flag, flag, sizeof(int32_t) * N) || up(d_quat, quat, sizeof(double) * N * 4) ||
      up(d_t_pose, t_pose, sizeof(double) * N * 3))
    return MOCAP_E_HIP;
  if (int rc = fit_dev_locked(ctx, a, iters, tb)) return rc;
  if (down(quat_s, a.quat_s, sizeof(double) * N * 4) || down(Rm_s, a.Rm_s, sizeof(double) * N * 9) ||
      down(t_s, a.t_s, sizeof(double) * N * 3) || down(rms_s, a.rms_s, sizeof(double) * N) || down(cost0, a.cost0, sizeof(double) * F) ||
      down(cost, a.cost, sizeof(double) * F) || down(steps, a.steps, sizeof(int32_t) * F) || down(n_act, a.n_act, sizeof(int32_t) * F))
    return MOCAP_E_HIP;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
