// resect_capi.hip -- the "camera resection" section of include/mocap_core.h: argument checks, the workspace, and the two-round
// Levenberg-Marquardt schedule around the kernels of resect.hip.  Search, scoring, the winner and the first linearisation are queued
// without the host seeing anything; from then on the host sees one 64-double pinned record per linearisation (sums down; a trial
// pose, its base and the increment between them up: one round trip, as in mocap_ba_joint_solve) and takes the 6 x 6 step itself
// (rs_lm_step, csrc/resect_math.hpp -- the same text the host check runs).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>

#include "../../include/mocap_core.h"
#include "ctx.hpp"
#include "resect.hpp"

using namespace mocap;

static_assert(kRsMaxPoints == MOCAP_RESECT_MAX_POINTS && kRsMaxHyp == MOCAP_RESECT_MAX_HYP && kRsInfo == MOCAP_RESECT_INFO &&
                  kRsOk == MOCAP_RESECT_OK && kRsTooFew == MOCAP_RESECT_TOO_FEW && kRsNoModel == MOCAP_RESECT_NO_MODEL,
              "resect_math.hpp mirrors include/mocap_core.h");

namespace {

struct RsWork {
  RsArgs a{};
  double *d_X = nullptr, *d_obs = nullptr;  // the host forms' copies of the inputs
  double* h_pose = nullptr;                 // pinned: [4][12] the prior; the pose, its base and the increment on their way up
};

int rs_check(mocap_ctx* ctx, const char* who, int64_t N, const double* X, const double* obs, const double* K, const double* prior_R,
             const double* prior_t, double threshold_px, int n_hyp, int n_hyp_min) {
  if (N < 1 || N > MOCAP_RESECT_MAX_POINTS) return ctx->fail(MOCAP_E_ARG, "%s: N must be 1 .. %d", who, MOCAP_RESECT_MAX_POINTS);
  if (n_hyp < n_hyp_min || n_hyp > MOCAP_RESECT_MAX_HYP)
    return ctx->fail(MOCAP_E_ARG, "%s: n_hyp must be %d .. %d", who, n_hyp_min, MOCAP_RESECT_MAX_HYP);
  if (!X || !obs || !K) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  if ((prior_R == nullptr) != (prior_t == nullptr)) return ctx->fail(MOCAP_E_ARG, "%s: prior_R and prior_t come together", who);
  if (n_hyp == 0 && !prior_R) return ctx->fail(MOCAP_E_ARG, "%s: n_hyp = 0 needs a prior pose", who);
  if (!(rs_finite(threshold_px) && threshold_px > 0.0)) return ctx->fail(MOCAP_E_ARG, "%s: threshold_px must be finite and > 0", who);
  if (K[1] != 0.0 || K[3] != 0.0 || K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0 || !(rs_finite(K[0]) && K[0] > 0.0) ||
      !(rs_finite(K[4]) && K[4] > 0.0) || !rs_finite(K[2]) || !rs_finite(K[5]))
    return ctx->fail(MOCAP_E_ARG, "%s: the intrinsic matrix is not [[fx,0,cx],[0,fy,cy],[0,0,1]] with finite fx, fy > 0", who);
  return MOCAP_OK;
}

// the workspace, the prior on the device and the output mask cleared; X and obs on the device already with `dev`
int rs_setup(mocap_ctx* ctx, RsWork& w, int64_t N, const double* X, const double* obs, bool dev, const double* K, const double* prior_R,
             const double* prior_t, double threshold_px, int n_hyp, uint64_t seed, int min_inliers) {
  RsArgs& a = w.a;
  a.N = N;
  a.has_prior = prior_R ? 1 : 0;
  a.H = n_hyp > 0 ? n_hyp : 1;
  a.min_inliers = min_inliers;
  a.seed = seed;
  a.k4[0] = K[0];
  a.k4[1] = K[4];
  a.k4[2] = K[2];
  a.k4[3] = K[5];
  a.thr2 = threshold_px * threshold_px;
  const size_t n = (size_t)N, H = (size_t)a.H;
  auto lay = [&](void* base) {
    Carver c(base);
    w.d_X = c.take<double>(dev ? 0 : n * 3);
    w.d_obs = c.take<double>(dev ? 0 : n * 2);
    a.rows = c.take<double>(n * 5);
    a.orig = c.take<int32_t>(n);
    a.hdr = c.take<int32_t>(8);
    a.blk = c.take<int32_t>((size_t)calib_partials(N));
    a.poses = c.take<double>(H * 48);
    a.n_sol = c.take<int32_t>(H);
    a.samp = c.take<int32_t>(H * 3);
    a.counts = c.take<int32_t>(H * 4);
    a.state = c.take<double>(8);
    a.pose = c.take<double>(12 * kRsSlots);
    a.mask = c.take<uint8_t>(n);
    a.mask_out = c.take<uint8_t>(n);
    a.slab = c.take<double>((size_t)calib_partials(N) * kRsSums);
    return c.off;
  };
  if (ctx->rs_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(camera resection workspace) failed");
  lay(ctx->rs_ws.ptr);
  const size_t pin = sizeof(double) * (kRsRec + 48);
  HIP_TRY(ctx, ctx->rs_pin.reserve(pin, pin, hipHostMallocCoherent));  // the record is written by the fold kernels
  a.rec = (double*)ctx->rs_pin.ptr;
  w.h_pose = a.rec + kRsRec;
  if (dev) {
    a.X = X;
    a.obs = obs;
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(w.d_X, X, sizeof(double) * n * 3, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(w.d_obs, obs, sizeof(double) * n * 2, hipMemcpyHostToDevice, ctx->stream));
    a.X = w.d_X;
    a.obs = w.d_obs;
  }
  for (int k = 0; k < 12; k++) w.h_pose[k] = prior_R ? (k < 9 ? prior_R[k] : prior_t[k - 9]) : std::nan("");
  HIP_TRY(ctx, hipMemcpyAsync(a.pose + 12 * kRsSlotPrior, w.h_pose, sizeof(double) * 12, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(a.mask_out, 0, n, ctx->stream));
  return MOCAP_OK;
}

int rs_solve(mocap_ctx* ctx, const char* who, int64_t N, const double* X, const double* obs, bool dev, const double* K,
             const double* prior_R, const double* prior_t, double threshold_px, int n_hyp, uint64_t seed, int min_inliers, int max_iter,
             double* R, double* t, uint8_t* mask, double* info) {
  int rc = rs_check(ctx, who, N, X, obs, K, prior_R, prior_t, threshold_px, n_hyp, 0);
  if (rc) return rc;
  if (!R || !t) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  if (min_inliers < 4) return ctx->fail(MOCAP_E_ARG, "%s: min_inliers must be at least 4", who);
  if (max_iter < 0) return ctx->fail(MOCAP_E_ARG, "%s: max_iter must be >= 0", who);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  RsWork w;
  if ((rc = rs_setup(ctx, w, N, X, obs, dev, K, prior_R, prior_t, threshold_px, n_hyp, seed, min_inliers))) return rc;
  const RsArgs& a = w.a;
  HIP_TRY(ctx, launch_resect_search(a, ctx->stream));
  double pose[12];
  int accepted = 0, linearisations = 0;
  if (max_iter > 0) {
    // the first linearisation, at the winner the device chose: queued behind the search, no wait in between
    HIP_TRY(ctx, launch_resect_normal_eq(a, 0, ctx->stream));
    if ((rc = spin_wait(ctx, ctx->ba_event))) return rc;
    linearisations = 1;
    if ((int)a.rec[kRsRecState + 5] == kRsOk) {
      for (int k = 0; k < 12; k++) pose[k] = a.rec[kRsRecPose + k];
      int lin_rc = MOCAP_OK;
      auto lin = [&](const double* p, const double* base, const double* inc, double* sums) {
        for (int k = 0; k < 12; k++) {  // slots 0 .. 2 are one run
          w.h_pose[12 + k] = p[k];
          w.h_pose[24 + k] = base ? base[k] : 0.0;
          w.h_pose[36 + k] = base ? inc[k] : 0.0;
        }
        hipError_t e = hipMemcpyAsync(a.pose + 12 * kRsSlotCur, w.h_pose + 12, sizeof(double) * 36, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = launch_resect_normal_eq(a, base ? 1 : 0, ctx->stream);
        if (e != hipSuccess) {
          lin_rc = ctx->hip_fail(e, "camera resection: linearisation");
          return false;
        }
        if ((lin_rc = spin_wait(ctx, ctx->ba_event))) return false;
        for (int k = 0; k < kRsSums; k++) sums[k] = a.rec[k];
        return true;
      };
      double first[kRsSums];
      for (int k = 0; k < kRsSums; k++) first[k] = a.rec[k];
      for (int round = 0; round < 2; round++) {
        RsRound out;
        if (!rs_round(pose, max_iter, lin, out, round == 0 ? first : nullptr)) return lin_rc;
        accepted += out.accepted;
        linearisations += out.linearisations - (round == 0 ? 1 : 0);
      }
      for (int k = 0; k < 12; k++) w.h_pose[12 + k] = pose[k];
      HIP_TRY(ctx, hipMemcpyAsync(a.pose + 12 * kRsSlotCur, w.h_pose + 12, sizeof(double) * 12, hipMemcpyHostToDevice, ctx->stream));
    }
  }
  HIP_TRY(ctx, launch_resect_finish(a, ctx->stream));
  if (mask) HIP_TRY(ctx, hipMemcpyAsync(mask, a.mask_out, (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = spin_wait(ctx, ctx->ba_event))) return rc;
  if (mask) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a copy into pageable memory
  const double* st = a.rec + kRsRecState;
  const double* fin = a.rec + kRsRecFinish;
  for (int k = 0; k < 9; k++) R[k] = a.rec[kRsRecPose + k];
  for (int k = 0; k < 3; k++) t[k] = a.rec[kRsRecPose + 9 + k];
  if (info) {
    const double qnan = std::nan("");
    const bool some = fin[0] > 0.0;
    info[0] = st[0];
    info[1] = st[1];
    info[2] = st[2];
    info[3] = st[3];
    info[4] = st[4];
    info[5] = fin[0];
    info[6] = accepted;
    info[7] = linearisations;
    info[8] = some && prior_R ? std::sqrt(fin[3] / fin[0]) : qnan;
    info[9] = some ? std::sqrt(fin[2] / fin[0]) : qnan;
    info[10] = some ? std::sqrt(fin[1] / fin[0]) : qnan;
    info[11] = st[5];
  }
  return MOCAP_OK;
}

}  // namespace

extern "C" int mocap_resect_camera(mocap_ctx* ctx, int64_t N, const double* X, const double* obs, const double* K, const double* prior_R,
                                   const double* prior_t, double threshold_px, int n_hyp, uint64_t seed, int min_inliers, int max_iter,
                                   double* R, double* t, uint8_t* mask, double* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return rs_solve(ctx, "mocap_resect_camera", N, X, obs, false, K, prior_R, prior_t, threshold_px, n_hyp, seed, min_inliers, max_iter, R, t,
                  mask, info);
}

extern "C" int mocap_resect_camera_dev(mocap_ctx* ctx, int64_t N, const double* d_X, const double* d_obs, const double* K,
                                       const double* prior_R, const double* prior_t, double threshold_px, int n_hyp, uint64_t seed,
                                       int min_inliers, int max_iter, double* R, double* t, uint8_t* mask, double* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int rc = rs_solve(ctx, "mocap_resect_camera_dev", N, d_X, d_obs, true, K, prior_R, prior_t, threshold_px, n_hyp, seed, min_inliers,
                          max_iter, R, t, mask, info);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_resect_hypotheses(mocap_ctx* ctx, int64_t N, const double* X, const double* obs, const double* K,
                                       const double* prior_R, const double* prior_t, double threshold_px, int n_hyp, uint64_t seed,
                                       int32_t* sample, int32_t* n_sol, double* poses, int32_t* counts) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const char* who = "mocap_resect_hypotheses";
  int rc = rs_check(ctx, who, N, X, obs, K, prior_R, prior_t, threshold_px, n_hyp, 1);
  if (rc) return rc;
  if (!sample || !n_sol || !poses || !counts) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  RsWork w;
  if ((rc = rs_setup(ctx, w, N, X, obs, false, K, prior_R, prior_t, threshold_px, n_hyp, seed, 4))) return rc;
  const RsArgs& a = w.a;
  HIP_TRY(ctx, launch_resect_search(a, ctx->stream));
  const size_t H = (size_t)a.H;
  HIP_TRY(ctx, hipMemcpyAsync(sample, a.samp, sizeof(int32_t) * H * 3, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(n_sol, a.n_sol, sizeof(int32_t) * H, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(poses, a.poses, sizeof(double) * H * 48, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(counts, a.counts, sizeof(int32_t) * H * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
