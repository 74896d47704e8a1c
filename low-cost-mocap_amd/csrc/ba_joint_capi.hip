// ba_joint_capi.hip -- the "joint bundle adjustment" section of include/mocap_core.h: argument checks, the workspace, and the
// Levenberg-Marquardt loop around the kernels of ba_joint.hip.  Per iteration the host sees the reduced camera system (S down,
// delta up: one round trip, as in mocap_ba_solve) and solves it with the dense Cholesky of tr_host.cpp; everything per point stays on
// the context's stream.  Two sets of (poses, points, E, L) alternate: the linearisation at an accepted trial is the next system.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/mocap_core.h"
#include "ba_joint.hpp"
#include "ctx.hpp"
#include "tr_host.hpp"

using namespace mocap;

static_assert(kBajMaxCameras == MOCAP_BAJ_MAX_CAMERAS && kBajMaxPoints == MOCAP_BAJ_MAX_POINTS, "ba_joint.hpp mirrors include/mocap_core.h");

namespace {

struct BajWork {
  int C = 0, focal = 0, n_c = 0, NP = 0, ksplit = 1;
  int64_t N = 0, m_pad = 0, P = 0;
  double huber = 0.0;
  // device
  double *d_obs = nullptr, *d_Ptab = nullptr, *d_cams[2] = {nullptr, nullptr}, *d_X[2] = {nullptr, nullptr}, *d_L[2] = {nullptr, nullptr},
         *d_Jaug[2] = {nullptr, nullptr}, *d_rho = nullptr, *d_partial = nullptr, *d_delta = nullptr, *d_slab = nullptr, *d_Xout = nullptr;
  int32_t *d_part = nullptr, *d_flags[2] = {nullptr, nullptr};
  // pinned host
  double *h_G[2] = {nullptr, nullptr}, *h_sums[2] = {nullptr, nullptr}, *h_cams[2] = {nullptr, nullptr}, *h_delta = nullptr, *h_Ptab = nullptr;
};

// what the host reads off one linearisation
struct BajStats {
  double cost = 0.0, views = 0.0, down = 0.0, skipped = 0.0, part = 0.0, singular = 0.0;
  bool camera_unseen = false;
};

int baj_check(mocap_ctx* ctx, const char* who, int64_t N, const double* obs, const double* R, const double* t, const double* fscale,
              uint32_t flags, double huber_px) {
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "%s: mocap_set_cameras has not been called", who);
  const int C = ctx->C;
  if (C < 2 || C > MOCAP_BAJ_MAX_CAMERAS) return ctx->fail(MOCAP_E_ARG, "%s: %d cameras, 2 .. %d are taken", who, C, MOCAP_BAJ_MAX_CAMERAS);
  if (N < 1 || N > MOCAP_BAJ_MAX_POINTS) return ctx->fail(MOCAP_E_ARG, "%s: N must be 1 .. %d", who, MOCAP_BAJ_MAX_POINTS);
  if (flags & ~(uint32_t)MOCAP_BAJ_FOCAL) return ctx->fail(MOCAP_E_ARG, "%s: unknown flag bits 0x%x", who, flags);
  if ((flags & MOCAP_BAJ_FOCAL) && C < 3) return ctx->fail(MOCAP_E_ARG, "%s: MOCAP_BAJ_FOCAL needs at least 3 cameras", who);
  if (!obs || !R || !t || ((flags & MOCAP_BAJ_FOCAL) && !fscale)) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  if (!(huber_px >= 0.0) || !baj_finite(huber_px)) return ctx->fail(MOCAP_E_ARG, "%s: huber_px must be finite and >= 0", who);
  for (int c = 0; c < C; c++) {
    const double* K = ctx->hK.data() + 9 * c;
    if (K[1] != 0.0 || K[3] != 0.0 || K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0)
      return ctx->fail(MOCAP_E_ARG, "%s: the intrinsic matrix of camera %d is not [[fx,0,cx],[0,fy,cy],[0,0,1]]", who, c);
  }
  return MOCAP_OK;
}

int baj_setup(mocap_ctx* ctx, BajWork& w, int64_t N, const double* obs, uint32_t flags, double huber_px) {
  const int C = ctx->C;
  w.C = C;
  w.focal = (flags & MOCAP_BAJ_FOCAL) ? 1 : 0;
  w.n_c = 6 * (C - 1) + (w.focal ? C : 0);
  w.NP = (w.n_c + 1 + 15) / 16 * 16;
  w.N = N;
  w.m_pad = (3 * N + 3) / 4 * 4;
  w.P = calib_partials(N);
  w.ksplit = ba_gram_ksplit(w.m_pad, w.NP);
  w.huber = huber_px;
  const size_t n = (size_t)N, nJ = (size_t)w.m_pad * w.NP, nG = (size_t)w.NP * w.NP;
  auto lay = [&](void* base) {
    Carver c(base);
    w.d_obs = c.take<double>(n * C * 2);
    w.d_Ptab = c.take<double>((size_t)C * 12);
    for (int s = 0; s < 2; s++) {
      w.d_cams[s] = c.take<double>((size_t)C * kBajCam);
      w.d_X[s] = c.take<double>(n * 3);
      w.d_L[s] = c.take<double>(n * 6);
      w.d_flags[s] = c.take<int32_t>(n);
    }
    w.d_Jaug[0] = c.take<double>(2 * nJ);  // the two in one run: one fill zeroes both
    w.d_Jaug[1] = w.d_Jaug[0] + nJ;
    w.d_rho = c.take<double>(n);
    w.d_partial = c.take<double>((size_t)w.ksplit * nG);
    w.d_delta = c.take<double>((size_t)w.NP);
    w.d_slab = c.take<double>((size_t)C * w.P * kBajSlab);
    w.d_Xout = c.take<double>(n * 3);
    w.d_part = c.take<int32_t>(n);
    return c.off;
  };
  if (ctx->baj_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(joint bundle adjustment workspace) failed");
  lay(ctx->baj_ws.ptr);
  auto lay_pin = [&](void* base) {
    Carver c(base);
    for (int s = 0; s < 2; s++) {
      w.h_G[s] = c.take<double>(nG);
      w.h_sums[s] = c.take<double>((size_t)C * kBajSlab);
      w.h_cams[s] = c.take<double>((size_t)C * kBajCam);
    }
    w.h_delta = c.take<double>((size_t)w.NP);
    w.h_Ptab = c.take<double>((size_t)C * 12);
    return c.off;
  };
  const size_t pin = lay_pin(nullptr);
  HIP_TRY(ctx, ctx->baj_pin.reserve(pin, pin, hipHostMallocCoherent));  // G and the camera blocks are written by the kernels
  lay_pin(ctx->baj_pin.ptr);
  HIP_TRY(ctx, hipMemcpyAsync(w.d_obs, obs, sizeof(double) * n * C * 2, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w.d_Jaug[0], 0, sizeof(double) * 2 * nJ, ctx->stream));
  return MOCAP_OK;
}

// the pose table of one set: R, t as given, fx = fx0 s, fy = fy0 s
void baj_fill_cams(const mocap_ctx* ctx, const double* R, const double* t, const double* s, double* out) {
  for (int c = 0; c < ctx->C; c++) {
    const double* K = ctx->hK.data() + 9 * c;
    double* o = out + kBajCam * c;
    for (int k = 0; k < 9; k++) o[k] = R[9 * c + k];
    for (int k = 0; k < 3; k++) o[9 + k] = t[3 * c + k];
    o[12] = K[0] * s[c];
    o[13] = K[4] * s[c];
    o[14] = K[2];
    o[15] = K[5];
  }
}

int baj_upload_cams(mocap_ctx* ctx, BajWork& w, int slot, const double* R, const double* t, const double* s) {
  baj_fill_cams(ctx, R, t, s, w.h_cams[slot]);
  HIP_TRY(ctx, hipMemcpyAsync(w.d_cams[slot], w.h_cams[slot], sizeof(double) * w.C * kBajCam, hipMemcpyHostToDevice, ctx->stream));
  return MOCAP_OK;
}

BajArgs baj_args(const BajWork& w, int slot, double lambda) {
  BajArgs a{};
  a.C = w.C;
  a.focal = w.focal;
  a.n_c = w.n_c;
  a.NP = w.NP;
  a.N = w.N;
  a.m_pad = w.m_pad;
  a.huber = w.huber;
  a.lambda = lambda;
  a.obs = w.d_obs;
  a.cams = w.d_cams[slot];
  a.X = w.d_X[slot];
  a.part = w.d_part;
  a.Jaug = w.d_Jaug[slot];
  a.L = w.d_L[slot];
  a.rho = w.d_rho;
  a.flags = w.d_flags[slot];
  a.partial = w.d_partial;
  a.ksplit = w.ksplit;
  a.G = w.h_G[slot];
  a.slab = w.d_slab;
  a.sums = w.h_sums[slot];
  return a;
}

// linearise set `slot` at damping lambda and wait for G and the camera blocks
int baj_linearise(mocap_ctx* ctx, BajWork& w, int slot, double lambda, BajStats& st) {
  HIP_TRY(ctx, launch_baj_linearise(baj_args(w, slot, lambda), ctx->stream));
  const int rc = spin_wait(ctx, ctx->ba_event);
  if (rc) return rc;
  st = BajStats{};
  for (int c = 0; c < w.C; c++) {  // camera order
    const double* s = w.h_sums[slot] + kBajSlab * c;
    st.views += s[36];
    st.down += s[37];
    st.skipped += s[38];
    if (s[36] + s[38] == 0.0) st.camera_unseen = true;
  }
  st.cost = w.h_sums[slot][35];
  st.part = w.h_sums[slot][39];
  st.singular = w.h_sums[slot][40];
  return MOCAP_OK;
}

// the DLT table of the start: P_c = K_c [R_c | t_c], left to right
void baj_ptab(const mocap_ctx* ctx, const double* R, const double* t, double* P) {
  for (int c = 0; c < ctx->C; c++) {
    const double* K = ctx->hK.data() + 9 * c;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 4; j++) {
        const double m0 = j < 3 ? R[9 * c + j] : t[3 * c], m1 = j < 3 ? R[9 * c + 3 + j] : t[3 * c + 1],
                     m2 = j < 3 ? R[9 * c + 6 + j] : t[3 * c + 2];
        P[12 * c + 4 * i + j] = (K[3 * i] * m0 + K[3 * i + 1] * m1) + K[3 * i + 2] * m2;
      }
  }
}

void baj_ones(std::vector<double>& s, int C, const double* fscale, bool focal) {
  s.assign(C, 1.0);
  if (focal)
    for (int c = 0; c < C; c++) s[c] = fscale[c];
}

}  // namespace

extern "C" int mocap_ba_joint_normal_eq(mocap_ctx* ctx, int64_t N, const double* obs, const double* R, const double* t,
                                        const double* fscale, const double* X, uint32_t flags, double huber_px, double lambda,
                                        double* S, double* rhs, double* cost, double* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const char* who = "mocap_ba_joint_normal_eq";
  int rc = baj_check(ctx, who, N, obs, R, t, fscale, flags, huber_px);
  if (rc) return rc;
  if (!X || !S || !rhs) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  if (!(lambda >= 0.0) || !baj_finite(lambda)) return ctx->fail(MOCAP_E_ARG, "%s: lambda must be finite and >= 0", who);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  BajWork w;
  if ((rc = baj_setup(ctx, w, N, obs, flags, huber_px))) return rc;
  std::vector<double> s;
  baj_ones(s, w.C, fscale, w.focal != 0);
  if ((rc = baj_upload_cams(ctx, w, 0, R, t, s.data()))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(w.d_X[0], X, sizeof(double) * (size_t)N * 3, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, launch_baj_start(w.C, N, w.d_obs, nullptr, 1, w.d_X[0], w.d_part, ctx->stream));
  BajStats st;
  if ((rc = baj_linearise(ctx, w, 0, lambda, st))) return rc;
  baj_assemble(w.C, w.focal != 0, w.NP, w.h_G[0], w.h_sums[0], lambda, S, rhs);
  if (cost) *cost = st.cost;
  if (info) {
    for (int i = 0; i < MOCAP_BAJ_INFO; i++) info[i] = 0.0;
    info[2] = info[3] = st.cost;
    info[4] = lambda;
    info[5] = st.part;
    info[6] = (double)N - st.part;
    info[7] = st.down;
    info[8] = (double)((st.camera_unseen ? MOCAP_BAJ_ST_CAMERA_UNSEEN : 0) | (st.part == 0.0 ? MOCAP_BAJ_ST_NO_POINTS : 0) |
                       (st.singular > 0.0 ? MOCAP_BAJ_ST_POINT_SINGULAR : 0) | (st.skipped > 0.0 ? MOCAP_BAJ_ST_BAD_DEPTH : 0));
  }
  return MOCAP_OK;
}

extern "C" int mocap_ba_joint_solve(mocap_ctx* ctx, int64_t N, const double* obs, double* R, double* t, double* fscale, double* X_out,
                                    uint32_t flags, double huber_px, double ftol, int max_iter, double* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const char* who = "mocap_ba_joint_solve";
  int rc = baj_check(ctx, who, N, obs, R, t, fscale, flags, huber_px);
  if (rc) return rc;
  if (!(ftol >= 0.0) || !baj_finite(ftol)) return ctx->fail(MOCAP_E_ARG, "%s: ftol must be finite and >= 0", who);
  if (max_iter < 1) return ctx->fail(MOCAP_E_ARG, "%s: max_iter must be at least 1", who);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const auto t_begin = std::chrono::steady_clock::now();
  BajWork w;
  if ((rc = baj_setup(ctx, w, N, obs, flags, huber_px))) return rc;
  const int C = w.C, n_c = w.n_c;
  const bool focal = w.focal != 0;
  // the current set of poses on the host, and the trial
  std::vector<double> Rc(R, R + 9 * C), tc(t, t + 3 * C), sc, Rt, tt, st_;
  baj_ones(sc, C, fscale, focal);
  baj_ptab(ctx, Rc.data(), tc.data(), w.h_Ptab);
  HIP_TRY(ctx, hipMemcpyAsync(w.d_Ptab, w.h_Ptab, sizeof(double) * C * 12, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, launch_baj_start(C, N, w.d_obs, w.d_Ptab, 0, w.d_X[0], w.d_part, ctx->stream));
  int cur = 0;
  if ((rc = baj_upload_cams(ctx, w, cur, Rc.data(), tc.data(), sc.data()))) return rc;
  double lambda = 1e-3;
  BajStats st;
  if ((rc = baj_linearise(ctx, w, cur, lambda, st))) return rc;
  const double cost0 = st.cost, part = st.part;
  double cost = cost0, down = st.down, dev_ms = 0.0;
  int passes = 0, accepted = 0, linearisations = 1;
  uint32_t status = 0;
  if (st.singular > 0.0) status |= MOCAP_BAJ_ST_POINT_SINGULAR;
  if (part == 0.0) status |= MOCAP_BAJ_ST_NO_POINTS;
  if (st.camera_unseen) status |= MOCAP_BAJ_ST_CAMERA_UNSEEN;
  const bool run = !(status & (MOCAP_BAJ_ST_NO_POINTS | MOCAP_BAJ_ST_CAMERA_UNSEEN));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  struct Events {
    hipEvent_t &a, &b;
    ~Events() {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  } events{e0, e1};
  if (run) {
    HIP_TRY(ctx, hipEventCreate(&e0));
    HIP_TRY(ctx, hipEventCreate(&e1));
  }
  std::vector<double> S((size_t)n_c * n_c), rhs(n_c), delta(n_c), xprog(1 + 7 * (C - 1));
  bool stale = false;  // the current set's E and L belong to another lambda (a trial was rejected)
  while (run) {
    if (lambda > 1e12) {
      status |= MOCAP_BAJ_ST_LAMBDA;
      break;
    }
    if (passes >= max_iter) {
      status |= MOCAP_BAJ_ST_MAX_ITER;
      break;
    }
    passes++;
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    BajStats tr;
    bool ok = true;
    if (stale) {
      if ((rc = baj_linearise(ctx, w, cur, lambda, st))) return rc;
      linearisations++;
      stale = false;
    }
    baj_assemble(C, focal, w.NP, w.h_G[cur], w.h_sums[cur], lambda, S.data(), rhs.data());
    if (!baj_chol_solve(n_c, S.data(), rhs.data(), delta.data())) {
      status |= MOCAP_BAJ_ST_SINGULAR;
      ok = false;
    }
    const double lambda_t = lambda / 10.0 > 1e-12 ? lambda / 10.0 : 1e-12;
    if (ok) {
      // the trial poses
      Rt = Rc;
      tt = tc;
      st_ = sc;
      for (int c = 1; c < C; c++) {
        baj_rotate(delta.data() + 6 * (c - 1), Rt.data() + 9 * c);
        for (int k = 0; k < 3; k++) tt[3 * c + k] = tc[3 * c + k] + delta[6 * (c - 1) + 3 + k];
      }
      if (focal)
        for (int c = 0; c < C; c++) st_[c] = sc[c] * (1.0 + delta[6 * (C - 1) + c]);
      const int trial = 1 - cur;
      if ((rc = baj_upload_cams(ctx, w, trial, Rt.data(), tt.data(), st_.data()))) return rc;
      for (int i = 0; i < w.NP; i++) w.h_delta[i] = i < n_c ? delta[i] : 0.0;
      HIP_TRY(ctx, hipMemcpyAsync(w.d_delta, w.h_delta, sizeof(double) * w.NP, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, launch_baj_backsub(baj_args(w, cur, lambda), w.d_delta, w.d_X[trial], ctx->stream));
      if ((rc = baj_linearise(ctx, w, trial, lambda_t, tr))) return rc;
      linearisations++;
      ok = baj_finite(tr.cost) && tr.skipped == 0.0 && tr.cost < cost;
    }
    HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
    dev_ms += ms;
    if (!ok) {
      lambda = lambda * 10.0;
      stale = true;
      continue;
    }
    const double before = cost;
    cost = tr.cost;
    down = tr.down;
    if (tr.singular > 0.0) status |= MOCAP_BAJ_ST_POINT_SINGULAR;
    cur = 1 - cur;
    lambda = lambda_t;
    Rc.swap(Rt);
    tc.swap(tt);
    sc.swap(st_);
    accepted++;
    if (ctx->ba_progress) {  // the reference's vector layout [f0, (f_i, rotvec_i, t_i)]
      xprog[0] = ctx->hK[0] * sc[0];
      for (int c = 1; c < C; c++) {
        double* x = xprog.data() + 1 + 7 * (c - 1);
        x[0] = ctx->hK[9 * c] * sc[c];
        baj_rotvec(Rc.data() + 9 * c, x + 1);
        for (int k = 0; k < 3; k++) x[4 + k] = tc[3 * c + k];
      }
      ctx->ba_progress(xprog.data(), (int)xprog.size(), ctx->ba_progress_user);
    }
    if (before - cost <= ftol * before) break;
  }
  // the gauge: |t_1| as it came
  double scale = 1.0;
  if (run) {
    const double n_in = std::sqrt((t[3] * t[3] + t[4] * t[4]) + t[5] * t[5]);
    const double n_out = std::sqrt((tc[3] * tc[3] + tc[4] * tc[4]) + tc[5] * tc[5]);
    if (baj_finite(n_in) && baj_finite(n_out) && n_in > 0.0 && n_out > 0.0) scale = n_in / n_out;
  }
  if (X_out) {
    HIP_TRY(ctx, launch_baj_finish(N, w.d_X[cur], w.d_part, scale, w.d_Xout, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(X_out, w.d_Xout, sizeof(double) * (size_t)N * 3, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (run && accepted > 0) {  // camera 0 is never written
    for (int c = 1; c < C; c++) {
      for (int k = 0; k < 9; k++) R[9 * c + k] = Rc[9 * c + k];
      for (int k = 0; k < 3; k++) t[3 * c + k] = tc[3 * c + k] * scale;
    }
    if (focal)
      for (int c = 0; c < C; c++) fscale[c] = sc[c];
  }
  if (info) {
    info[0] = passes;
    info[1] = accepted;
    info[2] = cost0;
    info[3] = cost;
    info[4] = lambda;
    info[5] = part;
    info[6] = (double)N - part;
    info[7] = down;
    info[8] = (double)status;
    info[9] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    info[10] = dev_ms;
    info[11] = linearisations;
  }
  return MOCAP_OK;
}
