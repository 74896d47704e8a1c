// ba_schur_host.hpp -- the host's half of the bundle adjustment with eliminated points, written once for the "joint bundle
// adjustment" and the "lens calibration" sections of include/mocap_core.h (csrc/ba_joint_capi.hip, csrc/ba_lens_capi.hip): the
// workspace, one linearisation, the assembly of the reduced camera system, and the Levenberg-Marquardt loop around the kernels of
// csrc/ba_schur.hpp.  Per iteration the host sees the reduced camera system (S down, delta up: one round trip, as in
// mocap_ba_solve) and solves it with the dense Cholesky of tr_host.cpp; everything per point stays on the context's stream.  Two sets
// of (cameras, points, E, L) alternate: the linearisation at an accepted trial is the next system.  The workspace is ctx->baj_ws and
// ctx->baj_pin for every solver: one context is one serialised caller, two solvers never run at the same time.
// A solver H describes its cameras and is never asked which one it is:
//   H::Dev, H::kSection, H::launch         the device model (csrc/ba_schur.hpp), the section's name in a failure text, the 5 launches
//   int C; uint32_t sel                    set by check(): the cameras, and which pairs of intrinsics are unknowns
//   check (ctx, who, N, obs, R, t, huber)  the argument check: MOCAP_OK or ctx->fail(...)
//   K9 ()                                  K [C][9] of the DLT start
//   init (state)                           the intrinsic state of the caller's cameras
//   fill_cams (R, t, state, out)           the camera table [C][Dev::kCam] of one set
//   trial (w, delta, cur, next)            next = cur stepped by delta; false: the trial is rejected unseen
//   accepted (R, t, state)                 runs on an accepted step
//   write_back (w, state)                  the intrinsics back to the caller (after at least one accepted step)
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <vector>

#include "../../include/mocap_core.h"
#include "ba_schur.hpp"
#include "ctx.hpp"
#include "tr_host.hpp"

namespace mocap {

// the loop below speaks of one set of status bits and one info layout
static_assert((int)MOCAP_BAL_ST_CAMERA_UNSEEN == (int)MOCAP_BAJ_ST_CAMERA_UNSEEN && (int)MOCAP_BAL_ST_NO_POINTS == (int)MOCAP_BAJ_ST_NO_POINTS &&
                  (int)MOCAP_BAL_ST_SINGULAR == (int)MOCAP_BAJ_ST_SINGULAR && (int)MOCAP_BAL_ST_POINT_SINGULAR == (int)MOCAP_BAJ_ST_POINT_SINGULAR &&
                  (int)MOCAP_BAL_ST_LAMBDA == (int)MOCAP_BAJ_ST_LAMBDA && (int)MOCAP_BAL_ST_MAX_ITER == (int)MOCAP_BAJ_ST_MAX_ITER &&
                  (int)MOCAP_BAL_ST_BAD_DEPTH == (int)MOCAP_BAJ_ST_BAD_DEPTH,
              "the lens calibration reports in the joint bundle adjustment's status bits");
static_assert(MOCAP_BAL_INFO == MOCAP_BAJ_INFO, "... and in its info slots");

struct SchurWork {
  int C = 0, q = 0, n_c = 0, NP = 0, ksplit = 1;
  int rank[8] = {-1, -1, -1, -1, -1, -1, -1, -1};  // per intrinsic (parameter 6 + k): its place among the camera's q unknowns, -1 = fixed
  uint32_t sel = 0;
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
struct SchurStats {
  double cost = 0.0, views = 0.0, down = 0.0, skipped = 0.0, part = 0.0, singular = 0.0;
  bool camera_unseen = false;
};

inline uint32_t schur_status(const SchurStats& st) {
  return (st.camera_unseen ? MOCAP_BAJ_ST_CAMERA_UNSEEN : 0) | (st.part == 0.0 ? MOCAP_BAJ_ST_NO_POINTS : 0) |
         (st.singular > 0.0 ? MOCAP_BAJ_ST_POINT_SINGULAR : 0);
}

template <class H>
int schur_setup(mocap_ctx* ctx, SchurWork& w, const H& m, int64_t N, const double* obs, double huber_px) {
  using M = typename H::Dev;
  static_assert(M::kPar - 6 <= 8, "SchurWork::rank");
  const int C = m.C;
  w.C = C;
  w.q = 0;
  w.sel = m.sel;
  for (int k = 0; k < M::kPar - 6; k++)  // the device's column rule (schur_linearise_kernel)
    if (w.sel >> (k >> 1) & 1u) w.rank[k] = w.q++;
  w.n_c = 6 * (C - 1) + w.q * C;
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
      w.d_cams[s] = c.take<double>((size_t)C * M::kCam);
      w.d_X[s] = c.take<double>(n * 3);
      w.d_L[s] = c.take<double>(n * 6);
      w.d_flags[s] = c.take<int32_t>(n);
    }
    w.d_Jaug[0] = c.take<double>(2 * nJ);  // the two in one run: one fill zeroes both
    w.d_Jaug[1] = w.d_Jaug[0] + nJ;
    w.d_rho = c.take<double>(n);
    w.d_partial = c.take<double>((size_t)w.ksplit * nG);
    w.d_delta = c.take<double>((size_t)w.NP);
    w.d_slab = c.take<double>((size_t)C * M::kBands * w.P * M::kSlab);
    w.d_Xout = c.take<double>(n * 3);
    w.d_part = c.take<int32_t>(n);
    return c.off;
  };
  if (ctx->baj_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%s workspace) failed", H::kSection);
  lay(ctx->baj_ws.ptr);
  auto lay_pin = [&](void* base) {
    Carver c(base);
    for (int s = 0; s < 2; s++) {
      w.h_G[s] = c.take<double>(nG);
      w.h_sums[s] = c.take<double>((size_t)C * M::kBands * M::kSlab);
      w.h_cams[s] = c.take<double>((size_t)C * M::kCam);
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

template <class H>
int schur_upload_cams(mocap_ctx* ctx, SchurWork& w, const H& m, int slot, const double* R, const double* t, const double* state) {
  m.fill_cams(R, t, state, w.h_cams[slot]);
  HIP_TRY(ctx, hipMemcpyAsync(w.d_cams[slot], w.h_cams[slot], sizeof(double) * w.C * H::Dev::kCam, hipMemcpyHostToDevice, ctx->stream));
  return MOCAP_OK;
}

inline SchurArgs schur_args(const SchurWork& w, int slot, double lambda) {
  SchurArgs a{};
  a.C = w.C;
  a.q = w.q;
  a.n_c = w.n_c;
  a.NP = w.NP;
  a.sel = w.sel;
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
template <class H>
int schur_linearise(mocap_ctx* ctx, SchurWork& w, int slot, double lambda, SchurStats& st) {
  using M = typename H::Dev;
  HIP_TRY(ctx, H::launch(schur_args(w, slot, lambda), ctx->stream));
  const int rc = spin_wait(ctx, ctx->ba_event);
  if (rc) return rc;
  st = SchurStats{};
  for (int c = 0; c < w.C; c++) {  // camera order
    const double* s = w.h_sums[slot] + ((size_t)c * M::kBands + (M::kBands - 1)) * M::kSlab + M::kCount;
    st.views += s[1];
    st.down += s[2];
    st.skipped += s[3];
    if (s[1] + s[3] == 0.0) st.camera_unseen = true;
  }
  const double* s0 = w.h_sums[slot] + (size_t)(M::kBands - 1) * M::kSlab + M::kCount;
  st.cost = s0[0];
  st.part = s0[4];
  st.singular = s0[5];
  return MOCAP_OK;
}

// S = U_lambda - sum E^T E, rhs = -g_c + sum E^T z.  G [NP][NP] = [E | z]^T [E | z] (its upper triangle is read), sums the camera
// blocks as csrc/ba_schur.hpp lays them out.  S [n_c][n_c] row-major, rhs [n_c]; plain double loops in the order the header states.
template <class M>
void schur_assemble(const SchurWork& w, const double* G, const double* sums, double lambda, double* S, double* rhs) {
  const int n = w.n_c, C = w.C, NP = w.NP;
  for (int i = 0; i < n * n; i++) S[i] = 0.0;
  for (int i = 0; i < n; i++) rhs[i] = 0.0;
  for (int c = 0; c < C; c++) {
    int idx[M::kPar];  // the block's rows in S; -1 = not an unknown
    for (int k = 0; k < 6; k++) idx[k] = c ? 6 * (c - 1) + k : -1;
    for (int k = 6; k < M::kPar; k++) idx[k] = w.rank[k - 6] < 0 ? -1 : 6 * (C - 1) + w.q * c + w.rank[k - 6];
    for (int i = 0; i < M::kPar; i++) {
      if (idx[i] < 0) continue;
      const double* row = sums + ((size_t)c * M::kBands + M::band_of(i)) * M::kSlab + M::row_off(i);  // U[i][i ..], g[i]
      for (int j = i; j < M::kPar; j++) {
        if (idx[j] < 0) continue;
        const double v = i == j ? row[0] + lambda * row[0] : row[j - i];
        S[idx[i] * n + idx[j]] = v;
        S[idx[j] * n + idx[i]] = v;
      }
      rhs[idx[i]] = -row[M::kPar - i];
    }
  }
  for (int i = 0; i < n; i++) {
    for (int j = i; j < n; j++) {
      const double v = S[i * n + j] - G[(size_t)i * NP + j];
      S[i * n + j] = v;
      S[j * n + i] = v;
    }
    rhs[i] = rhs[i] + G[(size_t)i * NP + n];
  }
}

// the DLT table of the start: P_c = K_c [R_c | t_c], left to right (a lens is ignored)
inline void schur_ptab(int C, const double* K9, const double* R, const double* t, double* P) {
  for (int c = 0; c < C; c++) {
    const double* K = K9 + 9 * c;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 4; j++) {
        const double m0 = j < 3 ? R[9 * c + j] : t[3 * c], m1 = j < 3 ? R[9 * c + 3 + j] : t[3 * c + 1],
                     m2 = j < 3 ? R[9 * c + 6 + j] : t[3 * c + 2];
        P[12 * c + 4 * i + j] = (K[3 * i] * m0 + K[3 * i + 1] * m1) + K[3 * i + 2] * m2;
      }
  }
}

// mocap_ba_*_normal_eq: one linearisation at the caller's cameras and points
template <class H>
int schur_normal_eq(mocap_ctx* ctx, const char* who, H& m, int64_t N, const double* obs, const double* R, const double* t,
                    const double* X, double huber_px, double lambda, double* S, double* rhs, double* cost, double* info) {
  int rc = m.check(ctx, who, N, obs, R, t, huber_px);
  if (rc) return rc;
  if (!X || !S || !rhs) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  if (!(lambda >= 0.0) || !schur_finite(lambda)) return ctx->fail(MOCAP_E_ARG, "%s: lambda must be finite and >= 0", who);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  SchurWork w;
  if ((rc = schur_setup(ctx, w, m, N, obs, huber_px))) return rc;
  std::vector<double> state;
  m.init(state);
  if ((rc = schur_upload_cams(ctx, w, m, 0, R, t, state.data()))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(w.d_X[0], X, sizeof(double) * (size_t)N * 3, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, launch_baj_start(w.C, N, w.d_obs, nullptr, 1, w.d_X[0], w.d_part, ctx->stream));
  SchurStats st;
  if ((rc = schur_linearise<H>(ctx, w, 0, lambda, st))) return rc;
  schur_assemble<typename H::Dev>(w, w.h_G[0], w.h_sums[0], lambda, S, rhs);
  if (cost) *cost = st.cost;
  if (info) {
    for (int i = 0; i < MOCAP_BAJ_INFO; i++) info[i] = 0.0;
    info[2] = info[3] = st.cost;
    info[4] = lambda;
    info[5] = st.part;
    info[6] = (double)N - st.part;
    info[7] = st.down;
    info[8] = (double)(schur_status(st) | (st.skipped > 0.0 ? MOCAP_BAJ_ST_BAD_DEPTH : 0));
  }
  return MOCAP_OK;
}

// mocap_ba_*_solve: the Levenberg-Marquardt loop.  R, t in and out; the intrinsics go in and out through the solver's hooks.
template <class H>
int schur_solve(mocap_ctx* ctx, const char* who, H& m, int64_t N, const double* obs, double* R, double* t, double* X_out,
                double huber_px, double ftol, int max_iter, double* info) {
  int rc = m.check(ctx, who, N, obs, R, t, huber_px);
  if (rc) return rc;
  if (!(ftol >= 0.0) || !schur_finite(ftol)) return ctx->fail(MOCAP_E_ARG, "%s: ftol must be finite and >= 0", who);
  if (max_iter < 1) return ctx->fail(MOCAP_E_ARG, "%s: max_iter must be at least 1", who);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const auto t_begin = std::chrono::steady_clock::now();
  SchurWork w;
  if ((rc = schur_setup(ctx, w, m, N, obs, huber_px))) return rc;
  const int C = w.C, n_c = w.n_c;
  // the current set of cameras on the host, and the trial
  std::vector<double> Rc(R, R + 9 * C), tc(t, t + 3 * C), ic, Rt, tt, it;
  m.init(ic);
  schur_ptab(C, m.K9(), Rc.data(), tc.data(), w.h_Ptab);
  HIP_TRY(ctx, hipMemcpyAsync(w.d_Ptab, w.h_Ptab, sizeof(double) * C * 12, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, launch_baj_start(C, N, w.d_obs, w.d_Ptab, 0, w.d_X[0], w.d_part, ctx->stream));
  int cur = 0;
  if ((rc = schur_upload_cams(ctx, w, m, cur, Rc.data(), tc.data(), ic.data()))) return rc;
  double lambda = 1e-3;
  SchurStats st;
  if ((rc = schur_linearise<H>(ctx, w, cur, lambda, st))) return rc;
  const double cost0 = st.cost, part = st.part;
  double cost = cost0, down = st.down, dev_ms = 0.0;
  int passes = 0, accepted = 0, linearisations = 1;
  uint32_t status = schur_status(st);
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
  std::vector<double> S((size_t)n_c * n_c), rhs(n_c), delta(n_c);
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
    SchurStats tr;
    bool ok = true;
    if (stale) {
      if ((rc = schur_linearise<H>(ctx, w, cur, lambda, st))) return rc;
      linearisations++;
      stale = false;
    }
    schur_assemble<typename H::Dev>(w, w.h_G[cur], w.h_sums[cur], lambda, S.data(), rhs.data());
    if (!baj_chol_solve(n_c, S.data(), rhs.data(), delta.data())) {
      status |= MOCAP_BAJ_ST_SINGULAR;
      ok = false;
    }
    const double lambda_t = lambda / 10.0 > 1e-12 ? lambda / 10.0 : 1e-12;
    if (ok) {
      // the trial cameras
      Rt = Rc;
      tt = tc;
      for (int c = 1; c < C; c++) {
        baj_rotate(delta.data() + 6 * (c - 1), Rt.data() + 9 * c);
        for (int k = 0; k < 3; k++) tt[3 * c + k] = tc[3 * c + k] + delta[6 * (c - 1) + 3 + k];
      }
      ok = m.trial(w, delta.data(), ic, it);
    }
    if (ok) {
      const int trial = 1 - cur;
      if ((rc = schur_upload_cams(ctx, w, m, trial, Rt.data(), tt.data(), it.data()))) return rc;
      for (int i = 0; i < w.NP; i++) w.h_delta[i] = i < n_c ? delta[i] : 0.0;
      HIP_TRY(ctx, hipMemcpyAsync(w.d_delta, w.h_delta, sizeof(double) * w.NP, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, launch_schur_backsub(schur_args(w, cur, lambda), w.d_delta, w.d_X[trial], ctx->stream));
      if ((rc = schur_linearise<H>(ctx, w, trial, lambda_t, tr))) return rc;
      linearisations++;
      ok = schur_finite(tr.cost) && tr.skipped == 0.0 && tr.cost < cost;
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
    ic.swap(it);
    accepted++;
    m.accepted(Rc.data(), tc.data(), ic.data());
    if (before - cost <= ftol * before) break;
  }
  // the gauge: |t_1| as it came
  double scale = 1.0;
  if (run) {
    const double n_in = std::sqrt((t[3] * t[3] + t[4] * t[4]) + t[5] * t[5]);
    const double n_out = std::sqrt((tc[3] * tc[3] + tc[4] * tc[4]) + tc[5] * tc[5]);
    if (schur_finite(n_in) && schur_finite(n_out) && n_in > 0.0 && n_out > 0.0) scale = n_in / n_out;
  }
  if (X_out) {
    HIP_TRY(ctx, launch_baj_finish(N, w.d_X[cur], w.d_part, scale, w.d_Xout, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(X_out, w.d_Xout, sizeof(double) * (size_t)N * 3, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (run && accepted > 0) {  // camera 0's pose is never written
    for (int c = 1; c < C; c++) {
      for (int k = 0; k < 9; k++) R[9 * c + k] = Rc[9 * c + k];
      for (int k = 0; k < 3; k++) t[3 * c + k] = tc[3 * c + k] * scale;
    }
    m.write_back(w, ic.data());
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

}  // namespace mocap
