// ba_lens_capi.hip -- the "lens calibration" section of include/mocap_core.h: argument checks, the workspace, the Levenberg-Marquardt
// loop around the kernels of ba_lens.hip, and mocap_undistort_points.  The loop is the joint bundle adjustment's (ba_joint_capi.hip)
// with a wider camera block: per iteration the host sees the reduced camera system (S down, delta up) and solves it with the dense
// Cholesky of tr_host.cpp; everything per point stays on the context's stream.  The workspace is the joint bundle adjustment's
// (ctx->baj_ws, ctx->baj_pin): one context is one serialised caller, the two solvers never run at the same time.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/mocap_core.h"
#include "ba_joint.hpp"
#include "ba_lens.hpp"
#include "ctx.hpp"
#include "tr_host.hpp"

using namespace mocap;

static_assert(kBalMaxCameras == MOCAP_BAL_MAX_CAMERAS && kBalMaxPoints == MOCAP_BAL_MAX_POINTS && kBalNewton == MOCAP_UNDISTORT_NEWTON,
              "ba_lens.hpp mirrors include/mocap_core.h");

namespace {

constexpr uint32_t kAllFlags = MOCAP_BAL_FOCAL | MOCAP_BAL_CENTRE | MOCAP_BAL_RADIAL | MOCAP_BAL_TANGENTIAL;

struct BalWork {
  int C = 0, q = 0, n_c = 0, NP = 0, ksplit = 1;
  int rank[8] = {-1, -1, -1, -1, -1, -1, -1, -1};  // per intrinsic (fx fy cx cy k1 k2 p1 p2): its place among the camera's q unknowns, -1 = fixed
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
struct BalStats {
  double cost = 0.0, views = 0.0, down = 0.0, skipped = 0.0, part = 0.0, singular = 0.0;
  bool camera_unseen = false;
};

// every camera's K plain with fx, fy finite and > 0, cx, cy finite; every coefficient finite
int lens_tables_check(mocap_ctx* ctx, const char* who, int C, const double* K, const double* dist) {
  for (int c = 0; c < C; c++) {
    const double* k = K + 9 * c;
    if (k[1] != 0.0 || k[3] != 0.0 || k[6] != 0.0 || k[7] != 0.0 || k[8] != 1.0)
      return ctx->fail(MOCAP_E_ARG, "%s: the intrinsic matrix of camera %d is not [[fx,0,cx],[0,fy,cy],[0,0,1]]", who, c);
    if (!bal_finite(k[0]) || !(k[0] > 0.0) || !bal_finite(k[4]) || !(k[4] > 0.0) || !bal_finite(k[2]) || !bal_finite(k[5]))
      return ctx->fail(MOCAP_E_ARG, "%s: fx, fy of camera %d must be finite and > 0, cx, cy finite", who, c);
    for (int i = 0; i < 5; i++)
      if (!bal_finite(dist[5 * c + i])) return ctx->fail(MOCAP_E_ARG, "%s: a distortion coefficient of camera %d is not finite", who, c);
  }
  return MOCAP_OK;
}

int bal_check(mocap_ctx* ctx, const char* who, int C, int64_t N, const double* obs, const double* R, const double* t, const double* K,
              const double* dist, uint32_t flags, double huber_px) {
  if (C < 2 || C > MOCAP_BAL_MAX_CAMERAS) return ctx->fail(MOCAP_E_ARG, "%s: %d cameras, 2 .. %d are taken", who, C, MOCAP_BAL_MAX_CAMERAS);
  if (N < 1 || N > MOCAP_BAL_MAX_POINTS) return ctx->fail(MOCAP_E_ARG, "%s: N must be 1 .. %d", who, MOCAP_BAL_MAX_POINTS);
  if (flags & ~kAllFlags) return ctx->fail(MOCAP_E_ARG, "%s: unknown flag bits 0x%x", who, flags);
  if (flags && C < 3) return ctx->fail(MOCAP_E_ARG, "%s: intrinsics as unknowns need at least 3 cameras", who);
  if (!obs || !R || !t || !K || !dist) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  if (!(huber_px >= 0.0) || !bal_finite(huber_px)) return ctx->fail(MOCAP_E_ARG, "%s: huber_px must be finite and >= 0", who);
  return lens_tables_check(ctx, who, C, K, dist);
}

int bal_setup(mocap_ctx* ctx, BalWork& w, int C, int64_t N, const double* obs, uint32_t flags, double huber_px) {
  w.C = C;
  w.q = 0;
  w.sel = flags;
  for (int f = 0; f < 4; f++)
    if (flags & (1u << f)) {
      w.rank[2 * f] = w.q++;
      w.rank[2 * f + 1] = w.q++;
    }
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
      w.d_cams[s] = c.take<double>((size_t)C * kBalCam);
      w.d_X[s] = c.take<double>(n * 3);
      w.d_L[s] = c.take<double>(n * 6);
      w.d_flags[s] = c.take<int32_t>(n);
    }
    w.d_Jaug[0] = c.take<double>(2 * nJ);  // the two in one run: one fill zeroes both
    w.d_Jaug[1] = w.d_Jaug[0] + nJ;
    w.d_rho = c.take<double>(n);
    w.d_partial = c.take<double>((size_t)w.ksplit * nG);
    w.d_delta = c.take<double>((size_t)w.NP);
    w.d_slab = c.take<double>((size_t)C * kBalBands * w.P * kBalSlab);
    w.d_Xout = c.take<double>(n * 3);
    w.d_part = c.take<int32_t>(n);
    return c.off;
  };
  if (ctx->baj_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(lens calibration workspace) failed");
  lay(ctx->baj_ws.ptr);
  auto lay_pin = [&](void* base) {
    Carver c(base);
    for (int s = 0; s < 2; s++) {
      w.h_G[s] = c.take<double>(nG);
      w.h_sums[s] = c.take<double>((size_t)C * kBalBands * kBalSlab);
      w.h_cams[s] = c.take<double>((size_t)C * kBalCam);
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

// the camera table of one set: R, t as given, in [C][9] = fx fy cx cy k1 k2 p1 p2 k3
void bal_fill_cams(int C, const double* R, const double* t, const double* in, double* out) {
  for (int c = 0; c < C; c++) {
    double* o = out + kBalCam * c;
    for (int k = 0; k < 9; k++) o[k] = R[9 * c + k];
    for (int k = 0; k < 3; k++) o[9 + k] = t[3 * c + k];
    for (int k = 0; k < 9; k++) o[12 + k] = in[9 * c + k];
    o[21] = o[22] = o[23] = 0.0;
  }
}

int bal_upload_cams(mocap_ctx* ctx, BalWork& w, int slot, const double* R, const double* t, const double* in) {
  bal_fill_cams(w.C, R, t, in, w.h_cams[slot]);
  HIP_TRY(ctx, hipMemcpyAsync(w.d_cams[slot], w.h_cams[slot], sizeof(double) * w.C * kBalCam, hipMemcpyHostToDevice, ctx->stream));
  return MOCAP_OK;
}

BalArgs bal_args(const BalWork& w, int slot, double lambda) {
  BalArgs a{};
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
int bal_linearise(mocap_ctx* ctx, BalWork& w, int slot, double lambda, BalStats& st) {
  HIP_TRY(ctx, launch_bal_linearise(bal_args(w, slot, lambda), ctx->stream));
  const int rc = spin_wait(ctx, ctx->ba_event);
  if (rc) return rc;
  st = BalStats{};
  for (int c = 0; c < w.C; c++) {  // camera order
    const double* s = w.h_sums[slot] + ((size_t)c * kBalBands + (kBalBands - 1)) * kBalSlab + kBalCount;
    st.views += s[1];
    st.down += s[2];
    st.skipped += s[3];
    if (s[1] + s[3] == 0.0) st.camera_unseen = true;
  }
  const double* s0 = w.h_sums[slot] + (size_t)(kBalBands - 1) * kBalSlab + kBalCount;
  st.cost = s0[0];
  st.part = s0[4];
  st.singular = s0[5];
  return MOCAP_OK;
}

// S = U_lambda - sum E^T E, rhs = -g_c + sum E^T z, as baj_assemble states it, for 14-parameter camera blocks cut into row bands
void bal_assemble(const BalWork& w, const double* G, const double* sums, double lambda, double* S, double* rhs) {
  const int n = w.n_c, C = w.C, NP = w.NP;
  for (int i = 0; i < n * n; i++) S[i] = 0.0;
  for (int i = 0; i < n; i++) rhs[i] = 0.0;
  for (int c = 0; c < C; c++) {
    int idx[kBalPar];  // the block's rows in S; -1 = not an unknown
    for (int k = 0; k < 6; k++) idx[k] = c ? 6 * (c - 1) + k : -1;
    for (int k = 0; k < 8; k++) idx[6 + k] = w.rank[k] < 0 ? -1 : 6 * (C - 1) + w.q * c + w.rank[k];
    for (int i = 0; i < kBalPar; i++) {
      if (idx[i] < 0) continue;
      const double* row = sums + ((size_t)c * kBalBands + bal_band_of(i)) * kBalSlab + bal_row_off(i);  // U[i][i ..], g[i]
      for (int j = i; j < kBalPar; j++) {
        if (idx[j] < 0) continue;
        const double v = i == j ? row[0] + lambda * row[0] : row[j - i];
        S[idx[i] * n + idx[j]] = v;
        S[idx[j] * n + idx[i]] = v;
      }
      rhs[idx[i]] = -row[kBalPar - i];
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

// the DLT table of the start: P_c = K_c [R_c | t_c], left to right (the lens is ignored)
void bal_ptab(int C, const double* K9, const double* R, const double* t, double* P) {
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

// fx fy cx cy k1 k2 p1 p2 k3 per camera from K [C][9], dist [C][5]
void bal_intrinsics(int C, const double* K, const double* dist, std::vector<double>& in) {
  in.resize((size_t)9 * C);
  for (int c = 0; c < C; c++) {
    double* o = in.data() + 9 * c;
    o[0] = K[9 * c];
    o[1] = K[9 * c + 4];
    o[2] = K[9 * c + 2];
    o[3] = K[9 * c + 5];
    for (int k = 0; k < 5; k++) o[4 + k] = dist[5 * c + k];
  }
}

uint32_t bal_status(const BalStats& st) {
  return (st.camera_unseen ? MOCAP_BAL_ST_CAMERA_UNSEEN : 0) | (st.part == 0.0 ? MOCAP_BAL_ST_NO_POINTS : 0) |
         (st.singular > 0.0 ? MOCAP_BAL_ST_POINT_SINGULAR : 0);
}

int undistort_check(mocap_ctx* ctx, const char* who, int C, int64_t N, const void* in, const double* K, const double* dist, const void* out) {
  if (C < 1 || C > MOCAP_BAL_MAX_CAMERAS) return ctx->fail(MOCAP_E_ARG, "%s: %d cameras, 1 .. %d are taken", who, C, MOCAP_BAL_MAX_CAMERAS);
  if (N < 1 || N > MOCAP_UNDISTORT_MAX_POINTS) return ctx->fail(MOCAP_E_ARG, "%s: N must be 1 .. %d", who, MOCAP_UNDISTORT_MAX_POINTS);
  if (!in || !K || !dist || !out) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  return lens_tables_check(ctx, who, C, K, dist);
}

// K and dist behind each other in the joint bundle adjustment's workspace, on the stream; -> device pointers
int undistort_tables(mocap_ctx* ctx, int C, size_t extra, const double* K, const double* dist, double** d_K, double** d_dist, double** d_extra) {
  auto lay = [&](void* base) {
    Carver c(base);
    *d_K = c.take<double>((size_t)C * 9);
    *d_dist = c.take<double>((size_t)C * 5);
    *d_extra = c.take<double>(extra);
    return c.off;
  };
  if (ctx->baj_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(undistortion workspace) failed");
  lay(ctx->baj_ws.ptr);
  // (pageable sources: the copies are complete, as far as the caller's memory goes, when the calls return)
  HIP_TRY(ctx, hipMemcpyAsync(*d_K, K, sizeof(double) * C * 9, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(*d_dist, dist, sizeof(double) * C * 5, hipMemcpyHostToDevice, ctx->stream));
  return MOCAP_OK;
}

}  // namespace

extern "C" int mocap_ba_lens_normal_eq(mocap_ctx* ctx, int C, int64_t N, const double* obs, const double* R, const double* t,
                                       const double* K, const double* dist, const double* X, uint32_t flags, double huber_px,
                                       double lambda, double* S, double* rhs, double* cost, double* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const char* who = "mocap_ba_lens_normal_eq";
  int rc = bal_check(ctx, who, C, N, obs, R, t, K, dist, flags, huber_px);
  if (rc) return rc;
  if (!X || !S || !rhs) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  if (!(lambda >= 0.0) || !bal_finite(lambda)) return ctx->fail(MOCAP_E_ARG, "%s: lambda must be finite and >= 0", who);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  BalWork w;
  if ((rc = bal_setup(ctx, w, C, N, obs, flags, huber_px))) return rc;
  std::vector<double> in;
  bal_intrinsics(C, K, dist, in);
  if ((rc = bal_upload_cams(ctx, w, 0, R, t, in.data()))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(w.d_X[0], X, sizeof(double) * (size_t)N * 3, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, launch_baj_start(C, N, w.d_obs, nullptr, 1, w.d_X[0], w.d_part, ctx->stream));
  BalStats st;
  if ((rc = bal_linearise(ctx, w, 0, lambda, st))) return rc;
  bal_assemble(w, w.h_G[0], w.h_sums[0], lambda, S, rhs);
  if (cost) *cost = st.cost;
  if (info) {
    for (int i = 0; i < MOCAP_BAL_INFO; i++) info[i] = 0.0;
    info[2] = info[3] = st.cost;
    info[4] = lambda;
    info[5] = st.part;
    info[6] = (double)N - st.part;
    info[7] = st.down;
    info[8] = (double)(bal_status(st) | (st.skipped > 0.0 ? MOCAP_BAL_ST_BAD_DEPTH : 0));
  }
  return MOCAP_OK;
}

extern "C" int mocap_ba_lens_solve(mocap_ctx* ctx, int C, int64_t N, const double* obs, double* R, double* t, double* K, double* dist,
                                   double* X_out, uint32_t flags, double huber_px, double ftol, int max_iter, double* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const char* who = "mocap_ba_lens_solve";
  int rc = bal_check(ctx, who, C, N, obs, R, t, K, dist, flags, huber_px);
  if (rc) return rc;
  if (!(ftol >= 0.0) || !bal_finite(ftol)) return ctx->fail(MOCAP_E_ARG, "%s: ftol must be finite and >= 0", who);
  if (max_iter < 1) return ctx->fail(MOCAP_E_ARG, "%s: max_iter must be at least 1", who);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const auto t_begin = std::chrono::steady_clock::now();
  BalWork w;
  if ((rc = bal_setup(ctx, w, C, N, obs, flags, huber_px))) return rc;
  const int n_c = w.n_c, q = w.q;
  // the current set on the host, and the trial
  std::vector<double> Rc(R, R + 9 * C), tc(t, t + 3 * C), ic, Rt, tt, it;
  bal_intrinsics(C, K, dist, ic);
  bal_ptab(C, K, Rc.data(), tc.data(), w.h_Ptab);
  HIP_TRY(ctx, hipMemcpyAsync(w.d_Ptab, w.h_Ptab, sizeof(double) * C * 12, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, launch_baj_start(C, N, w.d_obs, w.d_Ptab, 0, w.d_X[0], w.d_part, ctx->stream));
  int cur = 0;
  if ((rc = bal_upload_cams(ctx, w, cur, Rc.data(), tc.data(), ic.data()))) return rc;
  double lambda = 1e-3;
  BalStats st;
  if ((rc = bal_linearise(ctx, w, cur, lambda, st))) return rc;
  const double cost0 = st.cost, part = st.part;
  double cost = cost0, down = st.down, dev_ms = 0.0;
  int passes = 0, accepted = 0, linearisations = 1;
  uint32_t status = bal_status(st);
  const bool run = !(status & (MOCAP_BAL_ST_NO_POINTS | MOCAP_BAL_ST_CAMERA_UNSEEN));
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
      status |= MOCAP_BAL_ST_LAMBDA;
      break;
    }
    if (passes >= max_iter) {
      status |= MOCAP_BAL_ST_MAX_ITER;
      break;
    }
    passes++;
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    BalStats tr;
    bool ok = true;
    if (stale) {
      if ((rc = bal_linearise(ctx, w, cur, lambda, st))) return rc;
      linearisations++;
      stale = false;
    }
    bal_assemble(w, w.h_G[cur], w.h_sums[cur], lambda, S.data(), rhs.data());
    if (!baj_chol_solve(n_c, S.data(), rhs.data(), delta.data())) {
      status |= MOCAP_BAL_ST_SINGULAR;
      ok = false;
    }
    const double lambda_t = lambda / 10.0 > 1e-12 ? lambda / 10.0 : 1e-12;
    if (ok) {
      // the trial cameras
      Rt = Rc;
      tt = tc;
      it = ic;
      for (int c = 1; c < C; c++) {
        baj_rotate(delta.data() + 6 * (c - 1), Rt.data() + 9 * c);
        for (int k = 0; k < 3; k++) tt[3 * c + k] = tc[3 * c + k] + delta[6 * (c - 1) + 3 + k];
      }
      for (int c = 0; c < C; c++)
        for (int k = 0; k < 8; k++) {
          if (w.rank[k] < 0) continue;
          const double d = delta[6 * (C - 1) + q * c + w.rank[k]];
          it[9 * c + k] = k < 2 ? ic[9 * c + k] * (1.0 + d) : ic[9 * c + k] + d;
          if (k < 2 && !(it[9 * c + k] > 0.0)) ok = false;  // a focal length that is not > 0: the trial is rejected unseen
        }
    }
    if (ok) {
      const int trial = 1 - cur;
      if ((rc = bal_upload_cams(ctx, w, trial, Rt.data(), tt.data(), it.data()))) return rc;
      for (int i = 0; i < w.NP; i++) w.h_delta[i] = i < n_c ? delta[i] : 0.0;
      HIP_TRY(ctx, hipMemcpyAsync(w.d_delta, w.h_delta, sizeof(double) * w.NP, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, launch_bal_backsub(bal_args(w, cur, lambda), w.d_delta, w.d_X[trial], ctx->stream));
      if ((rc = bal_linearise(ctx, w, trial, lambda_t, tr))) return rc;
      linearisations++;
      ok = bal_finite(tr.cost) && tr.skipped == 0.0 && tr.cost < cost;
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
    if (tr.singular > 0.0) status |= MOCAP_BAL_ST_POINT_SINGULAR;
    cur = 1 - cur;
    lambda = lambda_t;
    Rc.swap(Rt);
    tc.swap(tt);
    ic.swap(it);
    accepted++;
    if (before - cost <= ftol * before) break;
  }
  // the gauge: |t_1| as it came
  double scale = 1.0;
  if (run) {
    const double n_in = std::sqrt((t[3] * t[3] + t[4] * t[4]) + t[5] * t[5]);
    const double n_out = std::sqrt((tc[3] * tc[3] + tc[4] * tc[4]) + tc[5] * tc[5]);
    if (bal_finite(n_in) && bal_finite(n_out) && n_in > 0.0 && n_out > 0.0) scale = n_in / n_out;
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
    for (int c = 0; c < C; c++) {  // only what was an unknown is written; k3 never
      if (w.rank[0] >= 0) K[9 * c] = ic[9 * c], K[9 * c + 4] = ic[9 * c + 1];
      if (w.rank[2] >= 0) K[9 * c + 2] = ic[9 * c + 2], K[9 * c + 5] = ic[9 * c + 3];
      if (w.rank[4] >= 0) dist[5 * c] = ic[9 * c + 4], dist[5 * c + 1] = ic[9 * c + 5];
      if (w.rank[6] >= 0) dist[5 * c + 2] = ic[9 * c + 6], dist[5 * c + 3] = ic[9 * c + 7];
    }
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

extern "C" int mocap_undistort_points_dev(mocap_ctx* ctx, int C, int64_t N, const double* d_in, const double* K, const double* dist,
                                          double* d_out) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = undistort_check(ctx, "mocap_undistort_points_dev", C, N, d_in, K, dist, d_out);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  double *d_K, *d_dist, *d_none;
  if ((rc = undistort_tables(ctx, C, 0, K, dist, &d_K, &d_dist, &d_none))) return rc;
  HIP_TRY(ctx, launch_bal_undistort(C, N, d_in, d_K, d_dist, d_out, ctx->stream));
  return ctx->mark_enqueued();
}

extern "C" int mocap_undistort_points(mocap_ctx* ctx, int C, int64_t N, const double* in, const double* K, const double* dist,
                                      double* out) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = undistort_check(ctx, "mocap_undistort_points", C, N, in, K, dist, out);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)N * C * 2;
  double *d_K, *d_dist, *d_io;
  if ((rc = undistort_tables(ctx, C, 2 * n, K, dist, &d_K, &d_dist, &d_io))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(d_io, in, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, launch_bal_undistort(C, N, d_io, d_K, d_dist, d_io + n, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(out, d_io + n, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
