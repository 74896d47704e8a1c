// ba_lens_capi.hip -- the "lens calibration" section of include/mocap_core.h: what this solver's cameras are (24 doubles, up to eight
// intrinsic unknowns per camera in pairs, K and dist from the caller) for the loop of csrc/ba_schur_host.hpp, and
// mocap_undistort_points.
#include <mutex>

#include "ba_lens.hpp"
#include "ba_schur_host.hpp"

using namespace mocap;

static_assert(kBalMaxCameras == MOCAP_BAL_MAX_CAMERAS && kBalMaxPoints == MOCAP_BAL_MAX_POINTS && kBalNewton == MOCAP_UNDISTORT_NEWTON,
              "ba_lens.hpp mirrors include/mocap_core.h");

namespace {

constexpr uint32_t kAllFlags = MOCAP_BAL_FOCAL | MOCAP_BAL_CENTRE | MOCAP_BAL_RADIAL | MOCAP_BAL_TANGENTIAL;

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

struct BalSolver {
  using Dev = BalModel;
  static constexpr const char* kSection = "lens calibration";
  static hipError_t launch(const SchurArgs& a, hipStream_t stream) { return launch_bal_linearise(a, stream); }

  int C;
  double *K, *dist;  // [C][9], [C][5] in and out
  uint32_t flags;
  uint32_t sel = 0;

  int check(mocap_ctx* ctx, const char* who, int64_t N, const double* obs, const double* R, const double* t, double huber_px) {
    if (C < 2 || C > MOCAP_BAL_MAX_CAMERAS) return ctx->fail(MOCAP_E_ARG, "%s: %d cameras, 2 .. %d are taken", who, C, MOCAP_BAL_MAX_CAMERAS);
    if (N < 1 || N > MOCAP_BAL_MAX_POINTS) return ctx->fail(MOCAP_E_ARG, "%s: N must be 1 .. %d", who, MOCAP_BAL_MAX_POINTS);
    if (flags & ~kAllFlags) return ctx->fail(MOCAP_E_ARG, "%s: unknown flag bits 0x%x", who, flags);
    if (flags && C < 3) return ctx->fail(MOCAP_E_ARG, "%s: intrinsics as unknowns need at least 3 cameras", who);
    if (!obs || !R || !t || !K || !dist) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
    if (!(huber_px >= 0.0) || !bal_finite(huber_px)) return ctx->fail(MOCAP_E_ARG, "%s: huber_px must be finite and >= 0", who);
    sel = flags;  // MOCAP_BAL_* bits: the pairs fx fy | cx cy | k1 k2 | p1 p2 = parameters 6 ..
    return lens_tables_check(ctx, who, C, K, dist);
  }

  const double* K9() const { return K; }

  // the state: fx fy cx cy k1 k2 p1 p2 k3 per camera from K [C][9], dist [C][5]
  void init(std::vector<double>& in) const {
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

  // the camera table of one set: R, t as given, then the state
  void fill_cams(const double* R, const double* t, const double* in, double* out) const {
    for (int c = 0; c < C; c++) {
      double* o = out + kBalCam * c;
      for (int k = 0; k < 9; k++) o[k] = R[9 * c + k];
      for (int k = 0; k < 3; k++) o[9 + k] = t[3 * c + k];
      for (int k = 0; k < 9; k++) o[12 + k] = in[9 * c + k];
      o[21] = o[22] = o[23] = 0.0;
    }
  }

  bool trial(const SchurWork& w, const double* delta, const std::vector<double>& ic, std::vector<double>& it) const {
    bool ok = true;
    it = ic;
    for (int c = 0; c < C; c++)
      for (int k = 0; k < 8; k++) {
        if (w.rank[k] < 0) continue;
        const double d = delta[6 * (C - 1) + w.q * c + w.rank[k]];
        it[9 * c + k] = k < 2 ? ic[9 * c + k] * (1.0 + d) : ic[9 * c + k] + d;
        if (k < 2 && !(it[9 * c + k] > 0.0)) ok = false;  // a focal length that is not > 0: the trial is rejected unseen
      }
    return ok;
  }

  void accepted(const double*, const double*, const double*) const {}

  void write_back(const SchurWork& w, const double* ic) const {
    for (int c = 0; c < C; c++) {  // only what was an unknown is written; k3 never
      if (w.rank[0] >= 0) K[9 * c] = ic[9 * c], K[9 * c + 4] = ic[9 * c + 1];
      if (w.rank[2] >= 0) K[9 * c + 2] = ic[9 * c + 2], K[9 * c + 5] = ic[9 * c + 3];
      if (w.rank[4] >= 0) dist[5 * c] = ic[9 * c + 4], dist[5 * c + 1] = ic[9 * c + 5];
      if (w.rank[6] >= 0) dist[5 * c + 2] = ic[9 * c + 6], dist[5 * c + 3] = ic[9 * c + 7];
    }
  }
};

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
  BalSolver m{C, const_cast<double*>(K), const_cast<double*>(dist), flags};  // (read only: nothing is written back from one linearisation)
  return schur_normal_eq(ctx, "mocap_ba_lens_normal_eq", m, N, obs, R, t, X, huber_px, lambda, S, rhs, cost, info);
}

extern "C" int mocap_ba_lens_solve(mocap_ctx* ctx, int C, int64_t N, const double* obs, double* R, double* t, double* K, double* dist,
                                   double* X_out, uint32_t flags, double huber_px, double ftol, int max_iter, double* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BalSolver m{C, K, dist, flags};
  return schur_solve(ctx, "mocap_ba_lens_solve", m, N, obs, R, t, X_out, huber_px, ftol, max_iter, info);
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
