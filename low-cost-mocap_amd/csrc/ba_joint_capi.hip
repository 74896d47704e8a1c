// ba_joint_capi.hip -- the "joint bundle adjustment" section of include/mocap_core.h: what this solver's cameras are (16 doubles, one
// focal scale per camera as the only intrinsic unknown, K from mocap_set_cameras) for the loop of csrc/ba_schur_host.hpp.
#include <mutex>

#include "ba_joint.hpp"
#include "ba_schur_host.hpp"

using namespace mocap;

static_assert(kBajMaxCameras == MOCAP_BAJ_MAX_CAMERAS && kBajMaxPoints == MOCAP_BAJ_MAX_POINTS, "ba_joint.hpp mirrors include/mocap_core.h");

namespace {

struct BajSolver {
  using Dev = BajModel;
  static constexpr const char* kSection = "joint bundle adjustment";
  static hipError_t launch(const SchurArgs& a, hipStream_t stream) { return launch_baj_linearise(a, stream); }

  mocap_ctx* ctx;
  double* fscale;  // [C] in and out with MOCAP_BAJ_FOCAL
  uint32_t flags;
  int C = 0;
  uint32_t sel = 0;
  std::vector<double> xprog;

  int check(mocap_ctx*, const char* who, int64_t N, const double* obs, const double* R, const double* t, double huber_px) {
    if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "%s: mocap_set_cameras has not been called", who);
    C = ctx->C;
    if (C < 2 || C > MOCAP_BAJ_MAX_CAMERAS) return ctx->fail(MOCAP_E_ARG, "%s: %d cameras, 2 .. %d are taken", who, C, MOCAP_BAJ_MAX_CAMERAS);
    if (N < 1 || N > MOCAP_BAJ_MAX_POINTS) return ctx->fail(MOCAP_E_ARG, "%s: N must be 1 .. %d", who, MOCAP_BAJ_MAX_POINTS);
    if (flags & ~(uint32_t)MOCAP_BAJ_FOCAL) return ctx->fail(MOCAP_E_ARG, "%s: unknown flag bits 0x%x", who, flags);
    if ((flags & MOCAP_BAJ_FOCAL) && C < 3) return ctx->fail(MOCAP_E_ARG, "%s: MOCAP_BAJ_FOCAL needs at least 3 cameras", who);
    if (!obs || !R || !t || ((flags & MOCAP_BAJ_FOCAL) && !fscale)) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
    if (!(huber_px >= 0.0) || !schur_finite(huber_px)) return ctx->fail(MOCAP_E_ARG, "%s: huber_px must be finite and >= 0", who);
    for (int c = 0; c < C; c++) {
      const double* K = ctx->hK.data() + 9 * c;
      if (K[1] != 0.0 || K[3] != 0.0 || K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0)
        return ctx->fail(MOCAP_E_ARG, "%s: the intrinsic matrix of camera %d is not [[fx,0,cx],[0,fy,cy],[0,0,1]]", who, c);
    }
    sel = flags;  // MOCAP_BAJ_FOCAL is bit 0: parameter 6
    return MOCAP_OK;
  }

  const double* K9() const { return ctx->hK.data(); }

  // the state: one focal scale per camera
  void init(std::vector<double>& s) const {
    s.assign(C, 1.0);
    if (sel)
      for (int c = 0; c < C; c++) s[c] = fscale[c];
  }

  // the pose table of one set: R, t as given, fx = fx0 s, fy = fy0 s
  void fill_cams(const double* R, const double* t, const double* s, double* out) const {
    for (int c = 0; c < C; c++) {
      const double* K = ctx->hK.data() + 9 * c;
      double* o = out + BajModel::kCam * c;
      for (int k = 0; k < 9; k++) o[k] = R[9 * c + k];
      for (int k = 0; k < 3; k++) o[9 + k] = t[3 * c + k];
      o[12] = K[0] * s[c];
      o[13] = K[4] * s[c];
      o[14] = K[2];
      o[15] = K[5];
    }
  }

  bool trial(const SchurWork& w, const double* delta, const std::vector<double>& cur, std::vector<double>& next) const {
    next = cur;
    if (w.q)
      for (int c = 0; c < C; c++) next[c] = cur[c] * (1.0 + delta[6 * (C - 1) + c]);
    return true;
  }

  void accepted(const double* R, const double* t, const double* s) {
    if (!ctx->ba_progress) return;
    xprog.resize(1 + 7 * (C - 1));  // the reference's vector layout [f0, (f_i, rotvec_i, t_i)]
    xprog[0] = ctx->hK[0] * s[0];
    for (int c = 1; c < C; c++) {
      double* x = xprog.data() + 1 + 7 * (c - 1);
      x[0] = ctx->hK[9 * c] * s[c];
      baj_rotvec(R + 9 * c, x + 1);
      for (int k = 0; k < 3; k++) x[4 + k] = t[3 * c + k];
    }
    ctx->ba_progress(xprog.data(), (int)xprog.size(), ctx->ba_progress_user);
  }

  void write_back(const SchurWork& w, const double* s) const {
    if (w.q)
      for (int c = 0; c < C; c++) fscale[c] = s[c];
  }
};

}  // namespace

extern "C" int mocap_ba_joint_normal_eq(mocap_ctx* ctx, int64_t N, const double* obs, const double* R, const double* t,
                                        const double* fscale, const double* X, uint32_t flags, double huber_px, double lambda,
                                        double* S, double* rhs, double* cost, double* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BajSolver m{ctx, const_cast<double*>(fscale), flags};  // (read only: nothing is written back from one linearisation)
  return schur_normal_eq(ctx, "mocap_ba_joint_normal_eq", m, N, obs, R, t, X, huber_px, lambda, S, rhs, cost, info);
}

extern "C" int mocap_ba_joint_solve(mocap_ctx* ctx, int64_t N, const double* obs, double* R, double* t, double* fscale, double* X_out,
                                    uint32_t flags, double huber_px, double ftol, int max_iter, double* info) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  BajSolver m{ctx, fscale, flags};
  return schur_solve(ctx, "mocap_ba_joint_solve", m, N, obs, R, t, X_out, huber_px, ftol, max_iter, info);
}
