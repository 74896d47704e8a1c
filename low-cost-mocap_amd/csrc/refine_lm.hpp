// refine_lm.hpp -- the arithmetic of the "point refinement" section of include/mocap_core.h: a fixed number of Levenberg-Marquardt
// steps on one point's reprojection error, each camera with its own P = K [R|t].
// Plain C++ (no intrinsics, no fused operation), the same text for the kernel (csrc/point_refine.hip) and for a host compiler:
// tests/native/refine_check.cpp runs it on the CPU and the tests compare its bits with tests/point_refine_reference.py.  Every
// expression below is written in the order the header pins; both sides compile with -ffp-contract=off.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RLM_HD __host__ __device__ __forceinline__
#else
#define RLM_HD inline
#endif

namespace mocap {

constexpr int kRefineMaxIters = 16;     // mirrored from include/mocap_core.h (MOCAP_REFINE_MAX_ITERS)
// the info word of a point (MOCAP_RF_*)
constexpr int kRfRefined = 1, kRfFewViews = 2, kRfBadIndex = 4, kRfBadObs = 8, kRfBadStart = 16, kRfStepsShift = 8;

// finite: neither NaN nor an infinity (x - x is 0 for every finite x and NaN otherwise)
RLM_HD bool rlm_finite(double x) { return x - x == 0.0; }

// One evaluation: cost, and with `grad` the normal equations H (packed 00 01 02 11 12 22) and g, summed over the views in
// ascending camera order, the u row before the v row.  valid: every depth finite and > 0.
struct RefineEval {
  double cost, H[6], g[3];
  bool valid;
};

// P: the camera table [C][12] (row-major 3 x 4 per camera); obs(c, u, v) -> true when camera c sees the point.
template <class Tab, class Obs>
RLM_HD void rlm_eval(int C, Tab P0, Obs&& obs, double X, double Y, double Z, bool grad, RefineEval& s) {
  s.cost = 0.0;
  for (int e = 0; e < 6; e++) s.H[e] = 0.0;
  s.g[0] = s.g[1] = s.g[2] = 0.0;
  s.valid = true;
  for (int c = 0; c < C; c++) {
    double u, v;
    if (!obs(c, u, v)) continue;
    const Tab P = P0 + 12 * c;
    const double a = P[0] * X + P[1] * Y + P[2] * Z + P[3];
    const double b = P[4] * X + P[5] * Y + P[6] * Z + P[7];
    const double w = P[8] * X + P[9] * Y + P[10] * Z + P[11];
    s.valid = s.valid && rlm_finite(w) && w > 0.0;
    const double pu = a / w, pv = b / w;
    const double ru = pu - u, rv = pv - v;
    s.cost = s.cost + ru * ru;
    s.cost = s.cost + rv * rv;
    if (grad) {
      const double ju0 = (P[0] - pu * P[8]) / w, ju1 = (P[1] - pu * P[9]) / w, ju2 = (P[2] - pu * P[10]) / w;
      const double jv0 = (P[4] - pv * P[8]) / w, jv1 = (P[5] - pv * P[9]) / w, jv2 = (P[6] - pv * P[10]) / w;
      s.H[0] = s.H[0] + ju0 * ju0;
      s.H[0] = s.H[0] + jv0 * jv0;
      s.H[1] = s.H[1] + ju0 * ju1;
      s.H[1] = s.H[1] + jv0 * jv1;
      s.H[2] = s.H[2] + ju0 * ju2;
      s.H[2] = s.H[2] + jv0 * jv2;
      s.H[3] = s.H[3] + ju1 * ju1;
      s.H[3] = s.H[3] + jv1 * jv1;
      s.H[4] = s.H[4] + ju1 * ju2;
      s.H[4] = s.H[4] + jv1 * jv2;
      s.H[5] = s.H[5] + ju2 * ju2;
      s.H[5] = s.H[5] + jv2 * jv2;
      s.g[0] = s.g[0] + ju0 * ru;
      s.g[0] = s.g[0] + jv0 * rv;
      s.g[1] = s.g[1] + ju1 * ru;
      s.g[1] = s.g[1] + jv1 * rv;
      s.g[2] = s.g[2] + ju2 * ru;
      s.g[2] = s.g[2] + jv2 * rv;
    }
  }
}

// `iters` steps from the start X (in: the start, out: the last accepted point).  Returns false, with X as it came, when the
// start is not finite or not valid; otherwise cost is the cost at the returned X and accepted the number of steps taken.
// Accept and reject are selects: every point walks the same instructions, whatever it decides.
template <class Tab, class Obs>
RLM_HD bool refine_lm(int C, Tab P, Obs&& obs, int iters, double (&X)[3], double& cost, int& accepted) {
  RefineEval cur;
  rlm_eval(C, P, obs, X[0], X[1], X[2], iters > 0, cur);
  const bool start_ok = cur.valid && rlm_finite(X[0]) && rlm_finite(X[1]) && rlm_finite(X[2]);
  double x0 = X[0], x1 = X[1], x2 = X[2], lam = 1e-3;
  int acc_n = 0;
  for (int it = 0; it < iters; it++) {
    // A = H with the diagonal H_ii + lam * H_ii; A = L D L^T without pivoting
    const double d0 = cur.H[0] + lam * cur.H[0];
    const double a11 = cur.H[3] + lam * cur.H[3];
    const double a22 = cur.H[5] + lam * cur.H[5];
    const double l10 = cur.H[1] / d0, l20 = cur.H[2] / d0;
    const double d1 = a11 - l10 * cur.H[1];
    const double t21 = cur.H[4] - l20 * cur.H[1];
    const double l21 = t21 / d1;
    const double d2 = (a22 - l20 * cur.H[2]) - l21 * t21;
    const bool piv_ok = rlm_finite(d0) && d0 > 0.0 && rlm_finite(d1) && d1 > 0.0 && rlm_finite(d2) && d2 > 0.0;
    // A delta = -g
    const double z0 = -cur.g[0];
    const double z1 = -cur.g[1] - l10 * z0;
    const double z2 = (-cur.g[2] - l20 * z0) - l21 * z1;
    const double y0 = z0 / d0, y1 = z1 / d1, y2 = z2 / d2;
    const double e2 = y2;
    const double e1 = y1 - l21 * e2;
    const double e0 = (y0 - l10 * e1) - l20 * e2;
    const double t0 = x0 + e0, t1 = x1 + e1, t2 = x2 + e2;
    RefineEval tr;
    rlm_eval(C, P, obs, t0, t1, t2, it + 1 < iters, tr);
    const bool take = piv_ok && tr.valid && tr.cost < cur.cost;
    x0 = take ? t0 : x0;
    x1 = take ? t1 : x1;
    x2 = take ? t2 : x2;
    cur.cost = take ? tr.cost : cur.cost;
    for (int e = 0; e < 6; e++) cur.H[e] = take ? tr.H[e] : cur.H[e];
    for (int e = 0; e < 3; e++) cur.g[e] = take ? tr.g[e] : cur.g[e];
    lam = take ? lam / 10.0 : lam * 10.0;
    acc_n += take ? 1 : 0;
  }
  if (!start_ok) return false;
  X[0] = x0;
  X[1] = x1;
  X[2] = x2;
  cost = cur.cost;
  accepted = acc_n;
  return true;
}

}  // namespace mocap
