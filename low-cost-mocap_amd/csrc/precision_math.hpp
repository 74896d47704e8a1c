// precision_math.hpp -- the arithmetic of the "predicted precision" section of include/mocap_core.h: at a point x, the normal matrix
// H = sum over the views of J^T J of the reprojection error (the expressions of csrc/refine_lm.hpp's rlm_eval, without observations),
// its eigen-decomposition by cyclic Jacobi, and sigma_px^2 H^-1 read out as principal standard deviations, the worst axis and the
// packed covariance.  Plain C++ with constant loop bounds (no intrinsics, no fused operation), the same text for the kernels
// (csrc/precision.hip) and for a host compiler: tests/native/precision_check.cpp runs it on the CPU and the tests compare its bits
// with tests/precision_reference.py.  Every expression is written in the order the header pins; both sides compile with
// -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#include "refine_lm.hpp"

#if defined(__HIPCC__)
#define PM_UNROLL _Pragma("unroll")
#else
#define PM_UNROLL
#endif

namespace mocap {

constexpr int kPmSweeps = 16;  // mirrored from include/mocap_core.h (MOCAP_PM_SWEEPS)
// the info word of a point (MOCAP_PM_*)
constexpr int kPmOk = 1, kPmBadPoint = 2, kPmBadView = 4, kPmFewViews = 8, kPmDegenerate = 16;

// by-visibility rule: the picture and the depth range, as doubles
struct PmVis {
  double width, height, near, far;
};

struct PmPoint {
  int info, n_views;
  uint64_t seen;  // bit c: camera c was a view
  double sig_max;  // = sig[2], or NaN
  double sig[3], axis[3], cov[6];
};

RLM_HD double pm_nan() {
  union {
    uint64_t u;
    double d;
  } q;
  q.u = 0x7ff8000000000000ull;
  return q.d;
}

// camera c is a view by visibility (a NaN fails every comparison)
RLM_HD bool pm_visible(const PmVis& v, double w, double pu, double pv) {
  return rlm_finite(w) && w > 0.0 && w >= v.near && w <= v.far && pu >= 0.0 && pu < v.width && pv >= 0.0 && pv < v.height;
}

// H over the views, ascending camera order, the u row before the v row.  named(c): the caller names camera c (read only with
// by_vis false).  -> the views' count, their bits, and whether a named view had a depth that is not finite or <= 0.
template <class Tab, class Named>
RLM_HD void pm_normal(int C, Tab P0, bool by_vis, Named&& named, const PmVis& vis, double X, double Y, double Z, double (&H)[6], int& n,
                      uint64_t& seen, bool& bad_view) {
  for (int e = 0; e < 6; e++) H[e] = 0.0;
  n = 0;
  seen = 0;
  bad_view = false;
  for (int c = 0; c < C; c++) {
    const Tab P = P0 + 12 * c;
    const double a = P[0] * X + P[1] * Y + P[2] * Z + P[3];
    const double b = P[4] * X + P[5] * Y + P[6] * Z + P[7];
    const double w = P[8] * X + P[9] * Y + P[10] * Z + P[11];
    const double pu = a / w, pv = b / w;
    const bool view = by_vis ? pm_visible(vis, w, pu, pv) : named(c);
    if (!view) continue;
    n++;
    seen |= 1ull << c;
    bad_view = bad_view || !(rlm_finite(w) && w > 0.0);
    const double ju0 = (P[0] - pu * P[8]) / w, ju1 = (P[1] - pu * P[9]) / w, ju2 = (P[2] - pu * P[10]) / w;
    const double jv0 = (P[4] - pv * P[8]) / w, jv1 = (P[5] - pv * P[9]) / w, jv2 = (P[6] - pv * P[10]) / w;
    H[0] = H[0] + ju0 * ju0;
    H[0] = H[0] + jv0 * jv0;
    H[1] = H[1] + ju0 * ju1;
    H[1] = H[1] + jv0 * jv1;
    H[2] = H[2] + ju0 * ju2;
    H[2] = H[2] + jv0 * jv2;
    H[3] = H[3] + ju1 * ju1;
    H[3] = H[3] + jv1 * jv1;
    H[4] = H[4] + ju1 * ju2;
    H[4] = H[4] + jv1 * jv2;
    H[5] = H[5] + ju2 * ju2;
    H[5] = H[5] + jv2 * jv2;
  }
}

// Cyclic Jacobi on the symmetric 3 x 3 A by the rules the header spells out for Horn's matrix (csrc/rb_pose.hpp; csrc/jacobi6.hpp at
// 6 x 6): the pairs 01, 02, 12, the skip rule, the g rule from the fifth sweep, V from the identity.  The loops over p, q, k have
// constant bounds and are unrolled, so A and V are registers; the sweep loop is not.
RLM_HD void pm_jacobi3(double (&A)[3][3], double (&V)[3][3]) {
  PM_UNROLL
  for (int i = 0; i < 3; i++) {
    PM_UNROLL
    for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
  }
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int sweep = 0; sweep < kPmSweeps; sweep++) {
    const double off = (fabs(A[0][1]) + fabs(A[0][2])) + fabs(A[1][2]);
    if (off == 0.0) break;
    PM_UNROLL
    for (int p = 0; p < 2; p++) {
      PM_UNROLL
      for (int q = p + 1; q < 3; q++) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double g = 100.0 * fabs(apq);
        if (sweep > 3 && fabs(A[p][p]) + g == fabs(A[p][p]) && fabs(A[q][q]) + g == fabs(A[q][q])) {
          A[p][q] = A[q][p] = 0.0;
          continue;
        }
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        t = theta < 0.0 ? -t : t;
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
        A[p][p] = A[p][p] - t * apq;
        A[q][q] = A[q][q] + t * apq;
        A[p][q] = A[q][p] = 0.0;
        PM_UNROLL
        for (int k = 0; k < 3; k++) {
          if (k != p && k != q) {
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = A[p][k] = cs * akp - sn * akq;
            A[k][q] = A[q][k] = sn * akp + cs * akq;
          }
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = cs * vkp - sn * vkq;
          V[k][q] = sn * vkp + cs * vkq;
        }
      }
    }
  }
}

// compare and swap of the sorting network: eigenvalue i above eigenvalue j (strictly) -> both and their columns of V change places
RLM_HD void pm_cas(double (&lam)[3], double (&V)[3][3], int i, int j) {
  const bool sw = lam[i] > lam[j];
  const double li = lam[i], lj = lam[j];
  lam[i] = sw ? lj : li;
  lam[j] = sw ? li : lj;
  PM_UNROLL
  for (int k = 0; k < 3; k++) {
    const double vi = V[k][i], vj = V[k][j];
    V[k][i] = sw ? vj : vi;
    V[k][j] = sw ? vi : vj;
  }
}

// One point, whole: the views, H, the decomposition, the outputs.  Every field of `o` is written.
template <class Tab, class Named>
RLM_HD void pm_point(int C, Tab P, bool by_vis, Named&& named, const PmVis& vis, double sigma_px, double X, double Y, double Z, PmPoint& o) {
  double H[6];
  bool bad_view;
  pm_normal(C, P, by_vis, named, vis, X, Y, Z, H, o.n_views, o.seen, bad_view);
  int flags = 0;
  if (!(rlm_finite(X) && rlm_finite(Y) && rlm_finite(Z))) flags |= kPmBadPoint;
  if (bad_view) flags |= kPmBadView;
  if (o.n_views < 2) flags |= kPmFewViews;
  const double qnan = pm_nan();
  o.sig_max = qnan;
  for (int e = 0; e < 3; e++) o.sig[e] = o.axis[e] = qnan;
  for (int e = 0; e < 6; e++) o.cov[e] = qnan;
  if (!flags) {
    double A[3][3] = {{H[0], H[1], H[2]}, {H[1], H[3], H[4]}, {H[2], H[4], H[5]}}, V[3][3];
    pm_jacobi3(A, V);
    double lam[3] = {A[0][0], A[1][1], A[2][2]};
    pm_cas(lam, V, 0, 1);
    pm_cas(lam, V, 1, 2);
    pm_cas(lam, V, 0, 1);
    const bool ok = rlm_finite(lam[0]) && rlm_finite(lam[1]) && rlm_finite(lam[2]) && !(lam[0] <= lam[2] * 0x1p-40);
    if (!ok) {
      flags = kPmDegenerate;
    } else {
      flags = kPmOk;
      o.sig[0] = sigma_px / sqrt(lam[2]);
      o.sig[1] = sigma_px / sqrt(lam[1]);
      o.sig[2] = sigma_px / sqrt(lam[0]);
      o.sig_max = o.sig[2];
      // the axis of the largest sig = the eigenvector of the smallest eigenvalue; its largest component (the first among equals) > 0
      const double v0 = V[0][0], v1 = V[1][0], v2 = V[2][0];
      double big = v0;
      big = fabs(v1) > fabs(big) ? v1 : big;
      big = fabs(v2) > fabs(big) ? v2 : big;
      const bool neg = big < 0.0;
      o.axis[0] = neg ? -v0 : v0;
      o.axis[1] = neg ? -v1 : v1;
      o.axis[2] = neg ? -v2 : v2;
      const double s2 = sigma_px * sigma_px;
      const double d0 = s2 / lam[0], d1 = s2 / lam[1], d2 = s2 / lam[2];
      int e = 0;
      PM_UNROLL
      for (int i = 0; i < 3; i++) {
        PM_UNROLL
        for (int j = i; j < 3; j++) o.cov[e++] = ((V[i][0] * V[j][0]) * d0 + (V[i][1] * V[j][1]) * d1) + (V[i][2] * V[j][2]) * d2;
      }
    }
  }
  o.info = flags;
}

}  // namespace mocap
