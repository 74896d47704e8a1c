// resect_math.hpp -- the arithmetic of the "camera resection" section of include/mocap_core.h: the counter-based sampler, Grunert's
// three-point solver, the per-view residual with its inlier rule, the rows of the normal equations and the Levenberg-Marquardt step.
// Plain C++ (no intrinsics, no fused operation), the same text for the kernels (csrc/resect.hip), for the host's share of the loop
// (csrc/resect_capi.hip) and for a host compiler: tests/native/resect_check.cpp runs it on the CPU and the tests compare it with
// tests/resection_reference.py.  Every expression is written in the order the header pins; all sides compile with -ffp-contract=off.
// The three-point solver calls acos, cos, cbrt and sqrt: its results depend on the math library and are compared by residual.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif

namespace mocap {

constexpr int kRsMaxPoints = 131072, kRsMaxHyp = 4096, kRsInfo = 12;  // mirrored from include/mocap_core.h (MOCAP_RESECT_*)
constexpr int kRsOk = 0, kRsTooFew = 1, kRsNoModel = 2;                // the status of info
// what one linearisation sums over the inliers: H (upper triangle, row-major: 00 01 .. 05 11 .. 55) | g [6] | cost | inliers |
// inliers that are not in front of the camera | the cost's change against a base pose (rs_delta_row; 0 without one)
constexpr int kRsSums = 31, kRsCost = 27, kRsCount = 28, kRsBehind = 29, kRsDelta = 30;

// finite: neither NaN nor an infinity (x - x is 0 for every finite x and NaN otherwise)
RS_HD bool rs_finite(double x) { return x - x == 0.0; }

// ------------------------------------------------------------------------------------------------------------------ sampler
// splitmix64: the output for the state z
RS_HD uint64_t rs_mix(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// the three distinct rows (indices into the valid rows, n >= 3) of hypothesis h: draw k is rs_mix(seed + (3 h + k) * golden)
RS_HD void rs_sample(uint64_t seed, uint32_t h, uint32_t n, int (&idx)[3]) {
  const uint64_t g = 0x9e3779b97f4a7c15ull;
  const uint64_t r0 = rs_mix(seed + (uint64_t)(3 * (uint64_t)h) * g);
  const uint64_t r1 = rs_mix(seed + (uint64_t)(3 * (uint64_t)h + 1) * g);
  const uint64_t r2 = rs_mix(seed + (uint64_t)(3 * (uint64_t)h + 2) * g);
  const int i0 = (int)(r0 % n);
  int i1 = (int)(r1 % (n - 1));
  if (i1 >= i0) i1++;
  int i2 = (int)(r2 % (n - 2));
  const int lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
  if (i2 >= lo) i2++;
  if (i2 >= hi) i2++;
  idx[0] = i0;
  idx[1] = i1;
  idx[2] = i2;
}

// ---------------------------------------------------------------------------------------------------- residual, inlier rule
// pose: R row-major [9] | t [3];  k4: fx, fy, cx, cy.  x = R X + t;  du = (fx (x0 / x2) + cx) - u, dv likewise.
struct RsView {
  double P[3], x[3], xn, yn, du, dv, s2;
};

template <class Pose, class K4>
RS_HD void rs_view(Pose pose, K4 k4, double X0, double X1, double X2, double u, double v, RsView& w) {
  w.P[0] = (pose[0] * X0 + pose[1] * X1) + pose[2] * X2;
  w.P[1] = (pose[3] * X0 + pose[4] * X1) + pose[5] * X2;
  w.P[2] = (pose[6] * X0 + pose[7] * X1) + pose[8] * X2;
  w.x[0] = w.P[0] + pose[9];
  w.x[1] = w.P[1] + pose[10];
  w.x[2] = w.P[2] + pose[11];
  w.xn = w.x[0] / w.x[2];
  w.yn = w.x[1] / w.x[2];
  w.du = (k4[0] * w.xn + k4[2]) - u;
  w.dv = (k4[1] * w.yn + k4[3]) - v;
  w.s2 = w.du * w.du + w.dv * w.dv;
}

// inlier iff x2 > 0 and du^2 + dv^2 < thr2 (strict; a NaN anywhere is an outlier)
RS_HD bool rs_inlier(const RsView& w, double thr2) { return w.x[2] > 0.0 && w.s2 < thr2; }

// the contribution of one inlier row to the sums of a linearisation (left increment R <- exp([w]x) R, t <- t + dt):
//   a0 = fx / x2, b1 = fy / x2, a2 = -(a0 xn), b2 = -(b1 yn)            (the rows of D = d(du, dv)/dx: (a0, 0, a2), (0, b1, b2))
//   Ju = (a2 P1, a0 P2 - a2 P0, -(a0 P1), a0, 0, a2),  Jv = (b2 P1 - b1 P2, -(b2 P0), b1 P0, 0, b1, b2)        ([-D [P]x | D], P = R X)
//   H_ij = Ju_i Ju_j + Jv_i Jv_j,  g_i = Ju_i du + Jv_i dv,  cost = du du + dv dv
template <class K4>
RS_HD void rs_jacobian(const RsView& w, K4 k4, double (&Ju)[6], double (&Jv)[6]) {
  const double a0 = k4[0] / w.x[2], b1 = k4[1] / w.x[2];
  const double a2 = -(a0 * w.xn), b2 = -(b1 * w.yn);
  Ju[0] = a2 * w.P[1];
  Ju[1] = a0 * w.P[2] - a2 * w.P[0];
  Ju[2] = -(a0 * w.P[1]);
  Ju[3] = a0;
  Ju[4] = 0.0;
  Ju[5] = a2;
  Jv[0] = b2 * w.P[1] - b1 * w.P[2];
  Jv[1] = -(b2 * w.P[0]);
  Jv[2] = b1 * w.P[0];
  Jv[3] = 0.0;
  Jv[4] = b1;
  Jv[5] = b2;
}

template <class K4>
RS_HD void rs_row(const RsView& w, K4 k4, double (&s)[kRsSums]) {
  double Ju[6], Jv[6];
  rs_jacobian(w, k4, Ju, Jv);
  int e = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 6; i++) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = i; j < 6; j++) s[e++] = Ju[i] * Ju[j] + Jv[i] * Jv[j];
  }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 6; i++) s[21 + i] = Ju[i] * w.du + Jv[i] * w.dv;
  s[kRsCost] = w.s2;
  s[kRsCount] = 1.0;
  s[kRsBehind] = (rs_finite(w.x[2]) && w.x[2] > 0.0) ? 0.0 : 1.0;
  s[kRsDelta] = 0.0;
}

// s2(trial) - s2(base) of one row, from the INCREMENT inc = (G [9] | dt [3]), G = exp([w]x) - I: the trial pose is (R + G R, t + dt).
// The two costs agree to fifteen digits near the minimum, and their difference is lost when each is rounded on its own; taken from
// the increment it keeps its own sixteen digits, so "strictly lower" is decided by the arithmetic's signal, not by its noise.
//   dx_i = ((G_i0 P0 + G_i1 P1) + G_i2 P2) + dt_i  (P = R X of the base);  x2' = x2 + dx2;
//   dxn = (dx0 - xn dx2) / x2',  dyn = (dx1 - yn dx2) / x2';  ddu = fx dxn, ddv = fy dyn;
//   delta = ddu (2 du + ddu) + ddv (2 dv + ddv)
template <class Inc, class K4>
RS_HD double rs_delta_row(const RsView& base, Inc inc, K4 k4) {
  const double dx0 = ((inc[0] * base.P[0] + inc[1] * base.P[1]) + inc[2] * base.P[2]) + inc[9];
  const double dx1 = ((inc[3] * base.P[0] + inc[4] * base.P[1]) + inc[5] * base.P[2]) + inc[10];
  const double dx2 = ((inc[6] * base.P[0] + inc[7] * base.P[1]) + inc[8] * base.P[2]) + inc[11];
  const double x2t = base.x[2] + dx2;
  const double dxn = (dx0 - base.xn * dx2) / x2t, dyn = (dx1 - base.yn * dx2) / x2t;
  const double ddu = k4[0] * dxn, ddv = k4[1] * dyn;
  return ddu * (2.0 * base.du + ddu) + ddv * (2.0 * base.dv + ddv);
}

// ------------------------------------------------------------------------------------------------- Levenberg-Marquardt step
// (H + lam diag H) delta = -g by a dense Cholesky, row by row, sums left to right.  false: a pivot is not finite or not > 0.
RS_HD bool rs_lm_step(const double* s, double lam, double (&delta)[6]) {
  double A[6][6], L[6][6];
  int e = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) {
      A[i][j] = s[e];
      A[j][i] = s[e];
      e++;
    }
  for (int i = 0; i < 6; i++) A[i][i] = A[i][i] + lam * A[i][i];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j <= i; j++) {
      double acc = A[i][j];
      for (int k = 0; k < j; k++) acc = acc - L[i][k] * L[j][k];
      if (i == j) {
        if (!(rs_finite(acc) && acc > 0.0)) return false;
        L[i][i] = sqrt(acc);
      } else {
        L[i][j] = acc / L[j][j];
      }
    }
  double y[6];
  for (int i = 0; i < 6; i++) {
    double acc = -s[21 + i];
    for (int k = 0; k < i; k++) acc = acc - L[i][k] * y[k];
    y[i] = acc / L[i][i];
  }
  for (int i = 5; i >= 0; i--) {
    double acc = y[i];
    for (int k = i + 1; k < 6; k++) acc = acc - L[k][i] * delta[k];
    delta[i] = acc / L[i][i];
  }
  return true;
}

// pose <- (exp([w]x) R, t + dt), delta = (w, dt).  Rodrigues: th2 = w.w, th = sqrt(th2); a = sin th / th, b = (1 - cos th) / th2
// (th < 1e-8: a = 1 - th2 / 6, b = 0.5 - th2 / 24);  G = a [w]x + b [w]x^2, E = I + G;  R' = E R, each entry (E_i0 R_0j + E_i1 R_1j) +
// E_i2 R_2j.  inc = (G | dt), the increment rs_delta_row takes.
RS_HD void rs_apply(const double* pose, const double (&d)[6], double* out, double* inc) {
  const double wx = d[0], wy = d[1], wz = d[2];
  const double th2 = (wx * wx + wy * wy) + wz * wz;
  const double th = sqrt(th2);
  double a, b;
  if (th < 1e-8) {
    a = 1.0 - th2 / 6.0;
    b = 0.5 - th2 / 24.0;
  } else {
    a = sin(th) / th;
    b = (1.0 - cos(th)) / th2;
  }
  inc[0] = -(b * (wy * wy + wz * wz));
  inc[1] = b * (wx * wy) - a * wz;
  inc[2] = b * (wx * wz) + a * wy;
  inc[3] = b * (wx * wy) + a * wz;
  inc[4] = -(b * (wx * wx + wz * wz));
  inc[5] = b * (wy * wz) - a * wx;
  inc[6] = b * (wx * wz) - a * wy;
  inc[7] = b * (wy * wz) + a * wx;
  inc[8] = -(b * (wx * wx + wy * wy));
  for (int k = 0; k < 3; k++) inc[9 + k] = d[3 + k];
  double E[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) E[i][j] = i == j ? 1.0 + inc[3 * i + j] : inc[3 * i + j];
  double R[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = (E[i][0] * pose[j] + E[i][1] * pose[3 + j]) + E[i][2] * pose[6 + j];
  for (int k = 0; k < 9; k++) out[k] = R[k];
  for (int k = 0; k < 3; k++) out[9 + k] = pose[9 + k] + d[3 + k];
}

// One round of the schedule: Levenberg-Marquardt from `pose` over a fixed inlier mask.  lin(pose, base, inc, sums) linearises at
// `pose`: without a base the mask becomes the classification at that pose first; with one (`pose` is the trial base + inc) the sums
// carry the cost's change against the base over the mask.  Returns false when lin fails (its error is the caller's).
//   lam_0 = 1e-3.  A trial is ACCEPTED iff the Cholesky factor exists, its cost is finite and strictly lower -- the sum of rs_delta_row
//   over the mask is < 0 -- and no inlier of the mask lies behind the camera: lam <- max(lam / 10, 1e-12); otherwise lam <- 10 lam.  The round ends after max_iter accepted steps, after
//   a trial whose step has |w|_inf <= 1e-12 and |dt|_inf <= 1e-12 (1 + |t|_inf) (taken first if it is accepted), when lam > 1e12, or at
//   once when the mask is empty.
struct RsRound {
  double cost;
  int accepted, linearisations;
};

template <class Lin>
inline bool rs_round(double* pose, int max_iter, Lin&& lin, RsRound& out, const double* start = nullptr) {
  double cur[kRsSums], tr[kRsSums], trial[12], inc[12], delta[6];
  out.accepted = 0;
  out.linearisations = 1;
  if (start) {  // the linearisation at `pose` with the mask of `pose`, made by the caller
    for (int k = 0; k < kRsSums; k++) cur[k] = start[k];
  } else if (!lin(pose, nullptr, nullptr, cur)) {
    return false;
  }
  double lam = 1e-3;
  while (out.accepted < max_iter && cur[kRsCount] > 0.0 && lam <= 1e12) {
    if (!rs_lm_step(cur, lam, delta)) {
      lam = lam * 10.0;
      continue;
    }
    rs_apply(pose, delta, trial, inc);
    if (!lin(trial, pose, inc, tr)) return false;
    out.linearisations++;
    double wmax = 0.0, dmax = 0.0, tmax = 0.0;
    for (int k = 0; k < 3; k++) {
      wmax = fabs(delta[k]) > wmax ? fabs(delta[k]) : wmax;
      dmax = fabs(delta[3 + k]) > dmax ? fabs(delta[3 + k]) : dmax;
      tmax = fabs(pose[9 + k]) > tmax ? fabs(pose[9 + k]) : tmax;
    }
    const bool small = wmax <= 1e-12 && dmax <= 1e-12 * (1.0 + tmax);
    const bool take = rs_finite(tr[kRsCost]) && tr[kRsBehind] == 0.0 && tr[kRsDelta] < 0.0;
    if (take) {
      for (int k = 0; k < 12; k++) pose[k] = trial[k];
      for (int k = 0; k < kRsSums; k++) cur[k] = tr[k];
      lam = lam / 10.0 > 1e-12 ? lam / 10.0 : 1e-12;
      out.accepted++;
    } else {
      lam = lam * 10.0;
    }
    if (small) break;
  }
  out.cost = cur[kRsCost];
  return true;
}

// ------------------------------------------------------------------------------------------------------ three-point solver
// the largest real root of x^3 + a1 x^2 + a2 x + a3 (Cardano / Viete), then two Newton steps
RS_HD double rs_cubic_largest(double a1, double a2, double a3) {
  const double Q = (a1 * a1 - 3.0 * a2) / 9.0, R = (2.0 * a1 * a1 * a1 - 9.0 * a1 * a2 + 27.0 * a3) / 54.0;
  const double d = Q * Q * Q - R * R;
  double x;
  if (d > 0.0) {  // three real roots: the largest is the one with the smallest angle
    const double theta = acos(R / sqrt(Q * Q * Q));
    const double pi = 3.14159265358979323846;
    x = -2.0 * sqrt(Q) * cos((theta + 2.0 * pi) / 3.0) - a1 / 3.0;
    const double x2 = -2.0 * sqrt(Q) * cos((theta + 4.0 * pi) / 3.0) - a1 / 3.0;
    const double x0 = -2.0 * sqrt(Q) * cos(theta / 3.0) - a1 / 3.0;
    x = x2 > x ? x2 : x;
    x = x0 > x ? x0 : x;
  } else {
    double e = cbrt(sqrt(-d) + fabs(R));
    if (R > 0.0) e = -e;
    x = e == 0.0 ? -a1 / 3.0 : (e + Q / e) - a1 / 3.0;
  }
  for (int it = 0; it < 2; it++) {
    const double f = ((x + a1) * x + a2) * x + a3, fp = (3.0 * x + 2.0 * a1) * x + a2;
    if (fp != 0.0 && rs_finite(f / fp)) x = x - f / fp;
  }
  return x;
}

// the real roots of A4 x^4 + .. + A0 (Ferrari on the resolvent cubic), each polished by two Newton steps on the quartic
RS_HD int rs_quartic(const double (&A)[5], double (&x)[4]) {
  double big = 0.0;
  for (int i = 0; i < 5; i++) big = fabs(A[i]) > big ? fabs(A[i]) : big;
  if (!(rs_finite(big) && fabs(A[4]) > 1e-14 * big)) return 0;
  const double b = A[3] / A[4], c = A[2] / A[4], d = A[1] / A[4], e = A[0] / A[4];
  // x = y - b / 4:  y^4 + p y^2 + q y + r
  const double b2 = b * b;
  const double p = c - 0.375 * b2;
  const double q = (d - 0.5 * (b * c)) + 0.125 * (b2 * b);
  const double r = ((e - 0.25 * (b * d)) + 0.0625 * (b2 * c)) - (3.0 / 256.0) * (b2 * b2);
  double y[4];
  int n = 0;
  // resolvent: m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 = 0, m > 0;  (y^2 + p / 2 + m)^2 = (s y - q / (2 s))^2, s = sqrt(2 m)
  const double m = rs_cubic_largest(p, 0.25 * (p * p) - r, -0.125 * (q * q));
  const double scale = fabs(p) > 1.0 ? fabs(p) : 1.0;
  if (!(m > 1e-14 * scale)) {  // q = 0: a quadratic in y^2
    const double disc = p * p - 4.0 * r;
    if (!(disc >= 0.0)) return 0;
    const double sq = sqrt(disc);
    const double z[2] = {0.5 * (-p + sq), 0.5 * (-p - sq)};
    for (int k = 0; k < 2; k++)
      if (z[k] >= 0.0) {
        y[n++] = sqrt(z[k]);
        y[n++] = -sqrt(z[k]);
      }
  } else {
    const double s = sqrt(2.0 * m), h = 0.5 * p + m, k = q / (2.0 * s);
    const double d1 = s * s - 4.0 * (h + k);  // y^2 - s y + (h + k)
    if (d1 >= 0.0) {
      const double sq = sqrt(d1);
      y[n++] = 0.5 * (s + sq);
      y[n++] = 0.5 * (s - sq);
    }
    const double d2 = s * s - 4.0 * (h - k);  // y^2 + s y + (h - k)
    if (d2 >= 0.0) {
      const double sq = sqrt(d2);
      y[n++] = 0.5 * (-s + sq);
      y[n++] = 0.5 * (-s - sq);
    }
  }
  for (int i = 0; i < n; i++) {
    double v = y[i] - 0.25 * b;
    for (int it = 0; it < 2; it++) {
      const double f = (((A[4] * v + A[3]) * v + A[2]) * v + A[1]) * v + A[0];
      const double fp = ((4.0 * A[4] * v + 3.0 * A[3]) * v + 2.0 * A[2]) * v + A[1];
      if (fp != 0.0 && rs_finite(f / fp)) v = v - f / fp;
    }
    x[i] = v;
  }
  return n;
}

// the orthonormal triad of a point triple as columns: e1 along 1 -> 2, e3 = e1 x (1 -> 3) normalised, e2 = e3 x e1
RS_HD bool rs_triad(const double* p1, const double* p2, const double* p3, double (&T)[3][3]) {
  double a[3], c[3];
  for (int k = 0; k < 3; k++) {
    a[k] = p2[k] - p1[k];
    c[k] = p3[k] - p1[k];
  }
  const double na = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  if (!(na > 0.0)) return false;
  const double e1[3] = {a[0] / na, a[1] / na, a[2] / na};
  double e3[3] = {e1[1] * c[2] - e1[2] * c[1], e1[2] * c[0] - e1[0] * c[2], e1[0] * c[1] - e1[1] * c[0]};
  const double n3 = sqrt((e3[0] * e3[0] + e3[1] * e3[1]) + e3[2] * e3[2]);
  if (!(n3 > 0.0)) return false;
  for (int k = 0; k < 3; k++) e3[k] = e3[k] / n3;
  const double e2[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
  for (int k = 0; k < 3; k++) {
    T[k][0] = e1[k];
    T[k][1] = e2[k];
    T[k][2] = e3[k];
  }
  return true;
}

// Grunert's solver.  P: the three world points [3][3];  uv: their pixels [3][2];  k4: fx, fy, cx, cy.  poses [4][12] (R | t), returns
// how many.  Zero for a sample that is collinear or near-coincident: the triangle's squared area (2 x) <= 1e-12 of b^2 c^2, or a side
// of squared length <= 1e-18 of the longest.
template <class K4>
RS_HD int rs_p3p(const double (&P)[3][3], const double (&uv)[3][2], K4 k4, double* poses) {
  double j[3][3];
  for (int i = 0; i < 3; i++) {
    const double x = (uv[i][0] - k4[2]) / k4[0], y = (uv[i][1] - k4[3]) / k4[1];
    const double nn = sqrt((x * x + y * y) + 1.0);
    j[i][0] = x / nn;
    j[i][1] = y / nn;
    j[i][2] = 1.0 / nn;
  }
  double a2 = 0.0, b2 = 0.0, c2 = 0.0;
  for (int k = 0; k < 3; k++) {
    a2 = a2 + (P[1][k] - P[2][k]) * (P[1][k] - P[2][k]);
    b2 = b2 + (P[0][k] - P[2][k]) * (P[0][k] - P[2][k]);
    c2 = c2 + (P[0][k] - P[1][k]) * (P[0][k] - P[1][k]);
  }
  double longest = a2 > b2 ? a2 : b2;
  longest = c2 > longest ? c2 : longest;
  if (!(rs_finite(longest) && a2 > 1e-18 * longest && b2 > 1e-18 * longest && c2 > 1e-18 * longest)) return 0;
  {
    const double e[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
    const double f[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    const double cr[3] = {e[1] * f[2] - e[2] * f[1], e[2] * f[0] - e[0] * f[2], e[0] * f[1] - e[1] * f[0]};
    const double area2 = (cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2];
    if (!(area2 > 1e-12 * (b2 * c2))) return 0;
  }
  const double ca = (j[1][0] * j[2][0] + j[1][1] * j[2][1]) + j[1][2] * j[2][2];
  const double cb = (j[0][0] * j[2][0] + j[0][1] * j[2][1]) + j[0][2] * j[2][2];
  const double cg = (j[0][0] * j[1][0] + j[0][1] * j[1][1]) + j[0][2] * j[1][2];
  const double q = (a2 - c2) / b2, p = (a2 + c2) / b2, rc = c2 / b2, ra = a2 / b2;
  const double ca2 = ca * ca, cb2 = cb * cb, cg2 = cg * cg;
  double A[5];
  A[4] = (q - 1.0) * (q - 1.0) - 4.0 * rc * ca2;
  A[3] = 4.0 * ((q * (1.0 - q) * cb - (1.0 - p) * ca * cg) + 2.0 * rc * ca2 * cb);
  A[2] = 2.0 * (((((q * q - 1.0) + 2.0 * q * q * cb2) + 2.0 * ((b2 - c2) / b2) * ca2) - 4.0 * p * ca * cb * cg) + 2.0 * ((b2 - a2) / b2) * cg2);
  A[1] = 4.0 * ((-(q * (1.0 + q)) * cb + 2.0 * ra * cg2 * cb) - (1.0 - p) * ca * cg);
  A[0] = (1.0 + q) * (1.0 + q) - 4.0 * ra * cg2;
  double roots[4];
  const int nr = rs_quartic(A, roots);
  const double b = sqrt(b2);
  double Tw[3][3];
  if (!rs_triad(P[0], P[1], P[2], Tw)) return 0;
  int n = 0;
  for (int r = 0; r < nr; r++) {
    const double v = roots[r];
    if (!(v > 0.0)) continue;
    const double den = 2.0 * (cg - v * ca);
    if (den == 0.0) continue;
    const double u = ((((q - 1.0) * v * v - 2.0 * q * cb * v) + 1.0) + q) / den;
    if (!(u > 0.0)) continue;
    const double w = (1.0 + v * v) - 2.0 * v * cb;
    if (!(w > 0.0)) continue;
    const double s1 = b / sqrt(w), s2 = u * s1, s3 = v * s1;
    const double Q1[3] = {s1 * j[0][0], s1 * j[0][1], s1 * j[0][2]};
    const double Q2[3] = {s2 * j[1][0], s2 * j[1][1], s2 * j[1][2]};
    const double Q3[3] = {s3 * j[2][0], s3 * j[2][1], s3 * j[2][2]};
    double Tc[3][3];
    if (!rs_triad(Q1, Q2, Q3, Tc)) continue;
    double* o = poses + 12 * n;
    bool ok = true;
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) {
        o[3 * i + k] = (Tc[i][0] * Tw[k][0] + Tc[i][1] * Tw[k][1]) + Tc[i][2] * Tw[k][2];
        ok = ok && rs_finite(o[3 * i + k]);
      }
    for (int i = 0; i < 3; i++) {
      o[9 + i] = Q1[i] - ((o[3 * i] * P[0][0] + o[3 * i + 1] * P[0][1]) + o[3 * i + 2] * P[0][2]);
      ok = ok && rs_finite(o[9 + i]);
    }
    if (ok) n++;
  }
  return n;
}

}  // namespace mocap
