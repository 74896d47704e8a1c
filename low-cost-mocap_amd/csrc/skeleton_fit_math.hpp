// skeleton_fit_math.hpp -- the arithmetic of "skeleton fit" (include/mocap_core.h): a point's terms of a body's 6 x 6 block, the
// block and the coupling to the parent as the solve reads them, L D L^T of a 6 x 6 block without pivoting, its solve, and the pose
// update.  Plain C++ (no intrinsics, no fused operation), the same text for the kernels (csrc/skeleton_fit.hip) and for a host
// compiler.  Every expression is written in the order the header pins; both sides compile with -ffp-contract=off.  Every loop has
// constant bounds and every index is a constant once unrolled: in a kernel the blocks live in registers.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SKM_HD __host__ __device__ __forceinline__
#else
#define SKM_HD inline
#endif

namespace mocap {

// the lower triangle of a symmetric 6 x 6 block, packed by rows: (0,0) (1,0) (1,1) (2,0) ...
SKM_HD constexpr int sk_tri(int i, int k) { return i * (i + 1) / 2 + k; }

SKM_HD bool sk_finite(double x) { return x - x == 0.0; }

// y = R p (R row-major 3 x 3)
SKM_HD void sk_rot(const double* R, const double* p, double* y) {
#pragma unroll
  for (int i = 0; i < 3; i++) y[i] = (R[3 * i] * p[0] + R[3 * i + 1] * p[1]) + R[3 * i + 2] * p[2];
}

// The terms of a body before they become a block: S (00 01 02 11 12 22) = sum w (|y|^2 I - y y^T), m = sum w y, s = sum w,
// g = sum w J^T r with J = [-[y]x, I].
struct SkOwn {
  double S[6], m[3], s, g[6];
};

SKM_HD void sk_own_zero(SkOwn& o) {
#pragma unroll
  for (int e = 0; e < 6; e++) o.S[e] = o.g[e] = 0.0;
  o.m[0] = o.m[1] = o.m[2] = o.s = 0.0;
}

// one point: y = the point relative to the body's origin (world axes), r its residual, w its weight
SKM_HD void sk_own_add(SkOwn& o, const double* y, const double* r, double w) {
  o.S[0] = o.S[0] + w * (y[1] * y[1] + y[2] * y[2]);
  o.S[1] = o.S[1] - w * (y[0] * y[1]);
  o.S[2] = o.S[2] - w * (y[0] * y[2]);
  o.S[3] = o.S[3] + w * (y[0] * y[0] + y[2] * y[2]);
  o.S[4] = o.S[4] - w * (y[1] * y[2]);
  o.S[5] = o.S[5] + w * (y[0] * y[0] + y[1] * y[1]);
  o.m[0] = o.m[0] + w * y[0];
  o.m[1] = o.m[1] + w * y[1];
  o.m[2] = o.m[2] + w * y[2];
  o.s = o.s + w;
  o.g[0] = o.g[0] + w * (y[1] * r[2] - y[2] * r[1]);
  o.g[1] = o.g[1] + w * (y[2] * r[0] - y[0] * r[2]);
  o.g[2] = o.g[2] + w * (y[0] * r[1] - y[1] * r[0]);
  o.g[3] = o.g[3] + w * r[0];
  o.g[4] = o.g[4] + w * r[1];
  o.g[5] = o.g[5] + w * r[2];
}

// the body's own block, its diagonal damped: H_ii + lam H_ii
SKM_HD void sk_own_block(const SkOwn& o, double lam, double* H) {
  const double tt = o.s + lam * o.s;
  H[0] = o.S[0] + lam * o.S[0];
  H[1] = o.S[1];
  H[2] = o.S[3] + lam * o.S[3];
  H[3] = o.S[2];
  H[4] = o.S[4];
  H[5] = o.S[5] + lam * o.S[5];
  H[6] = 0.0;
  H[7] = o.m[2];
  H[8] = -o.m[1];
  H[9] = tt;
  H[10] = -o.m[2];
  H[11] = 0.0;
  H[12] = o.m[0];
  H[13] = 0.0;
  H[14] = tt;
  H[15] = o.m[1];
  H[16] = -o.m[0];
  H[17] = 0.0;
  H[18] = 0.0;
  H[19] = 0.0;
  H[20] = tt;
}

// The coupling of a body to its parent through their joint, as 16 numbers: G [3][3] = -(w (sum (yc . yp) I - yp yc^T)),
// u = w sum yc, v = w sum yp, n = w * (the number of virtual points); the sums run over the joint's one or two points.
struct SkUp {
  double G[9], u[3], v[3], n;
};

SKM_HD void sk_up_point(const double* yc, const double* yp, double* E) {
  const double dot = (yc[0] * yp[0] + yc[1] * yp[1]) + yc[2] * yp[2];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) E[3 * i + k] = i == k ? dot - yp[i] * yc[k] : -(yp[i] * yc[k]);
}

SKM_HD void sk_up_make(SkUp& c, const double* yc0, const double* yp0, const double* yc1, const double* yp1, bool hinge, double w) {
  double E0[9], E1[9];
  sk_up_point(yc0, yp0, E0);
  sk_up_point(yc1, yp1, E1);
#pragma unroll
  for (int e = 0; e < 9; e++) c.G[e] = -(w * (hinge ? E0[e] + E1[e] : E0[e]));
#pragma unroll
  for (int i = 0; i < 3; i++) {
    c.u[i] = w * (hinge ? yc0[i] + yc1[i] : yc0[i]);
    c.v[i] = w * (hinge ? yp0[i] + yp1[i] : yp0[i]);
  }
  c.n = w * (hinge ? 2.0 : 1.0);
}

// the coupling as the 6 x 6 block C [child's rows][parent's columns]
SKM_HD void sk_up_block(const SkUp& c, double C[6][6]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      C[i][k] = c.G[3 * i + k];
      C[3 + i][3 + k] = i == k ? -c.n : 0.0;
    }
  C[0][3] = 0.0;
  C[0][4] = c.u[2];
  C[0][5] = -c.u[1];
  C[1][3] = -c.u[2];
  C[1][4] = 0.0;
  C[1][5] = c.u[0];
  C[2][3] = c.u[1];
  C[2][4] = -c.u[0];
  C[2][5] = 0.0;
  C[3][0] = 0.0;
  C[3][1] = -c.v[2];
  C[3][2] = c.v[1];
  C[4][0] = c.v[2];
  C[4][1] = 0.0;
  C[4][2] = -c.v[0];
  C[5][0] = -c.v[1];
  C[5][1] = c.v[0];
  C[5][2] = 0.0;
}

// A = L D L^T without pivoting, refine_lm.hpp's rule at 6 x 6: t_ik = a_ik - sum_{m < k} l_im t_km, l_ik = t_ik / d_k,
// d_i = a_ii - sum_{k < i} l_ik t_ik, every sum subtracted term by term in ascending index.  -> every pivot finite and > 0
SKM_HD bool sk_ldl6(const double* A, double* L, double* d) {
  double T[15];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double di = A[sk_tri(i, i)];
#pragma unroll
    for (int k = 0; k < i; k++) {
      double t = A[sk_tri(i, k)];
#pragma unroll
      for (int m = 0; m < k; m++) t = t - L[sk_tri(i - 1, m)] * T[sk_tri(k - 1, m)];
      T[sk_tri(i - 1, k)] = t;
      L[sk_tri(i - 1, k)] = t / d[k];
      di = di - L[sk_tri(i - 1, k)] * t;
    }
    d[i] = di;
    ok = ok && sk_finite(di) && di > 0.0;
  }
  return ok;
}

// x = A^-1 b from the factors (L's strict lower triangle packed by rows: row i at sk_tri(i - 1, 0))
SKM_HD void sk_solve6(const double* L, const double* d, const double* b, double* x) {
  double u[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) s = s - L[sk_tri(i - 1, k)] * u[k];
    u[i] = s;
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double s = u[i] / d[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) s = s - L[sk_tri(k - 1, i)] * x[k];
    x[i] = s;
  }
}

// q <- q_d (x) q normalised, q_d = (1, omega / 2) normalised; t <- t + tau.  No trigonometric function.
SKM_HD void sk_update(const double* q, const double* t, const double* delta, double* qn, double* tn) {
  const double hx = delta[0] * 0.5, hy = delta[1] * 0.5, hz = delta[2] * 0.5;
  const double nd = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
  const double dw = 1.0 / nd, dx = hx / nd, dy = hy / nd, dz = hz / nd;
  const double w = ((dw * q[0] - dx * q[1]) - dy * q[2]) - dz * q[3];
  const double x = ((dw * q[1] + dx * q[0]) + dy * q[3]) - dz * q[2];
  const double y = ((dw * q[2] - dx * q[3]) + dy * q[0]) + dz * q[1];
  const double z = ((dw * q[3] + dx * q[2]) - dy * q[1]) + dz * q[0];
  const double nq = sqrt(((w * w + x * x) + y * y) + z * z);
  qn[0] = w / nq;
  qn[1] = x / nq;
  qn[2] = y / nq;
  qn[3] = z / nq;
  tn[0] = t[0] + delta[3];
  tn[1] = t[1] + delta[4];
  tn[2] = t[2] + delta[5];
}

}  // namespace mocap
