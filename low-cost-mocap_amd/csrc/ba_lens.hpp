// ba_lens.hpp -- lens calibration (include/mocap_core.h, "lens calibration"): the lens model and the per-view arithmetic, written once
// for the kernels of csrc/ba_lens.hip and for a stand-alone host program (tests/native/bal_view_host.cpp), and what those kernels are
// instantiated with (the camera model of csrc/ba_schur.hpp).  Every expression is written in the order the header pins; the build compiles
// with -ffp-contract=off.  Without a HIP compiler this file includes nothing of the device and ends before the model: the host program
// compiles it with a plain C++ compiler.
#pragma once
#include <cmath>
#include <cstdint>
#ifdef __HIPCC__
#include "ba_schur.hpp"
#endif

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#ifndef BAL_INLINE
#define BAL_INLINE __host__ __device__ inline __attribute__((always_inline))
#endif

namespace mocap {

constexpr int kBalMaxCameras = 16;    // mirrored from include/mocap_core.h (MOCAP_BAL_MAX_CAMERAS)
constexpr int kBalMaxPoints = 65536;  // ... MOCAP_BAL_MAX_POINTS
constexpr int kBalNewton = 8;         // ... MOCAP_UNDISTORT_NEWTON
constexpr int kBalCam = 24;           // doubles per camera of the table: R [9] row-major, t [3], fx, fy, cx, cy, k1, k2, p1, p2, k3, 3 unused
constexpr int kBalPar = 14;           // a camera's parameters: omega 3, t 3, fx, fy, cx, cy, k1, k2, p1, p2
// The camera block (csrc/ba_schur.hpp: the upper triangle of 14 x 14 row by row, row i = 15 - i values) is cut into four ROW BANDS:
// rows 0-1 (29 values), 2-4 (36), 5-8 (34), 9-13 (20, then the six counters).
constexpr int kBalBands = 4;
constexpr int kBalSlab = 36;
constexpr int kBalCount = 20;

__host__ __device__ constexpr int bal_band_lo(int b) { return b == 0 ? 0 : b == 1 ? 2 : b == 2 ? 5 : 9; }
__host__ __device__ constexpr int bal_band_hi(int b) { return b == 0 ? 2 : b == 1 ? 5 : b == 2 ? 9 : 14; }
__host__ __device__ constexpr int bal_band_of(int i) { return i < 2 ? 0 : i < 5 ? 1 : i < 9 ? 2 : 3; }
// where row i starts inside its band
__host__ __device__ constexpr int bal_row_off(int i) {
  int o = 0;
  for (int r = bal_band_lo(bal_band_of(i)); r < i; r++) o += 15 - r;
  return o;
}

// finite: neither NaN nor an infinity
BAL_INLINE bool bal_finite(double x) { return x - x == 0.0; }

// The lens: where the normalised point (x, y) lands, and the (symmetric) Jacobian of that map.  k = k1 k2 p1 p2 k3.
struct BalLens {
  double r2, kr, xd, yd, Jxx, Jxy, Jyy;
};
template <class Tab>
BAL_INLINE void bal_lens(Tab k, double x, double y, BalLens& o) {
  const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4];
  const double r2 = x * x + y * y;
  const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
  o.r2 = r2;
  o.kr = kr;
  o.xd = (x * kr + ((2.0 * p1) * x) * y) + p2 * (r2 + (2.0 * x) * x);  // synth.distort_pixels, operation by operation
  o.yd = (y * kr + p1 * (r2 + (2.0 * y) * y)) + ((2.0 * p2) * x) * y;
  const double dk = ((3.0 * k3) * r2 + 2.0 * k2) * r2 + k1;
  const double dk2 = 2.0 * dk;
  o.Jxx = (kr + (dk2 * x) * x) + ((2.0 * p1) * y + (6.0 * p2) * x);
  o.Jxy = (dk2 * x) * y + ((2.0 * p1) * x + (2.0 * p2) * y);
  o.Jyy = (kr + (dk2 * y) * y) + ((6.0 * p1) * y + (2.0 * p2) * x);
}

// One view of one point: the residual and the rows of the Jacobian, scaled by sqrt(w) of the Huber weight.
struct BalView {
  bool ok;          // the depth is finite and > 0 (a view that is not ok contributes nothing)
  bool down;        // |r| > huber_px: the view is down-weighted
  double rho;       // the view's share of the cost
  double ru, rv;    // sqrt(w) r
  double Bu[3], Bv[3];              // sqrt(w) dr/dX
  double Au[kBalPar], Av[kBalPar];  // sqrt(w) dr/d(omega, t, fx, fy, cx, cy, k1, k2, p1, p2)
};

template <class Tab>
BAL_INLINE void bal_view(Tab cam, const double (&X)[3], double u, double v, double huber, BalView& o) {
  const double P0 = (cam[0] * X[0] + cam[1] * X[1]) + cam[2] * X[2];
  const double P1 = (cam[3] * X[0] + cam[4] * X[1]) + cam[5] * X[2];
  const double P2 = (cam[6] * X[0] + cam[7] * X[1]) + cam[8] * X[2];
  const double Y0 = P0 + cam[9], Y1 = P1 + cam[10], Y2 = P2 + cam[11];
  const double fx = cam[12], fy = cam[13];
  o.ok = bal_finite(Y2) && Y2 > 0.0;
  const double xn = Y0 / Y2, yn = Y1 / Y2;
  BalLens l;
  bal_lens(cam + 16, xn, yn, l);
  const double ru = (fx * l.xd + cam[14]) - u, rv = (fy * l.yd + cam[15]) - v;
  const double s2 = ru * ru + rv * rv;
  const double s = sqrt(s2);
  o.down = huber > 0.0 && s > huber;
  const double w = o.down ? huber / s : 1.0;
  o.rho = o.down ? (2.0 * huber) * s - huber * huber : s2;
  const double sw = sqrt(w);
  o.ru = sw * ru;
  o.rv = sw * rv;
  const double gu = sw * (fx / Y2), gv = sw * (fy / Y2);
  const double du0 = gu * l.Jxx, du1 = gu * l.Jxy, du2 = -(du0 * xn + du1 * yn);
  const double dv0 = gv * l.Jxy, dv1 = gv * l.Jyy, dv2 = -(dv0 * xn + dv1 * yn);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    o.Bu[j] = (du0 * cam[j] + du1 * cam[3 + j]) + du2 * cam[6 + j];
    o.Bv[j] = (dv0 * cam[j] + dv1 * cam[3 + j]) + dv2 * cam[6 + j];
  }
  o.Au[0] = du2 * P1 - du1 * P2;
  o.Au[1] = du0 * P2 - du2 * P0;
  o.Au[2] = du1 * P0 - du0 * P1;
  o.Au[3] = du0;
  o.Au[4] = du1;
  o.Au[5] = du2;
  o.Av[0] = dv2 * P1 - dv1 * P2;
  o.Av[1] = dv0 * P2 - dv2 * P0;
  o.Av[2] = dv1 * P0 - dv0 * P1;
  o.Av[3] = dv0;
  o.Av[4] = dv1;
  o.Av[5] = dv2;
  const double sfx = sw * fx, sfy = sw * fy;
  const double xr = xn * l.r2, yr = yn * l.r2, xy2 = (2.0 * xn) * yn;
  o.Au[6] = sfx * l.xd;
  o.Av[6] = 0.0;
  o.Au[7] = 0.0;
  o.Av[7] = sfy * l.yd;
  o.Au[8] = sw;
  o.Av[8] = 0.0;
  o.Au[9] = 0.0;
  o.Av[9] = sw;
  o.Au[10] = sfx * xr;
  o.Av[10] = sfy * yr;
  o.Au[11] = sfx * (xr * l.r2);
  o.Av[11] = sfy * (yr * l.r2);
  o.Au[12] = sfx * xy2;
  o.Av[12] = sfy * (l.r2 + (2.0 * yn) * yn);
  o.Au[13] = sfx * (l.r2 + (2.0 * xn) * xn);
  o.Av[13] = sfy * xy2;
}

// raw pixel -> ideal pinhole pixel: kBalNewton Newton steps on the 2 x 2 system lens(x, y) = (x0, y0), from (x0, y0).
// K9 row-major plain, k = k1 k2 p1 p2 k3.  All five coefficients zero: the pixel is copied.  A NaN in gives NaN out (both).
template <class TabK, class TabD>
BAL_INLINE void bal_undistort(TabK K9, TabD k, double u, double v, double& uo, double& vo) {
  if (u != u || v != v) {
    uo = vo = u != u ? u : v;
    return;
  }
  if (k[0] == 0.0 && k[1] == 0.0 && k[2] == 0.0 && k[3] == 0.0 && k[4] == 0.0) {
    uo = u;
    vo = v;
    return;
  }
  const double fx = K9[0], fy = K9[4], cx = K9[2], cy = K9[5];
  const double x0 = (u - cx) / fx, y0 = (v - cy) / fy;
  double x = x0, y = y0;
  for (int it = 0; it < kBalNewton; it++) {
    BalLens l;
    bal_lens(k, x, y, l);
    const double ex = l.xd - x0, ey = l.yd - y0;
    const double det = l.Jxx * l.Jyy - l.Jxy * l.Jxy;
    x = x - (l.Jyy * ex - l.Jxy * ey) / det;
    y = y - (l.Jxx * ey - l.Jxy * ex) / det;
  }
  uo = fx * x + cx;
  vo = fy * y + cy;
}

#ifdef __HIPCC__
// The model: 24 doubles per camera, 14 parameters (flag bits: fx fy | cx cy | k1 k2 | p1 p2), four row bands.
struct BalModel {
  using View = BalView;
  static constexpr int kCam = kBalCam, kPar = kBalPar, kBands = kBalBands, kSlab = kBalSlab, kCount = kBalCount;
  __host__ __device__ static constexpr int band_lo(int b) { return bal_band_lo(b); }
  __host__ __device__ static constexpr int band_hi(int b) { return bal_band_hi(b); }
  __host__ __device__ static constexpr int band_of(int i) { return bal_band_of(i); }
  __host__ __device__ static constexpr int row_off(int i) { return bal_row_off(i); }
  template <class Tab>
  __host__ __device__ static __forceinline__ void view(Tab cam, const double (&X)[3], double u, double v, double huber, View& o) {
    bal_view(cam, X, u, v, huber, o);
  }
};

hipError_t launch_bal_linearise(const SchurArgs& a, hipStream_t stream);
// out [N][C][2] = the ideal pinhole pixels of in [N][C][2] under K [C][9], dist [C][5] (all device pointers)
hipError_t launch_bal_undistort(int C, int64_t N, const double* in, const double* K, const double* dist, double* out,
                                hipStream_t stream);
#endif

}  // namespace mocap
