// ba_joint.hpp -- joint bundle adjustment (include/mocap_core.h, "joint bundle adjustment"): the per-view arithmetic and the camera
// model the kernels of csrc/ba_schur.hpp are instantiated with in csrc/ba_joint.hip.
// Every expression is written in the order the header pins; the build compiles with -ffp-contract=off.
#pragma once
#include "ba_schur.hpp"

namespace mocap {

constexpr int kBajMaxCameras = 16;     // mirrored from include/mocap_core.h (MOCAP_BAJ_MAX_CAMERAS)
constexpr int kBajMaxPoints = 131072;  // ... MOCAP_BAJ_MAX_POINTS

// One view of one point: the residual and the rows of the Jacobian, scaled by sqrt(w) of the Huber weight.
struct BajView {
  bool ok;          // the depth is finite and > 0 (a view that is not ok contributes nothing)
  bool down;        // |r| > huber_px: the view is down-weighted
  double rho;       // the view's share of the cost
  double ru, rv;    // sqrt(w) r
  double Bu[3], Bv[3];  // sqrt(w) dr/dX
  double Au[7], Av[7];  // sqrt(w) dr/d(omega, t, focal scale)
};

template <class Tab>
__host__ __device__ __forceinline__ void baj_view(Tab cam, const double (&X)[3], double u, double v, double huber, BajView& o) {
  const double P0 = (cam[0] * X[0] + cam[1] * X[1]) + cam[2] * X[2];
  const double P1 = (cam[3] * X[0] + cam[4] * X[1]) + cam[5] * X[2];
  const double P2 = (cam[6] * X[0] + cam[7] * X[1]) + cam[8] * X[2];
  const double Y0 = P0 + cam[9], Y1 = P1 + cam[10], Y2 = P2 + cam[11];
  const double fx = cam[12], fy = cam[13];
  o.ok = schur_finite(Y2) && Y2 > 0.0;
  const double xn = Y0 / Y2, yn = Y1 / Y2;
  const double ru = (fx * xn + cam[14]) - u, rv = (fy * yn + cam[15]) - v;
  const double s2 = ru * ru + rv * rv;
  const double s = sqrt(s2);
  o.down = huber > 0.0 && s > huber;
  const double w = o.down ? huber / s : 1.0;
  o.rho = o.down ? (2.0 * huber) * s - huber * huber : s2;
  const double sw = sqrt(w);
  o.ru = sw * ru;
  o.rv = sw * rv;
  const double du0 = sw * (fx / Y2), dv1 = sw * (fy / Y2);
  const double du2 = -(du0 * xn), dv2 = -(dv1 * yn);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    o.Bu[j] = du0 * cam[j] + du2 * cam[6 + j];
    o.Bv[j] = dv1 * cam[3 + j] + dv2 * cam[6 + j];
  }
  o.Au[0] = du2 * P1;
  o.Au[1] = du0 * P2 - du2 * P0;
  o.Au[2] = -(du0 * P1);
  o.Au[3] = du0;
  o.Au[4] = 0.0;
  o.Au[5] = du2;
  o.Au[6] = sw * (fx * xn);
  o.Av[0] = dv2 * P1 - dv1 * P2;
  o.Av[1] = -(dv2 * P0);
  o.Av[2] = dv1 * P0;
  o.Av[3] = 0.0;
  o.Av[4] = dv1;
  o.Av[5] = dv2;
  o.Av[6] = sw * (fy * yn);
}

// The model: 16 doubles per camera (R [9] row-major, t [3], fx, fy, cx, cy), 7 parameters (omega 3, t 3, focal scale: flag bit 0),
// the 7 x 7 block in one band: rows 0 .. 6 are 35 values, then the six counters.
struct BajModel {
  using View = BajView;
  static constexpr int kCam = 16, kPar = 7, kBands = 1, kSlab = 41, kCount = 35;
  __host__ __device__ static constexpr int band_lo(int) { return 0; }
  __host__ __device__ static constexpr int band_hi(int) { return kPar; }
  __host__ __device__ static constexpr int band_of(int) { return 0; }
  __host__ __device__ static constexpr int row_off(int i) { return i * (kPar + 1) - i * (i - 1) / 2; }
  template <class Tab>
  __host__ __device__ static __forceinline__ void view(Tab cam, const double (&X)[3], double u, double v, double huber, View& o) {
    baj_view(cam, X, u, v, huber, o);
  }
};

hipError_t launch_baj_linearise(const SchurArgs& a, hipStream_t stream);

}  // namespace mocap
