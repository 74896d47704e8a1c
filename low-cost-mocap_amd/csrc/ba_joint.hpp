// ba_joint.hpp -- joint bundle adjustment (include/mocap_core.h, "joint bundle adjustment"): the per-view arithmetic, written once
// for the three kernels of csrc/ba_joint.hip, and what those kernels are launched with (laid out by csrc/ba_joint_capi.hip).
// Every expression is written in the order the header pins; the build compiles with -ffp-contract=off.
#pragma once
#include "kernels.hpp"

namespace mocap {

constexpr int kBajMaxCameras = 16;     // mirrored from include/mocap_core.h (MOCAP_BAJ_MAX_CAMERAS)
constexpr int kBajMaxPoints = 131072;  // ... MOCAP_BAJ_MAX_POINTS
constexpr int kBajCam = 16;            // doubles per camera of the pose table: R [9] row-major, t [3], fx, fy, cx, cy
// one partial per workgroup and camera (grid: calib_partials(N) x C), in this order:
//   [0, 28) U, the upper triangle of the camera's 7 x 7 block A^T A row by row (rows / columns: omega 3, t 3, focal scale)
//   [28, 35) g = A^T r     [35] sum of the points' rho (camera 0 only)     [36] views used     [37] views down-weighted
//   [38] views skipped (depth not finite or <= 0)     [39] participating points (camera 0 only)     [40] singular points (camera 0 only)
constexpr int kBajSlab = 41;
constexpr int kBajPointSingular = 1;   // a point's flag: V_lambda had no Cholesky factor, the point stays where it is this pass

// finite: neither NaN nor an infinity
__host__ __device__ inline bool baj_finite(double x) { return x - x == 0.0; }
// packed upper triangle of a 7 x 7 matrix, row by row
__host__ __device__ constexpr int baj_u(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }

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
  o.ok = baj_finite(Y2) && Y2 > 0.0;
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

// what one linearisation reads and writes; every pointer device-accessible (G and sums: pinned host memory)
struct BajArgs {
  int C, focal, n_c, NP;
  int64_t N, m_pad;
  double huber, lambda;
  const double* obs;      // [N][C][2], NaN = unseen
  const double* cams;     // [C][kBajCam] of the point of linearisation
  const double* X;        // [N][3]
  const int32_t* part;    // [N] 1 = the point takes part
  double* Jaug;           // [m_pad][NP]: the point's rows 3 p .. 3 p + 2 of [E | z | 0]
  double* L;              // [N][6]: l00 l10 l20 l11 l21 l22
  double* rho;            // [N]
  int32_t* flags;         // [N] kBajPoint*
  double* partial;        // launch_ba_gram's K slices
  int ksplit;
  double* G;              // [NP][NP] out: Jaug^T Jaug
  double* slab;           // [C][calib_partials(N)][kBajSlab]
  double* sums;           // [C][kBajSlab] out
};

// start: which points take part, and (given == 0) their DLT start from Ptab [C][12], each camera's own K [R | t]
hipError_t launch_baj_start(int C, int64_t N, const double* obs, const double* Ptab, int given, double* X, int32_t* part,
                            hipStream_t stream);
// linearise + Gram + camera blocks + fold: 5 launches
hipError_t launch_baj_linearise(const BajArgs& a, hipStream_t stream);
// X_trial = X - L^-T (z + E delta) per point, from the linearisation `a`
hipError_t launch_baj_backsub(const BajArgs& a, const double* delta, double* X_trial, hipStream_t stream);
// X_out = scale X for the points that take part, NaN for the others
hipError_t launch_baj_finish(int64_t N, const double* X, const int32_t* part, double scale, double* X_out, hipStream_t stream);

}  // namespace mocap
