// ba_schur.hpp -- bundle adjustment with the points eliminated (Schur complement), written once for the joint bundle adjustment
// (csrc/ba_joint.hip) and the lens calibration (csrc/ba_lens.hip): what a linearisation is launched with, and its kernels as
// templates over a camera MODEL.  A model M says what a camera is and nothing about the loop:
//   M::View, M::view(cam, X, u, v, huber, out)   the per-view arithmetic: ok, down, rho, ru, rv, Bu / Bv [3], Au / Av [kPar]
//   M::kCam                                      doubles per camera of the camera table
//   M::kPar                                      a camera's parameters: omega 3, t 3, then the intrinsics in pairs of flag bits
//   M::kBands, M::band_lo / band_hi (b)          the camera block's rows cut into row bands, one per blockIdx.z
//   M::band_of (i), M::row_off (i)               the band of row i, and where the row starts inside its band
//   M::kSlab, M::kCount                          doubles per slab entry, and where the last band's six counters start
// The camera block U (upper triangle of kPar x kPar) is laid out row by row, row i = U[i][i .. kPar - 1] followed by g[i]:
// kPar + 1 - i values.  One partial per workgroup, camera and band: slab [C][kBands][calib_partials(N)][kSlab], sums
// [C][kBands][kSlab].  Behind the rows of the last band: [kCount] sum of the points' rho (camera 0 only)  [+1] views used
// [+2] views down-weighted  [+3] views skipped (depth not finite or <= 0)  [+4] participating points (camera 0 only)
// [+5] singular points (camera 0 only).  Every slot goes through the project's one tree (csrc/tree_fold.hpp) by itself, in an order
// that is a function of N alone: where a sum stands in the slab does not change its bits.
//   linearise  one lane per point, two walks over its views: V and g_p, the 3 x 3 Cholesky factor of V_lambda, then per view
//              E_c = L^-1 W_c^T straight into the point's three rows of Jaug = [E | z | 0] -- the layout launch_ba_gram takes, so
//              sum E^T E and sum E^T z come out of the FP64 matrix cores in ba_gram_reduce_kernel's fixed slice order
//   cameras    grid (points / 256, camera, row band), one lane per point: the band's rows of U_c = sum A^T A and g_c = sum A^T r,
//              the cost and the counters; every band recomputes the view.  Then one wave per (camera, band) folds the slab.
// The per-view arithmetic is recomputed wherever it is needed: a view is 60 to 150 FP64 operations, keeping sixteen views' blocks
// per lane would not fit the registers.  The camera table and delta are wave-uniform reads through the constant address space
// (scalar loads); a lane's rows of Jaug are 3 NP doubles of its own, written and read by that lane alone.
// FP64 throughout, nothing fused, no atomics: every output is a function of the inputs alone.
#pragma once
#include <utility>

#include "kernels.hpp"
#include "mocap_device.hpp"
#include "tree_fold.hpp"

namespace mocap {

constexpr int kSchurPointSingular = 1;  // a point's flag: V_lambda had no Cholesky factor, the point stays where it is this pass

// what one linearisation reads and writes; every pointer device-accessible (G and sums: pinned host memory)
struct SchurArgs {
  int C, q, n_c, NP;      // q: intrinsic unknowns per camera, columns 6 (C - 1) + q c ..
  uint32_t sel;           // which pairs of intrinsics are unknowns: parameter k >= 6 belongs to bit (k - 6) >> 1
  int64_t N, m_pad;
  double huber, lambda;
  const double* obs;      // [N][C][2], NaN = unseen
  const double* cams;     // [C][M::kCam] of the point of linearisation
  const double* X;        // [N][3]
  const int32_t* part;    // [N] 1 = the point takes part
  double* Jaug;           // [m_pad][NP]: the point's rows 3 p .. 3 p + 2 of [E | z | 0]
  double* L;              // [N][6]: l00 l10 l20 l11 l21 l22
  double* rho;            // [N]
  int32_t* flags;         // [N] kSchurPoint*
  double* partial;        // launch_ba_gram's K slices
  int ksplit;
  double* G;              // [NP][NP] out: Jaug^T Jaug
  double* slab;           // [C][M::kBands][calib_partials(N)][M::kSlab]
  double* sums;           // [C][M::kBands][M::kSlab] out
};

// finite: neither NaN nor an infinity
__host__ __device__ inline bool schur_finite(double x) { return x - x == 0.0; }

namespace {

__device__ __forceinline__ bool schur_seen(const double* o, int c, double& u, double& v) {
  u = o[2 * c];
  v = o[2 * c + 1];
  return !(isnan(u) || isnan(v));  // mocap_triangulate's rule
}

// --------------------------------------------------------------------------------------------------------------- linearise
template <class M>
__global__ __launch_bounds__(kCalibThreads) void schur_linearise_kernel(SchurArgs a) {
  const int64_t p = (int64_t)blockIdx.x * kCalibThreads + threadIdx.x;
  if (p >= a.N) return;
  if (!a.part[p]) {  // (its rows of Jaug were zeroed when the workspace was laid out)
    a.rho[p] = 0.0;
    a.flags[p] = 0;
    return;
  }
  const int C = a.C, NP = a.NP;
  const double* o = a.obs + (size_t)p * C * 2;
  const ctab_t cams = as_ctab(a.cams);
  const double X[3] = {a.X[3 * p], a.X[3 * p + 1], a.X[3 * p + 2]};
  double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, rho = 0.0;
  for (int c = 0; c < C; c++) {
    double u, v;
    if (!schur_seen(o, c, u, v)) continue;
    typename M::View w;
    M::view(cams + M::kCam * c, X, u, v, a.huber, w);
    if (!w.ok) continue;
    rho = rho + w.rho;
    V[0] = V[0] + (w.Bu[0] * w.Bu[0] + w.Bv[0] * w.Bv[0]);
    V[1] = V[1] + (w.Bu[0] * w.Bu[1] + w.Bv[0] * w.Bv[1]);
    V[2] = V[2] + (w.Bu[0] * w.Bu[2] + w.Bv[0] * w.Bv[2]);
    V[3] = V[3] + (w.Bu[1] * w.Bu[1] + w.Bv[1] * w.Bv[1]);
    V[4] = V[4] + (w.Bu[1] * w.Bu[2] + w.Bv[1] * w.Bv[2]);
    V[5] = V[5] + (w.Bu[2] * w.Bu[2] + w.Bv[2] * w.Bv[2]);
#pragma unroll
    for (int j = 0; j < 3; j++) g[j] = g[j] + (w.Bu[j] * w.ru + w.Bv[j] * w.rv);
  }
  // V_lambda = L L^T
  const double a00 = V[0] + a.lambda * V[0], a11 = V[3] + a.lambda * V[3], a22 = V[5] + a.lambda * V[5];
  const double l00 = sqrt(a00);
  const double l10 = V[1] / l00, l20 = V[2] / l00;
  const double d1 = a11 - l10 * l10;
  const double l11 = sqrt(d1);
  const double l21 = (V[4] - l20 * l10) / l11;
  const double d2 = (a22 - l20 * l20) - l21 * l21;
  const double l22 = sqrt(d2);
  const bool piv = schur_finite(a00) && a00 > 0.0 && schur_finite(d1) && d1 > 0.0 && schur_finite(d2) && d2 > 0.0;
  double* L = a.L + 6 * p;
  L[0] = piv ? l00 : 1.0;
  L[1] = piv ? l10 : 0.0;
  L[2] = piv ? l20 : 0.0;
  L[3] = piv ? l11 : 1.0;
  L[4] = piv ? l21 : 0.0;
  L[5] = piv ? l22 : 1.0;
  a.rho[p] = rho;
  a.flags[p] = piv ? 0 : kSchurPointSingular;
  // z = L^-1 g_p
  const double z0 = g[0] / l00;
  const double z1 = (g[1] - l10 * z0) / l11;
  const double z2 = ((g[2] - l20 * z0) - l21 * z1) / l22;
  double* row = a.Jaug + (size_t)(3 * p) * NP;
  row[a.n_c] = piv ? z0 : 0.0;
  row[NP + a.n_c] = piv ? z1 : 0.0;
  row[2 * NP + a.n_c] = piv ? z2 : 0.0;
  // E_c = L^-1 W_c^T, W_c = A^T B: one column of E per unknown of the camera
  const int base = 6 * (C - 1);
  for (int c = 0; c < C; c++) {
    double u, v;
    if (!schur_seen(o, c, u, v)) continue;
    typename M::View w;
    M::view(cams + M::kCam * c, X, u, v, a.huber, w);
    const bool use = piv && w.ok;
    int next = base + a.q * c;  // the camera's next intrinsic column
#pragma unroll
    for (int k = 0; k < M::kPar; k++) {
      int col;
      if (k < 6) {
        if (c == 0) continue;
        col = 6 * (c - 1) + k;
      } else {
        if (!(a.sel >> ((k - 6) >> 1) & 1u)) continue;
        col = next++;
      }
      const double w0 = w.Au[k] * w.Bu[0] + w.Av[k] * w.Bv[0];
      const double w1 = w.Au[k] * w.Bu[1] + w.Av[k] * w.Bv[1];
      const double w2 = w.Au[k] * w.Bu[2] + w.Av[k] * w.Bv[2];
      const double e0 = w0 / l00;
      const double e1 = (w1 - l10 * e0) / l11;
      const double e2 = ((w2 - l20 * e0) - l21 * e1) / l22;
      row[col] = use ? e0 : 0.0;
      row[NP + col] = use ? e1 : 0.0;
      row[2 * NP + col] = use ? e2 : 0.0;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------- cameras
// row band B of one camera's block: v = the lane's addends, zero where the point or the view does not count
template <class M, int B>
__device__ __forceinline__ void schur_band(const SchurArgs& a, int64_t p, int c, double (&v)[M::kSlab]) {
  constexpr int lo = M::band_lo(B), hi = M::band_hi(B);
  constexpr bool last = B == M::kBands - 1;
#pragma unroll
  for (int i = 0; i < M::kSlab; i++) v[i] = 0.0;
  if (p < a.N && a.part[p]) {
    const double X[3] = {a.X[3 * p], a.X[3 * p + 1], a.X[3 * p + 2]};
    double ou, ov;
    if (schur_seen(a.obs + (size_t)p * a.C * 2, c, ou, ov)) {
      typename M::View w;
      M::view(as_ctab(a.cams) + M::kCam * c, X, ou, ov, a.huber, w);
      if (w.ok) {
        int off = 0;  // = M::row_off(i)
#pragma unroll
        for (int i = lo; i < hi; i++) {
#pragma unroll
          for (int j = i; j < M::kPar; j++) v[off + (j - i)] = w.Au[i] * w.Au[j] + w.Av[i] * w.Av[j];
          v[off + (M::kPar - i)] = w.Au[i] * w.ru + w.Av[i] * w.rv;
          off += M::kPar + 1 - i;
        }
        if (last) {
          v[M::kCount + 1] = 1.0;
          v[M::kCount + 2] = w.down ? 1.0 : 0.0;
        }
      } else if (last) {
        v[M::kCount + 3] = 1.0;
      }
    }
    if (last && c == 0) {
      v[M::kCount] = a.rho[p];
      v[M::kCount + 4] = 1.0;
      v[M::kCount + 5] = (a.flags[p] & kSchurPointSingular) ? 1.0 : 0.0;
    }
  }
}

// the band is uniform over the workgroup: one branch per band in turn, the last taken without a test
template <class M, int... B>
__device__ __forceinline__ void schur_bands(int band, const SchurArgs& a, int64_t p, int c, double (&v)[M::kSlab],
                                            std::integer_sequence<int, B...>) {
  (void)(((band == B || B == M::kBands - 1) && (schur_band<M, B>(a, p, c, v), true)) || ...);
}

template <class M>
__global__ __launch_bounds__(kCalibThreads) void schur_cameras_kernel(SchurArgs a) {
  __shared__ double s_part[kFoldWaves][M::kSlab];
  const int64_t p = (int64_t)blockIdx.x * kCalibThreads + threadIdx.x;
  const int c = blockIdx.y, band = blockIdx.z;
  double v[M::kSlab];
  schur_bands<M>(band, a, p, c, v, std::make_integer_sequence<int, M::kBands>{});
  block_fold<M::kSlab, -1>(v, s_part, a.slab + (((size_t)c * M::kBands + band) * gridDim.x + blockIdx.x) * M::kSlab);
}

// one wave per (camera, band)
template <int kSlab>
__global__ __launch_bounds__(64) void schur_cameras_final_kernel(SchurArgs a, int64_t P) {
  const int cb = blockIdx.x;
  double v[kSlab];
  slab_fold<kSlab, -1>(a.slab + (size_t)cb * P * kSlab, P, 0.0, v);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int i = 0; i < kSlab; i++) a.sums[cb * kSlab + i] = v[i];
}

// linearise + Gram + camera blocks + fold: 5 launches
template <class M>
hipError_t schur_launch_linearise(const SchurArgs& a, hipStream_t stream) {
  const int64_t P = calib_partials(a.N);
  hipError_t e;
  hipLaunchKernelGGL(schur_linearise_kernel<M>, dim3((unsigned)P), dim3(kCalibThreads), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_ba_gram(a.Jaug, a.m_pad, a.NP, a.partial, a.ksplit, a.G, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(schur_cameras_kernel<M>, dim3((unsigned)P, (unsigned)a.C, M::kBands), dim3(kCalibThreads), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(schur_cameras_final_kernel<M::kSlab>, dim3((unsigned)(a.C * M::kBands)), dim3(64), 0, stream, a, P);
  return hipGetLastError();
}

}  // namespace

// The kernels that are not templates live in csrc/ba_joint.hip, for both solvers:
// start: which points take part, and (given == 0) their DLT start from Ptab [C][12], each camera's own K [R | t]
hipError_t launch_baj_start(int C, int64_t N, const double* obs, const double* Ptab, int given, double* X, int32_t* part,
                            hipStream_t stream);
// X_trial = X - L^-T (z + E delta) per point, from the linearisation `a`
hipError_t launch_schur_backsub(const SchurArgs& a, const double* delta, double* X_trial, hipStream_t stream);
// X_out = scale X for the points that take part, NaN for the others
hipError_t launch_baj_finish(int64_t N, const double* X, const int32_t* part, double scale, double* X_out, hipStream_t stream);

}  // namespace mocap
