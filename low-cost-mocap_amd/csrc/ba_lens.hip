// ba_lens.hip -- the kernels of the "lens calibration" section of include/mocap_core.h: the joint bundle adjustment with the full lens
// model -- per camera fx, fy, cx, cy, k1, k2, p1, p2 beside its pose -- and the inverse of that lens for observations.
//   linearise  one lane per point, two walks over its views: V and g_p, the 3 x 3 Cholesky factor of V_lambda, then per used view up to
//              14 columns of E = L^-1 W^T straight into the point's three rows of Jaug = [E | z | 0], the layout launch_ba_gram takes
//   cameras    grid (points / 256, camera, row band): the camera's 14 x 14 block is 105 + 14 sums, more than one lane can carry, so
//              the upper triangle is cut into four row bands (csrc/ba_lens.hpp) and every band recomputes the view; each band goes
//              through the project's one tree (csrc/tree_fold.hpp), one wave per (camera, band) folds its slab.  The order of every
//              sum is a function of N alone.
//   backsub    one lane per point: X_trial = X - L^-T (z + E delta)
//   undistort  one lane per observation: a fixed number of Newton steps on the 2 x 2 lens system
// The start (participation, DLT) and the finish (gauge) are the joint bundle adjustment's kernels, called as they are.
// FP64 throughout, nothing fused, no atomics: every output is a function of the inputs alone.
#include "ba_lens.hpp"

#include "ba_joint.hpp"
#include "mocap_device.hpp"
#include "tree_fold.hpp"

namespace mocap {

namespace {

constexpr int kT = kCalibThreads;

__device__ __forceinline__ bool bal_seen(const double* o, int c, double& u, double& v) {
  u = o[2 * c];
  v = o[2 * c + 1];
  return !(isnan(u) || isnan(v));  // mocap_triangulate's rule
}

// --------------------------------------------------------------------------------------------------------------- linearise
__global__ __launch_bounds__(kT) void bal_linearise_kernel(BalArgs a) {
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
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
    if (!bal_seen(o, c, u, v)) continue;
    BalView w;
    bal_view(cams + kBalCam * c, X, u, v, a.huber, w);
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
  const bool piv = bal_finite(a00) && a00 > 0.0 && bal_finite(d1) && d1 > 0.0 && bal_finite(d2) && d2 > 0.0;
  double* L = a.L + 6 * p;
  L[0] = piv ? l00 : 1.0;
  L[1] = piv ? l10 : 0.0;
  L[2] = piv ? l20 : 0.0;
  L[3] = piv ? l11 : 1.0;
  L[4] = piv ? l21 : 0.0;
  L[5] = piv ? l22 : 1.0;
  a.rho[p] = rho;
  a.flags[p] = piv ? 0 : kBalPointSingular;
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
    if (!bal_seen(o, c, u, v)) continue;
    BalView w;
    bal_view(cams + kBalCam * c, X, u, v, a.huber, w);
    const bool use = piv && w.ok;
    int next = base + a.q * c;  // the camera's next intrinsic column
#pragma unroll
    for (int k = 0; k < kBalPar; k++) {
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
// one row band of one camera's block: v = the lane's addends, zero where the point or the view does not count
template <int B>
__device__ __forceinline__ void bal_band(const BalArgs& a, int64_t p, int c, double (&v)[kBalSlab]) {
  constexpr int lo = bal_band_lo(B), hi = bal_band_hi(B);
#pragma unroll
  for (int i = 0; i < kBalSlab; i++) v[i] = 0.0;
  if (p < a.N && a.part[p]) {
    const double X[3] = {a.X[3 * p], a.X[3 * p + 1], a.X[3 * p + 2]};
    double ou, ov;
    if (bal_seen(a.obs + (size_t)p * a.C * 2, c, ou, ov)) {
      BalView w;
      bal_view(as_ctab(a.cams) + kBalCam * c, X, ou, ov, a.huber, w);
      if (w.ok) {
        int off = 0;  // = bal_row_off(i)
#pragma unroll
        for (int i = lo; i < hi; i++) {
#pragma unroll
          for (int j = i; j < kBalPar; j++) v[off + (j - i)] = w.Au[i] * w.Au[j] + w.Av[i] * w.Av[j];
          v[off + (kBalPar - i)] = w.Au[i] * w.ru + w.Av[i] * w.rv;
          off += 15 - i;
        }
        if (B == kBalBands - 1) {
          v[kBalCount + 1] = 1.0;
          v[kBalCount + 2] = w.down ? 1.0 : 0.0;
        }
      } else if (B == kBalBands - 1) {
        v[kBalCount + 3] = 1.0;
      }
    }
    if (B == kBalBands - 1 && c == 0) {
      v[kBalCount] = a.rho[p];
      v[kBalCount + 4] = 1.0;
      v[kBalCount + 5] = (a.flags[p] & kBalPointSingular) ? 1.0 : 0.0;
    }
  }
}

__global__ __launch_bounds__(kT) void bal_cameras_kernel(BalArgs a) {
  __shared__ double s_part[kFoldWaves][kBalSlab];
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int c = blockIdx.y, band = blockIdx.z;  // (the band is uniform over the workgroup)
  double v[kBalSlab];
  if (band == 0)
    bal_band<0>(a, p, c, v);
  else if (band == 1)
    bal_band<1>(a, p, c, v);
  else if (band == 2)
    bal_band<2>(a, p, c, v);
  else
    bal_band<3>(a, p, c, v);
  block_fold<kBalSlab, -1>(v, s_part, a.slab + (((size_t)c * kBalBands + band) * gridDim.x + blockIdx.x) * kBalSlab);
}

// one wave per (camera, band)
__global__ __launch_bounds__(64) void bal_cameras_final_kernel(BalArgs a, int64_t P) {
  const int cb = blockIdx.x;
  double v[kBalSlab];
  slab_fold<kBalSlab, -1>(a.slab + (size_t)cb * P * kBalSlab, P, 0.0, v);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int i = 0; i < kBalSlab; i++) a.sums[cb * kBalSlab + i] = v[i];
}

// ----------------------------------------------------------------------------------------------------------------- backsub
__global__ __launch_bounds__(kT) void bal_backsub_kernel(BalArgs a, const double* delta, double* __restrict__ Xt) {
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (p >= a.N) return;
  double X[3] = {a.X[3 * p], a.X[3 * p + 1], a.X[3 * p + 2]};
  if (a.part[p] && !(a.flags[p] & kBalPointSingular)) {
    const int C = a.C, NP = a.NP;
    const double* o = a.obs + (size_t)p * C * 2;
    const double* row = a.Jaug + (size_t)(3 * p) * NP;
    const ctab_t d = as_ctab(delta);
    double y0 = row[a.n_c], y1 = row[NP + a.n_c], y2 = row[2 * NP + a.n_c];
    // z + E delta over the columns in ascending order; the columns of a camera that does not see the point are zero
    for (int c = 1; c < C; c++) {
      double u, v;
      if (!bal_seen(o, c, u, v)) continue;
#pragma unroll
      for (int k = 0; k < 6; k++) {
        const int col = 6 * (c - 1) + k;
        const double dk = d[col];
        y0 = y0 + row[col] * dk;
        y1 = y1 + row[NP + col] * dk;
        y2 = y2 + row[2 * NP + col] * dk;
      }
    }
    if (a.q)
      for (int c = 0; c < C; c++) {
        double u, v;
        if (!bal_seen(o, c, u, v)) continue;
        for (int k = 0; k < a.q; k++) {
          const int col = 6 * (C - 1) + a.q * c + k;
          const double dk = d[col];
          y0 = y0 + row[col] * dk;
          y1 = y1 + row[NP + col] * dk;
          y2 = y2 + row[2 * NP + col] * dk;
        }
      }
    const double* L = a.L + 6 * p;
    const double x2 = y2 / L[5];
    const double x1 = (y1 - L[4] * x2) / L[3];
    const double x0 = ((y0 - L[1] * x1) - L[2] * x2) / L[0];
    X[0] = X[0] - x0;
    X[1] = X[1] - x1;
    X[2] = X[2] - x2;
  }
  Xt[3 * p] = X[0];
  Xt[3 * p + 1] = X[1];
  Xt[3 * p + 2] = X[2];
}

// --------------------------------------------------------------------------------------------------------------- undistort
__global__ __launch_bounds__(kT) void bal_undistort_kernel(int C, int64_t n_obs, const double* in, const double* K,
                                                           const double* dist, double* out) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n_obs) return;
  const int c = (int)(i % C);
  double uo, vo;
  bal_undistort(K + 9 * c, dist + 5 * c, in[2 * i], in[2 * i + 1], uo, vo);
  out[2 * i] = uo;
  out[2 * i + 1] = vo;
}

}  // namespace

hipError_t launch_bal_linearise(const BalArgs& a, hipStream_t stream) {
  const int64_t P = calib_partials(a.N);
  hipError_t e;
  hipLaunchKernelGGL(bal_linearise_kernel, dim3((unsigned)P), dim3(kT), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_ba_gram(a.Jaug, a.m_pad, a.NP, a.partial, a.ksplit, a.G, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(bal_cameras_kernel, dim3((unsigned)P, (unsigned)a.C, kBalBands), dim3(kT), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(bal_cameras_final_kernel, dim3((unsigned)(a.C * kBalBands)), dim3(64), 0, stream, a, P);
  return hipGetLastError();
}

hipError_t launch_bal_backsub(const BalArgs& a, const double* delta, double* X_trial, hipStream_t stream) {
  hipLaunchKernelGGL(bal_backsub_kernel, dim3((unsigned)calib_partials(a.N)), dim3(kT), 0, stream, a, delta, X_trial);
  return hipGetLastError();
}

hipError_t launch_bal_undistort(int C, int64_t N, const double* in, const double* K, const double* dist, double* out,
                                hipStream_t stream) {
  const int64_t n_obs = N * C;
  hipLaunchKernelGGL(bal_undistort_kernel, dim3((unsigned)calib_partials(n_obs)), dim3(kT), 0, stream, C, n_obs, in, K, dist, out);
  return hipGetLastError();
}

}  // namespace mocap
