// ba_joint.hip -- the kernels of the "joint bundle adjustment" section of include/mocap_core.h: camera poses, optional focal scales
// and all 3-D points as unknowns, analytic Jacobians, the points eliminated per lane (Schur complement).
//   start      one lane per point: does it take part, and its DLT start (the device functions of mocap_triangulate, on a table of
//              each camera's own K [R | t])
//   linearise  one lane per point, two walks over its views: V and g_p, the 3 x 3 Cholesky factor of V_lambda, then per view
//              E_c = L^-1 W_c^T straight into the point's three rows of Jaug = [E | z | 0] -- the layout launch_ba_gram takes, so
//              sum E^T E and sum E^T z come out of the FP64 matrix cores in ba_gram_reduce_kernel's fixed slice order
//   cameras    grid.y = camera, one lane per point: U_c = sum A^T A, g_c = sum A^T r, the cost and the counters through the
//              project's one tree (csrc/tree_fold.hpp), then one wave per camera folds the slab
//   backsub    one lane per point: X_trial = X - L^-T (z + E delta)
// The per-view arithmetic is baj_view (csrc/ba_joint.hpp), recomputed wherever it is needed: a view is ~60 FP64 operations, keeping
// sixteen views' blocks per lane would not fit the registers.  The pose table [C][16] and delta are wave-uniform reads through the
// constant address space (scalar loads); a lane's rows of Jaug are 3 NP doubles of its own, written and read by that lane alone.
// FP64 throughout, nothing fused, no atomics: every output is a function of the inputs alone.
#include "ba_joint.hpp"
#include "mocap_device.hpp"
#include "tree_fold.hpp"

namespace mocap {

namespace {

constexpr int kT = kCalibThreads;

__device__ __forceinline__ bool baj_seen(const double* o, int c, double& u, double& v) {
  u = o[2 * c];
  v = o[2 * c + 1];
  return !(isnan(u) || isnan(v));  // mocap_triangulate's rule
}

// ------------------------------------------------------------------------------------------------------------------- start
__global__ __launch_bounds__(kT) void baj_start_kernel(int C, int64_t N, const double* __restrict__ obs, const double* Ptab,
                                                       int given, double* __restrict__ X, int32_t* __restrict__ part) {
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (p >= N) return;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const double* o = obs + (size_t)p * C * 2;
  const ctab_t P = as_ctab(Ptab);
  int views = 0;
  bool ok = true;
  double B[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = 0; c < C; c++) {
    double u, v;
    if (!baj_seen(o, c, u, v)) continue;
    views++;
    ok = ok && baj_finite(u) && baj_finite(v);
    if (!given) dlt_accumulate(B, P + 12 * c, u, v);
  }
  ok = ok && views >= 2;
  double x[3];
  if (given) {
    x[0] = X[3 * p];
    x[1] = X[3 * p + 1];
    x[2] = X[3 * p + 2];
  } else {
    x[0] = x[1] = x[2] = qnan;
    if (ok) solve_point(B, x);
  }
  ok = ok && baj_finite(x[0]) && baj_finite(x[1]) && baj_finite(x[2]);
  if (ok && !given) {  // the start lies in front of every camera that sees it
    for (int c = 0; c < C; c++) {
      double u, v;
      if (!baj_seen(o, c, u, v)) continue;
      const ctab_t Pc = P + 12 * c;
      const double w = ((Pc[8] * x[0] + Pc[9] * x[1]) + Pc[10] * x[2]) + Pc[11];
      ok = ok && baj_finite(w) && w > 0.0;
    }
  }
  part[p] = ok ? 1 : 0;
  if (!given) {
    X[3 * p] = ok ? x[0] : qnan;
    X[3 * p + 1] = ok ? x[1] : qnan;
    X[3 * p + 2] = ok ? x[2] : qnan;
  }
}

// --------------------------------------------------------------------------------------------------------------- linearise
__global__ __launch_bounds__(kT) void baj_linearise_kernel(BajArgs a) {
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
    if (!baj_seen(o, c, u, v)) continue;
    BajView w;
    baj_view(cams + kBajCam * c, X, u, v, a.huber, w);
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
  const bool piv = baj_finite(a00) && a00 > 0.0 && baj_finite(d1) && d1 > 0.0 && baj_finite(d2) && d2 > 0.0;
  double* L = a.L + 6 * p;
  L[0] = piv ? l00 : 1.0;
  L[1] = piv ? l10 : 0.0;
  L[2] = piv ? l20 : 0.0;
  L[3] = piv ? l11 : 1.0;
  L[4] = piv ? l21 : 0.0;
  L[5] = piv ? l22 : 1.0;
  a.rho[p] = rho;
  a.flags[p] = piv ? 0 : kBajPointSingular;
  // z = L^-1 g_p
  const double z0 = g[0] / l00;
  const double z1 = (g[1] - l10 * z0) / l11;
  const double z2 = ((g[2] - l20 * z0) - l21 * z1) / l22;
  double* row = a.Jaug + (size_t)(3 * p) * NP;
  row[a.n_c] = piv ? z0 : 0.0;
  row[NP + a.n_c] = piv ? z1 : 0.0;
  row[2 * NP + a.n_c] = piv ? z2 : 0.0;
  // E_c = L^-1 W_c^T, W_c = A^T B: one column of E per parameter of the camera
  for (int c = 0; c < C; c++) {
    double u, v;
    if (!baj_seen(o, c, u, v)) continue;
    BajView w;
    baj_view(cams + kBajCam * c, X, u, v, a.huber, w);
    const bool use = piv && w.ok;
#pragma unroll
    for (int k = 0; k < 7; k++) {
      if (k < 6 ? c == 0 : !a.focal) continue;
      const int col = k < 6 ? 6 * (c - 1) + k : 6 * (C - 1) + c;
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
__global__ __launch_bounds__(kT) void baj_cameras_kernel(BajArgs a) {
  __shared__ double s_part[kFoldWaves][kBajSlab];
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int c = blockIdx.y;
  double v[kBajSlab];
#pragma unroll
  for (int i = 0; i < kBajSlab; i++) v[i] = 0.0;
  if (p < a.N && a.part[p]) {
    const double X[3] = {a.X[3 * p], a.X[3 * p + 1], a.X[3 * p + 2]};
    double ou, ov;
    if (baj_seen(a.obs + (size_t)p * a.C * 2, c, ou, ov)) {
      BajView w;
      baj_view(as_ctab(a.cams) + kBajCam * c, X, ou, ov, a.huber, w);
      if (w.ok) {
#pragma unroll
        for (int i = 0; i < 7; i++) {
#pragma unroll
          for (int j = i; j < 7; j++) v[baj_u(i, j)] = w.Au[i] * w.Au[j] + w.Av[i] * w.Av[j];
          v[28 + i] = w.Au[i] * w.ru + w.Av[i] * w.rv;
        }
        v[36] = 1.0;
        v[37] = w.down ? 1.0 : 0.0;
      } else {
        v[38] = 1.0;
      }
    }
    if (c == 0) {
      v[35] = a.rho[p];
      v[39] = 1.0;
      v[40] = (a.flags[p] & kBajPointSingular) ? 1.0 : 0.0;
    }
  }
  block_fold<kBajSlab, -1>(v, s_part, a.slab + ((size_t)c * gridDim.x + blockIdx.x) * kBajSlab);
}

// one wave per camera
__global__ __launch_bounds__(64) void baj_cameras_final_kernel(BajArgs a, int64_t P) {
  const int c = blockIdx.x;
  double v[kBajSlab];
  slab_fold<kBajSlab, -1>(a.slab + (size_t)c * P * kBajSlab, P, 0.0, v);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int i = 0; i < kBajSlab; i++) a.sums[c * kBajSlab + i] = v[i];
}

// ----------------------------------------------------------------------------------------------------------------- backsub
__global__ __launch_bounds__(kT) void baj_backsub_kernel(BajArgs a, const double* delta, double* __restrict__ Xt) {
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (p >= a.N) return;
  double X[3] = {a.X[3 * p], a.X[3 * p + 1], a.X[3 * p + 2]};
  if (a.part[p] && !(a.flags[p] & kBajPointSingular)) {
    const int C = a.C, NP = a.NP;
    const double* o = a.obs + (size_t)p * C * 2;
    const double* row = a.Jaug + (size_t)(3 * p) * NP;
    const ctab_t d = as_ctab(delta);
    double y0 = row[a.n_c], y1 = row[NP + a.n_c], y2 = row[2 * NP + a.n_c];
    // z + E delta over the columns in ascending order; the columns of a camera that does not see the point are zero
    for (int c = 1; c < C; c++) {
      double u, v;
      if (!baj_seen(o, c, u, v)) continue;
#pragma unroll
      for (int k = 0; k < 6; k++) {
        const int col = 6 * (c - 1) + k;
        const double dk = d[col];
        y0 = y0 + row[col] * dk;
        y1 = y1 + row[NP + col] * dk;
        y2 = y2 + row[2 * NP + col] * dk;
      }
    }
    if (a.focal)
      for (int c = 0; c < C; c++) {
        double u, v;
        if (!baj_seen(o, c, u, v)) continue;
        const int col = 6 * (C - 1) + c;
        const double dk = d[col];
        y0 = y0 + row[col] * dk;
        y1 = y1 + row[NP + col] * dk;
        y2 = y2 + row[2 * NP + col] * dk;
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

__global__ __launch_bounds__(kT) void baj_finish_kernel(int64_t N, const double* __restrict__ X, const int32_t* __restrict__ part,
                                                        double scale, double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (p >= N) return;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const bool in = part[p] != 0;
#pragma unroll
  for (int k = 0; k < 3; k++) out[3 * p + k] = in ? X[3 * p + k] * scale : qnan;
}

}  // namespace

hipError_t launch_baj_start(int C, int64_t N, const double* obs, const double* Ptab, int given, double* X, int32_t* part,
                            hipStream_t stream) {
  hipLaunchKernelGGL(baj_start_kernel, dim3((unsigned)calib_partials(N)), dim3(kT), 0, stream, C, N, obs, Ptab, given, X, part);
  return hipGetLastError();
}

hipError_t launch_baj_linearise(const BajArgs& a, hipStream_t stream) {
  const int64_t P = calib_partials(a.N);
  hipError_t e;
  hipLaunchKernelGGL(baj_linearise_kernel, dim3((unsigned)P), dim3(kT), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_ba_gram(a.Jaug, a.m_pad, a.NP, a.partial, a.ksplit, a.G, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(baj_cameras_kernel, dim3((unsigned)P, (unsigned)a.C), dim3(kT), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(baj_cameras_final_kernel, dim3((unsigned)a.C), dim3(64), 0, stream, a, P);
  return hipGetLastError();
}

hipError_t launch_baj_backsub(const BajArgs& a, const double* delta, double* X_trial, hipStream_t stream) {
  hipLaunchKernelGGL(baj_backsub_kernel, dim3((unsigned)calib_partials(a.N)), dim3(kT), 0, stream, a, delta, X_trial);
  return hipGetLastError();
}

hipError_t launch_baj_finish(int64_t N, const double* X, const int32_t* part, double scale, double* X_out, hipStream_t stream) {
  hipLaunchKernelGGL(baj_finish_kernel, dim3((unsigned)calib_partials(N)), dim3(kT), 0, stream, N, X, part, scale, X_out);
  return hipGetLastError();
}

}  // namespace mocap
