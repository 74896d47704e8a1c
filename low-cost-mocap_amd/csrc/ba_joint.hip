// ba_joint.hip -- the kernels of the "joint bundle adjustment" section of include/mocap_core.h: camera poses, optional focal scales
// and all 3-D points as unknowns, analytic Jacobians, the points eliminated per lane (Schur complement).  The linearisation and the
// camera blocks are the kernels of csrc/ba_schur.hpp with this section's camera model (csrc/ba_joint.hpp); the three kernels that
// know no model are written here, for the lens calibration (csrc/ba_lens.hip) as well:
//   start      one lane per point: does it take part, and its DLT start (the device functions of mocap_triangulate, on a table of
//              each camera's own K [R | t])
//   backsub    one lane per point: X_trial = X - L^-T (z + E delta)
//   finish     one lane per point: the gauge factor on the points that take part, NaN for the others
// FP64 throughout, nothing fused, no atomics: every output is a function of the inputs alone.
#include "ba_joint.hpp"

namespace mocap {

namespace {

constexpr int kT = kCalibThreads;

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
    if (!schur_seen(o, c, u, v)) continue;
    views++;
    ok = ok && schur_finite(u) && schur_finite(v);
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
  ok = ok && schur_finite(x[0]) && schur_finite(x[1]) && schur_finite(x[2]);
  if (ok && !given) {  // the start lies in front of every camera that sees it
    for (int c = 0; c < C; c++) {
      double u, v;
      if (!schur_seen(o, c, u, v)) continue;
      const ctab_t Pc = P + 12 * c;
      const double w = ((Pc[8] * x[0] + Pc[9] * x[1]) + Pc[10] * x[2]) + Pc[11];
      ok = ok && schur_finite(w) && w > 0.0;
    }
  }
  part[p] = ok ? 1 : 0;
  if (!given) {
    X[3 * p] = ok ? x[0] : qnan;
    X[3 * p + 1] = ok ? x[1] : qnan;
    X[3 * p + 2] = ok ? x[2] : qnan;
  }
}

// ----------------------------------------------------------------------------------------------------------------- backsub
__global__ __launch_bounds__(kT) void schur_backsub_kernel(SchurArgs a, const double* delta, double* __restrict__ Xt) {
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (p >= a.N) return;
  double X[3] = {a.X[3 * p], a.X[3 * p + 1], a.X[3 * p + 2]};
  if (a.part[p] && !(a.flags[p] & kSchurPointSingular)) {
    const int C = a.C, NP = a.NP;
    const double* o = a.obs + (size_t)p * C * 2;
    const double* row = a.Jaug + (size_t)(3 * p) * NP;
    const ctab_t d = as_ctab(delta);
    double y0 = row[a.n_c], y1 = row[NP + a.n_c], y2 = row[2 * NP + a.n_c];
    // z + E delta over the columns in ascending order; the columns of a camera that does not see the point are zero
    for (int c = 1; c < C; c++) {
      double u, v;
      if (!schur_seen(o, c, u, v)) continue;
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
        if (!schur_seen(o, c, u, v)) continue;
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

hipError_t launch_baj_linearise(const SchurArgs& a, hipStream_t stream) { return schur_launch_linearise<BajModel>(a, stream); }

hipError_t launch_schur_backsub(const SchurArgs& a, const double* delta, double* X_trial, hipStream_t stream) {
  hipLaunchKernelGGL(schur_backsub_kernel, dim3((unsigned)calib_partials(a.N)), dim3(kT), 0, stream, a, delta, X_trial);
  return hipGetLastError();
}

hipError_t launch_baj_finish(int64_t N, const double* X, const int32_t* part, double scale, double* X_out, hipStream_t stream) {
  hipLaunchKernelGGL(baj_finish_kernel, dim3((unsigned)calib_partials(N)), dim3(kT), 0, stream, N, X, part, scale, X_out);
  return hipGetLastError();
}

}  // namespace mocap
