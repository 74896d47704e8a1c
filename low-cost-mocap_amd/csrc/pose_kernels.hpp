// pose_kernels.hpp -- the device part of the initial pose estimation (csrc/pose_init.hip holds the host replay of
// OpenCV's RANSAC loop around it):
//   real_cubic_roots     the root set of cv::solveCubic
//   seven_point_kernel   one lane per RANSAC sample -> up to 3 fundamental matrices
//   score_kernel         one workgroup per model -> inlier count (and the mask of model 0)
// and the two launchers that own the grid formulas.  A header so that the product library and the test-only probe
// (tests/native/pose_probe.hip) run the same code; everything has internal linkage: no symbol leaves either library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mocap {

static __device__ int real_cubic_roots(const double* c, double* x) {
  // real roots of c0 x^3 + c1 x^2 + c2 x + c3 (the root set of cv::solveCubic)
  if (c[0] == 0) {
    if (c[1] == 0) {
      if (c[2] == 0) return 0;
      x[0] = -c[3] / c[2];
      return 1;
    }
    double d = c[2] * c[2] - 4 * c[1] * c[3];
    if (d < 0) return 0;
    d = sqrt(d);
    x[0] = (-c[2] + d) / (2 * c[1]);
    x[1] = (-c[2] - d) / (2 * c[1]);
    return d > 0 ? 2 : 1;
  }
  const double a1 = c[1] / c[0], a2 = c[2] / c[0], a3 = c[3] / c[0];
  const double Q = (a1 * a1 - 3 * a2) / 9, R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) / 54;
  const double d = Q * Q * Q - R * R;
  const double pi = 3.14159265358979323846;
  if (d > 0) {
    const double theta = acos(R / sqrt(Q * Q * Q)), t0 = -2 * sqrt(Q);
    x[0] = t0 * cos(theta / 3) - a1 / 3;
    x[1] = t0 * cos((theta + 2 * pi) / 3) - a1 / 3;
    x[2] = t0 * cos((theta + 4 * pi) / 3) - a1 / 3;
    return 3;
  }
  if (d == 0) {
    const double e = -cbrt(R);
    x[0] = 2 * e - a1 / 3;
    x[1] = -e - a1 / 3;
    return 2;
  }
  double e = cbrt(sqrt(-d) + fabs(R));
  if (R > 0) e = -e;
  x[0] = (e + Q / e) - a1 / 3;
  return 1;
}

struct SevenArgs {
  int n_samples;
  const int32_t* idx;  // [n_samples][7]
  const float* p1;     // [N][2]
  const float* p2;
  double* F;           // [n_samples][3][9]
  int32_t* nF;         // [n_samples]
};

static __global__ __launch_bounds__(64) void seven_point_kernel(SevenArgs a) {
  __shared__ double A[63 * 64];  // [row * 9 + col][lane]
  __shared__ int perm[9 * 64];
  const int lane = threadIdx.x, s = blockIdx.x * 64 + lane;
  if (s >= a.n_samples) return;
  double* M = A + lane;
  int* pm = perm + lane;
  double x0[7], y0[7], x1[7], y1[7];
  double m1x = 0, m1y = 0, m2x = 0, m2y = 0;
  for (int i = 0; i < 7; i++) {
    const int k = a.idx[s * 7 + i];
    x0[i] = a.p1[2 * k];
    y0[i] = a.p1[2 * k + 1];
    x1[i] = a.p2[2 * k];
    y1[i] = a.p2[2 * k + 1];
    m1x += x0[i];
    m1y += y0[i];
    m2x += x1[i];
    m2y += y1[i];
  }
  const double inv7 = 1. / 7;
  m1x *= inv7;
  m1y *= inv7;
  m2x *= inv7;
  m2y *= inv7;
  double sc1 = 0, sc2 = 0;
  for (int i = 0; i < 7; i++) {
    sc1 += sqrt((x0[i] - m1x) * (x0[i] - m1x) + (y0[i] - m1y) * (y0[i] - m1y));
    sc2 += sqrt((x1[i] - m2x) * (x1[i] - m2x) + (y1[i] - m2y) * (y1[i] - m2y));
  }
  sc1 *= inv7;
  sc2 *= inv7;
  a.nF[s] = 0;
  if (sc1 < 1.1920928955078125e-07 || sc2 < 1.1920928955078125e-07) return;  // FLT_EPSILON
  sc1 = sqrt(2.) / sc1;
  sc2 = sqrt(2.) / sc2;
  for (int i = 0; i < 7; i++) {
    const double u0 = (x0[i] - m1x) * sc1, v0 = (y0[i] - m1y) * sc1, u1 = (x1[i] - m2x) * sc2, v1 = (y1[i] - m2y) * sc2;
    double* r = M + i * 9 * 64;
    r[0] = u1 * u0;
    r[64] = u1 * v0;
    r[128] = u1;
    r[192] = v1 * u0;
    r[256] = v1 * v0;
    r[320] = v1;
    r[384] = u0;
    r[448] = v0;
    r[512] = 1;
  }
  for (int c = 0; c < 9; c++) pm[c * 64] = c;
  // Gauss-Jordan with full pivoting -> [I | B] up to the column permutation
  double top = 0;
  for (int k = 0; k < 7; k++) {
    int pr = k, pc = k;
    double best = -1;
    for (int r = k; r < 7; r++)
      for (int c = k; c < 9; c++) {
        const double v = fabs(M[(r * 9 + c) * 64]);
        if (v > best) {
          best = v;
          pr = r;
          pc = c;
        }
      }
    // rank deficient sample: no model.  The test is relative to the system's largest entry: a repeated correspondence
    // leaves a pivot of rounding size (<= 1e-15 after Hartley normalisation), rarely an exact zero, and the "models" of
    // such a residue are noise; a sample that passed checkSubset has pivots twelve orders above the threshold.
    if (k == 0) top = best;
    if (!(best > 1e-13 * top)) return;
    if (pr != k)
      for (int c = 0; c < 9; c++) {
        const double t = M[(k * 9 + c) * 64];
        M[(k * 9 + c) * 64] = M[(pr * 9 + c) * 64];
        M[(pr * 9 + c) * 64] = t;
      }
    if (pc != k) {
      for (int r = 0; r < 7; r++) {
        const double t = M[(r * 9 + k) * 64];
        M[(r * 9 + k) * 64] = M[(r * 9 + pc) * 64];
        M[(r * 9 + pc) * 64] = t;
      }
      const int t = pm[k * 64];
      pm[k * 64] = pm[pc * 64];
      pm[pc * 64] = t;
    }
    const double ip = 1.0 / M[(k * 9 + k) * 64];
    for (int c = k; c < 9; c++) M[(k * 9 + c) * 64] *= ip;
    for (int r = 0; r < 7; r++) {
      if (r == k) continue;
      const double f = M[(r * 9 + k) * 64];
      if (f != 0)
        for (int c = k; c < 9; c++) M[(r * 9 + c) * 64] -= f * M[(k * 9 + c) * 64];
    }
  }
  double f1[9], f2[9];
  for (int c = 0; c < 9; c++) f1[c] = f2[c] = 0;
  for (int i = 0; i < 9; i++) {
    const int col = pm[i * 64];
    const double v1 = i < 7 ? -M[(i * 9 + 7) * 64] : (i == 7 ? 1.0 : 0.0);
    const double v2 = i < 7 ? -M[(i * 9 + 8) * 64] : (i == 8 ? 1.0 : 0.0);
#pragma unroll
    for (int c = 0; c < 9; c++)
      if (c == col) {
        f1[c] = v1;
        f2[c] = v2;
      }
  }
  // normalise the basis vectors (scale only: keeps the cubic's coefficients O(1))
  {
    double n1 = 0, n2 = 0;
    for (int c = 0; c < 9; c++) {
      n1 += f1[c] * f1[c];
      n2 += f2[c] * f2[c];
    }
    n1 = 1.0 / sqrt(n1);
    n2 = 1.0 / sqrt(n2);
    for (int c = 0; c < 9; c++) {
      f1[c] *= n1;
      f2[c] *= n2;
    }
  }
  for (int c = 0; c < 9; c++) f1[c] -= f2[c];
  double cf[4];
  {
    double t0 = f2[4] * f2[8] - f2[5] * f2[7], t1 = f2[3] * f2[8] - f2[5] * f2[6], t2 = f2[3] * f2[7] - f2[4] * f2[6];
    cf[3] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2;
    cf[2] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2 - f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) +
            f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) - f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) +
            f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) - f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
            f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]);
    t0 = f1[4] * f1[8] - f1[5] * f1[7];
    t1 = f1[3] * f1[8] - f1[5] * f1[6];
    t2 = f1[3] * f1[7] - f1[4] * f1[6];
    cf[0] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2;
    cf[1] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2 - f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) +
            f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) - f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) +
            f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) - f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
            f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]);
  }
  double roots[3];
  const int n = real_cubic_roots(cf, roots);
  double Fm[3][9];
  for (int k = 0; k < n; k++) {
    double lam = roots[k], mu = 1.0, g[9];
    const double sden = f1[8] * lam + f2[8];
    if (fabs(sden) > 2.220446049250313e-16) {
      mu = 1.0 / sden;
      lam *= mu;
      g[8] = 1.0;
    } else {
      g[8] = 0.0;
    }
    for (int i = 0; i < 8; i++) g[i] = f1[i] * lam + f2[i] * mu;
    // F = T2^T g T1,  T = [[s, 0, -s mx], [0, s, -s my], [0, 0, 1]]
    double h[9];  // g T1
    for (int r = 0; r < 3; r++) {
      h[3 * r] = g[3 * r] * sc1;
      h[3 * r + 1] = g[3 * r + 1] * sc1;
      h[3 * r + 2] = g[3 * r + 2] - sc1 * (g[3 * r] * m1x + g[3 * r + 1] * m1y);
    }
    double* Fo = Fm[k];
    for (int c = 0; c < 3; c++) {
      Fo[c] = sc2 * h[c];
      Fo[3 + c] = sc2 * h[3 + c];
      Fo[6 + c] = h[6 + c] - sc2 * (m2x * h[c] + m2y * h[3 + c]);
    }
    if (fabs(Fo[8]) > 1.1920928955078125e-07) {
      const double sc = 1.0 / Fo[8];
      for (int i = 0; i < 9; i++) Fo[i] *= sc;
    }
  }
  // order the models of one sample by F[0][0] (OpenCV's order depends on its SVD's basis of the null space)
  int ord[3] = {0, 1, 2};
  for (int i = 1; i < n; i++)
    for (int j = i; j > 0 && Fm[ord[j]][0] < Fm[ord[j - 1]][0]; j--) {
      const int t = ord[j];
      ord[j] = ord[j - 1];
      ord[j - 1] = t;
    }
  for (int k = 0; k < n; k++)
    for (int i = 0; i < 9; i++) a.F[((size_t)s * 3 + k) * 9 + i] = Fm[ord[k]][i];
  a.nF[s] = n;
}

struct ScoreArgs {
  int64_t N;
  const float* p1;
  const float* p2;
  const double* F;     // [n_models][9]
  const int32_t* nF;   // [n_models / 3] or null (then every model is scored)
  float t;             // (float)(thr * thr)
  int32_t* count;      // [n_models]
  uint8_t* mask;       // [N] or null: inlier mask of model 0
};

static __device__ __forceinline__ bool fm_inlier(const double* f, float x1f, float y1f, float x2f, float y2f, float t) {
  const double x1 = x1f, y1 = y1f, x2 = x2f, y2 = y2f;
  double a = f[0] * x1 + f[1] * y1 + f[2], b = f[3] * x1 + f[4] * y1 + f[5], c = f[6] * x1 + f[7] * y1 + f[8];
  const double s2 = 1. / (a * a + b * b), d2 = x2 * a + y2 * b + c;
  a = f[0] * x2 + f[3] * y2 + f[6];
  b = f[1] * x2 + f[4] * y2 + f[7];
  c = f[2] * x2 + f[5] * y2 + f[8];
  const double s1 = 1. / (a * a + b * b), d1 = x1 * a + y1 * b + c;
  const double e1 = d1 * d1 * s1, e2 = d2 * d2 * s2;
  const float err = (float)(e1 < e2 ? e2 : e1);  // std::max(e1, e2): e1 unless e1 < e2, so a NaN e1 (x2 the epipole) stays
  return err <= t;
}

static __global__ __launch_bounds__(256) void score_kernel(ScoreArgs a) {
  const int m = blockIdx.x;
  if (a.nF && (m % 3) >= a.nF[m / 3]) {
    if (threadIdx.x == 0) a.count[m] = 0;
    return;
  }
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  double f[9];
  for (int i = 0; i < 9; i++) f[i] = a.F[(size_t)m * 9 + i];
  int local = 0;
  for (int64_t i = threadIdx.x; i < a.N; i += 256) {
    const bool in = fm_inlier(f, a.p1[2 * i], a.p1[2 * i + 1], a.p2[2 * i], a.p2[2 * i + 1], a.t);
    local += in ? 1 : 0;
    if (a.mask && m == 0) a.mask[i] = in ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o);
  if ((threadIdx.x & 63) == 0) atomicAdd(&total, local);
  __syncthreads();
  if (threadIdx.x == 0) a.count[m] = total;
}

// ---------------------------------------------------------------------------------------- launchers
// one lane per sample, 64 samples per block
static inline void launch_seven_point(const SevenArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(seven_point_kernel, dim3((a.n_samples + 63) / 64), dim3(64), 0, stream, a);
}

// one block of 256 per model; a.nF (if any) gates the three slots of each sample
static inline void launch_score(const ScoreArgs& a, int n_models, hipStream_t stream) {
  hipLaunchKernelGGL(score_kernel, dim3(n_models), dim3(256), 0, stream, a);
}

}  // namespace mocap
