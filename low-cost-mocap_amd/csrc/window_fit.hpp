// window_fit.hpp -- the windowed polynomial fit of the session smoothers (include/mocap_core.h, "trajectories"), for samples of C
// doubles and degree D: the marker rows (track_smooth.hip, C = 3) and the bodies' quaternions (body_session.hip, C = 4).  One
// workgroup of kTsTile lanes per kTsTile consecutive frames of one row; the tile and a halo of W frames on either side are staged once
// in LDS as planes (neighbouring lanes read neighbouring doubles, no bank conflict) with one byte of bits per frame; each lane then
// walks its own window out of LDS: count / h / the nearest present frames, the power sums and right-hand sides, and -- once the
// caller has looked at the coefficients -- the residual.  The power sums, right-hand sides, the Cholesky factor and the coefficients
// are arrays indexed by unrolled loops over the template parameters: registers, no scratch.  FP64 throughout, nothing fused
// (-ffp-contract=off is the build's rule), / and sqrt correctly rounded.  `a` is the kernel's argument structure, of which the
// window's parameters are read: n_frames, t, good, W, span, n_min, max_gap.  Device code only.
#pragma once
#include "track_smooth.hpp"

namespace mocap {

constexpr int kStage = kTsTile + 2 * kTsMaxHalfWindow;  // frames of a tile with its halo at the largest W
constexpr int kGood = 1, kPresent = 2;  // bits of a staged frame

template <int C>
struct WfStage {  // a tile with its halo; staged index i = frame f0 - W + i
  double t[kStage];
  double x[C][kStage];
  uint8_t ok[kStage];
};

// every lane of the workgroup: the frames f0 - W .. f0 + kTsTile + W - 1 of `row` ([F][C]) into s; ends with the barrier
template <int C, class Args>
__device__ __forceinline__ void wf_stage(const Args& a, const double* row, int64_t f0, WfStage<C>& s) {
  const int W = a.W;
  for (int i = threadIdx.x; i < kTsTile + 2 * W; i += kTsTile) {
    const int64_t g = f0 - W + i;
    double tv = 0.0, x[C];
#pragma unroll
    for (int k = 0; k < C; k++) x[k] = 0.0;
    int bits = 0;
    if (g >= 0 && g < a.n_frames) {
      tv = a.t[g];
#pragma unroll
      for (int k = 0; k < C; k++) x[k] = row[C * g + k];
      if (a.good[g]) bits = finiteN<C>(x) ? kGood | kPresent : kGood;
    }
    s.t[i] = tv;
#pragma unroll
    for (int k = 0; k < C; k++) s.x[k][i] = x[k];
    s.ok[i] = (uint8_t)bits;
  }
  __syncthreads();
}

// The fit of the lane whose frame is the staged frame c (its window: the staged frames c - W .. c + W).  -> the frame's flag:
// BAD_TIME, 0 (absent and not fillable), FEW, SINGULAR (a failed pivot), or SMOOTHED / FILLED with the coefficients cf in
// u = (t - t_f) / h.  n (the samples in the window) and h are set on every path but BAD_TIME's, where they stay 0.
template <int C, int D, class Args>
__device__ __forceinline__ int wf_fit(const Args& a, const WfStage<C>& s, int c, int& n, double& h, double (&cf)[D + 1][C]) {
  const int W = a.W;
  const double tf = s.t[c];
  n = 0;
  h = 0.0;
  if (!(s.ok[c] & kGood)) return kTsBadTime;
  int ja = 0, jb = 0;  // offsets of the nearest present frames below and above, 0 = none in the window
  bool sa = false, sb = false;
  for (int j = -W; j <= W; j++) {
    if (!(s.ok[c + j] & kPresent)) continue;
    const double as = fabs(s.t[c + j] - tf);
    const bool in = as <= a.span;
    if (in) {
      n++;
      h = as > h ? as : h;
    }
    if (j < 0) {
      ja = j;
      sa = in;
    } else if (j > 0 && jb == 0) {
      jb = j;
      sb = in;
    }
  }
  const bool present = s.ok[c] & kPresent;
  const bool fillable = !present && a.max_gap > 0 && ja != 0 && jb != 0 && jb - ja - 1 <= a.max_gap && sa && sb;
  if (!present && !fillable) return 0;
  if (n < a.n_min) return kTsFew;
  double S[2 * D + 1], B[D + 1][C];
#pragma unroll
  for (int i = 0; i <= 2 * D; i++) S[i] = 0.0;
#pragma unroll
  for (int i = 0; i <= D; i++)
#pragma unroll
    for (int k = 0; k < C; k++) B[i][k] = 0.0;
  for (int j = -W; j <= W; j++) {
    if (!(s.ok[c + j] & kPresent)) continue;
    const double d = s.t[c + j] - tf;
    if (!(fabs(d) <= a.span)) continue;
    const double u = d / h;
    double x[C];
#pragma unroll
    for (int k = 0; k < C; k++) x[k] = s.x[k][c + j];
    double p = 1.0;
#pragma unroll
    for (int i = 0; i <= 2 * D; i++) {
      S[i] = S[i] + p;
      if (i <= D) {
#pragma unroll
        for (int k = 0; k < C; k++) B[i][k] = B[i][k] + p * x[k];
      }
      p = p * u;
    }
  }
  // A_ij = S_{i+j} = L L^T, row by row
  double L[D + 1][D + 1];
  bool ok = true;
#pragma unroll
  for (int i = 0; i <= D; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      double v = S[i + j];
#pragma unroll
      for (int k = 0; k < j; k++) v = v - L[i][k] * L[j][k];
      if (j == i) {
        if (!(v > 0.0 && v < __builtin_inf())) ok = false;
        L[i][i] = sqrt(v);
      } else {
        L[i][j] = v / L[j][j];
      }
    }
  if (!ok) return kTsSingular;
#pragma unroll
  for (int k = 0; k < C; k++) {
    double y[D + 1];
#pragma unroll
    for (int i = 0; i <= D; i++) {
      double v = B[i][k];
#pragma unroll
      for (int m = 0; m < i; m++) v = v - L[i][m] * y[m];
      y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = D; i >= 0; i--) {
      double v = y[i];
#pragma unroll
      for (int m = i + 1; m <= D; m++) v = v - L[m][i] * cf[m][k];
      cf[i][k] = v / L[i][i];
    }
  }
  return present ? kTsSmoothed : kTsFilled;
}

// the sum of the squared residuals of a fit over its window, channel by channel within a frame
template <int C, int D, class Args>
__device__ __forceinline__ double wf_residual(const Args& a, const WfStage<C>& s, int c, double h, const double (&cf)[D + 1][C]) {
  const int W = a.W;
  const double tf = s.t[c];
  double ss = 0.0;
  for (int j = -W; j <= W; j++) {
    if (!(s.ok[c + j] & kPresent)) continue;
    const double d = s.t[c + j] - tf;
    if (!(fabs(d) <= a.span)) continue;
    const double u = d / h;
#pragma unroll
    for (int k = 0; k < C; k++) {
      double q = cf[D][k];
#pragma unroll
      for (int i = D - 1; i >= 0; i--) q = q * u + cf[i][k];
      const double e = s.x[k][c + j] - q;
      ss = ss + e * e;
    }
  }
  return ss;
}

}  // namespace mocap
