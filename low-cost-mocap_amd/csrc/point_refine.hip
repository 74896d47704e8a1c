// point_refine.hip -- the "point refinement" section of include/mocap_core.h: each kept correspondence group re-triangulated by
// minimising the true reprojection error, every camera with its own K.  The core's own contract (the reference stops at the DLT
// point, helpers.py:293-327).
//
// One lane per point slot.  A lane recomputes its DLT start with the device functions tri_kernel uses (dlt_accumulate,
// solve_point: the same bits as mocap_triangulate), then walks csrc/refine_lm.hpp: `iters` Levenberg-Marquardt steps in FP64,
// accept and reject by select.  The loops over the cameras are wave-uniform and the table P [C][12] is addressed through the
// constant address space: one scalar-cache read per wave and camera.  A lane's observations are re-read per pass (corr row ->
// blob) instead of being kept: 64 cameras would not fit the registers, and a pass's loads do not depend on its arithmetic.  No LDS.
#include "frame_common.hpp"
#include "kernels.hpp"
#include "mocap_device.hpp"
#include "refine_lm.hpp"

namespace mocap {

namespace {

// The DLT start of a group whose views are all usable, then the steps.  -> the point's info word; X and e are the results when
// it carries kRfRefined.
template <bool UNIFORM_K, class Obs>
__device__ __forceinline__ int refine_group(const CamView& cv, ctab_t P, Obs&& obs, int iters, double (&X)[3], double& e) {
  const int C = cv.C;
  double B[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int v = 0;
  for (int c = 0; c < C; c++) {
    double x, y;
    if (obs(c, x, y)) {
      dlt_accumulate(B, cv.pq(UNIFORM_K ? (size_t)12 * c : 12 * ((size_t)v * C + c)), x, y);
      v++;
    }
  }
  solve_point(B, X);
  double cost = 0.0;
  int accepted = 0;
  if (!refine_lm(C, P, obs, iters, X, cost, accepted)) return kRfBadStart;
  e = cost / (double)(2 * v);
  return kRfRefined | (accepted << kRfStepsShift);
}

template <bool UNIFORM_K>
__global__ __launch_bounds__(kRefineThreads) void refine_frames_kernel(RefineArgs a) {
  const int C = a.cv.C;
  const ctab_t P = as_ctab(a.P);
  const int64_t total = a.n_frames * a.K_max;
  for (int64_t i = (int64_t)blockIdx.x * kRefineThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kRefineThreads) {
    const int64_t f = i / a.K_max;
    const int k = (int)(i - f * a.K_max);
    const int n = a.n_pts[f];
    const int st = a.status ? a.status[f] : 0;
    if ((st & kPcStatusSkip) || n < 0 || n > a.K_max || k >= n) {  // the frame is not processed, or the slot holds no point
      if (a.info) a.info[i] = 0;
      continue;
    }
    const int16_t* row = a.corr + (size_t)i * C;
    const float* fb = a.blobs + (size_t)f * C * a.M * 2;
    const int32_t* cnt = a.counts + (size_t)f * C;
    int flags = 0, v = 0;
    for (int c = 0; c < C; c++) {
      const int j = row[c];
      if (j < 0) continue;
      v++;
      if (j >= cnt[c] || j >= a.M) {
        flags |= kRfBadIndex;  // (the blob is not read)
      } else {
        const float* o = fb + ((size_t)c * a.M + j) * 2;
        if (!(rlm_finite((double)o[0]) && rlm_finite((double)o[1]))) flags |= kRfBadObs;
      }
    }
    if (v < 2) flags |= kRfFewViews;
    if (!flags) {
      auto obs = [&](int c, double& x, double& y) -> bool {
        const int j = row[c];
        if (j < 0) return false;
        const float* o = fb + ((size_t)c * a.M + j) * 2;  // (checked above: j < min(counts, M))
        x = (double)o[0];
        y = (double)o[1];
        return true;
      };
      double X[3], e = 0.0;
      flags = refine_group<UNIFORM_K>(a.cv, P, obs, a.iters, X, e);
      if (flags & kRfRefined) {
        FrameArgs fa;  // (store_point only looks at xyz and world)
        fa.xyz = a.xyz;
        fa.world = a.world;
        store_point(fa, (size_t)i, X);
        a.err[i] = e;
      }
    }
    if (a.info) a.info[i] = flags;
  }
}

template <bool UNIFORM_K>
__global__ __launch_bounds__(kRefineThreads) void refine_obs_kernel(RefineArgs a) {
  const int C = a.cv.C;
  const ctab_t P = as_ctab(a.P);
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  for (int64_t i = (int64_t)blockIdx.x * kRefineThreads + threadIdx.x; i < a.N; i += (int64_t)gridDim.x * kRefineThreads) {
    const double* o = a.obs + (size_t)i * C * 2;
    auto obs = [&](int c, double& x, double& y) -> bool {
      x = o[2 * c];
      y = o[2 * c + 1];
      return !(isnan(x) || isnan(y));  // mocap_triangulate's rule
    };
    int flags = 0, v = 0;
    for (int c = 0; c < C; c++) {
      double x, y;
      if (!obs(c, x, y)) continue;
      v++;
      if (!(rlm_finite(x) && rlm_finite(y))) flags |= kRfBadObs;
    }
    if (v < 2) flags |= kRfFewViews;
    double X[3] = {qnan, qnan, qnan}, e = qnan;
    if (!flags) {
      flags = refine_group<UNIFORM_K>(a.cv, P, obs, a.iters, X, e);
      if (!(flags & kRfRefined)) {
        X[0] = X[1] = X[2] = qnan;
        e = qnan;
      }
    }
    a.xyz[i * 3 + 0] = X[0];
    a.xyz[i * 3 + 1] = X[1];
    a.xyz[i * 3 + 2] = X[2];
    if (a.err) a.err[i] = e;
    if (a.info) a.info[i] = flags;
  }
}

}  // namespace

hipError_t launch_point_refine(const RefineArgs& a, hipStream_t stream) {
  const int64_t total = a.obs ? a.N : a.n_frames * a.K_max;
  if (total <= 0) return hipSuccess;
  int64_t blocks = (total + kRefineThreads - 1) / kRefineThreads;
  if (blocks > (1 << 20)) blocks = 1 << 20;  // the lanes stride over the rest
  void (*k)(RefineArgs);
  if (a.obs)
    k = a.cv.uniformK ? refine_obs_kernel<true> : refine_obs_kernel<false>;
  else
    k = a.cv.uniformK ? refine_frames_kernel<true> : refine_frames_kernel<false>;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kRefineThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
