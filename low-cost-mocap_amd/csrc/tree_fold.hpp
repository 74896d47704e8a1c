// tree_fold.hpp -- the project's one reduction tree for sums over frames or points (the calibration tail's, csrc/calib_tail.hip), as
// templates over the number of values a lane carries: body_learn.hip and ba_joint.hip reduce through these.
//   lane -> wave by __shfl_down (offsets 32 .. 1), wave -> workgroup through LDS in wave order, one partial per workgroup into a
//   slab, one wave whose lane l folds the slab entries [l * ceil(P / 64), ...) in index order before the same shuffle tree.
// No atomics: every value is a function of the inputs and of the item count alone.  Workgroups of kCalibThreads lanes.
#pragma once
#include "kernels.hpp"
#include "mocap_device.hpp"

namespace mocap {

constexpr int kFoldWaves = kCalibThreads / 64;

// lane 0 of the wave ends up with the sum of all 64 lanes; entry kMin (if any) with the minimum
template <int n, int kMin>
__device__ __forceinline__ void wave_fold(double (&v)[n]) {
  for (int off = 32; off; off >>= 1) {
#pragma unroll
    for (int i = 0; i < n; i++) {
      const double o = __shfl_down(v[i], off);
      v[i] = i == kMin ? (o < v[i] ? o : v[i]) : v[i] + o;
    }
  }
}

// every lane's v -> out[0 .. n) of this workgroup's slab entry (thread 0 writes); s: [kFoldWaves][n] doubles of LDS
template <int n, int kMin>
__device__ __forceinline__ void block_fold(double (&v)[n], double (*s)[n], double* out) {
  wave_fold<n, kMin>(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < n; i++) s[wave][i] = v[i];
  }
  block_sync_lds();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kFoldWaves; w++) {
#pragma unroll
      for (int i = 0; i < n; i++) {
        const double o = s[w][i];
        v[i] = i == kMin ? (o < v[i] ? o : v[i]) : v[i] + o;
      }
    }
#pragma unroll
    for (int i = 0; i < n; i++) out[i] = v[i];
  }
}

// the one wave of a final launch: slab [P][n] -> v of lane 0; `init` = the neutral element of entry kMin
template <int n, int kMin>
__device__ __forceinline__ void slab_fold(const double* slab, int64_t P, double init, double (&v)[n]) {
  const int64_t chunk = (P + 63) / 64, lo = threadIdx.x * chunk, hi = lo + chunk < P ? lo + chunk : P;
#pragma unroll
  for (int i = 0; i < n; i++) v[i] = i == kMin ? init : 0.0;
  for (int64_t e = lo; e < hi; e++) {
#pragma unroll
    for (int i = 0; i < n; i++) {
      const double o = slab[e * n + i];
      v[i] = i == kMin ? (o < v[i] ? o : v[i]) : v[i] + o;
    }
  }
  wave_fold<n, kMin>(v);
}

}  // namespace mocap
