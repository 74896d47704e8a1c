// block_scan.hpp -- a prefix over the frames of a session in three launches, as the session stages use it (track_smooth.hip: the
// largest finite time before a frame; body_session.hip: the last POSED frame before a frame and the parity of the flips up to
// it): each workgroup of kTsTile lanes folds its tile, one workgroup per sequence turns the tile values into "the fold of the
// tiles before", and the stage's own kernel combines that with the prefix inside its tile.  The operations are exact in any order
// (maximum, exclusive or), so the tree's shape does not show in the result.  Device code only.
#pragma once
#include "track_smooth.hpp"

namespace mocap {

// An operation: its value type T, its neutral element kNone and op(x, y).
struct OpMaxF64 {
  using T = double;
  static constexpr double kNone = -__builtin_inf();
  __device__ static double op(double x, double y) { return x > y ? x : y; }
};
struct OpMaxI32 {
  using T = int32_t;
  static constexpr int32_t kNone = -1;  // of frame numbers: "none"
  __device__ static int32_t op(int32_t x, int32_t y) { return x > y ? x : y; }
};
struct OpXor {
  using T = int32_t;
  static constexpr int32_t kNone = 0;
  __device__ static int32_t op(int32_t x, int32_t y) { return x ^ y; }
};

// inclusive prefix over the workgroup's kTsTile values (Hillis-Steele through LDS); every lane calls it
template <class Op, class T = typename Op::T>
__device__ __forceinline__ T block_prefix(T v, T* s) {
  const int l = threadIdx.x;
  s[l] = v;
  __syncthreads();
  for (int d = 1; d < kTsTile; d <<= 1) {
    const T o = l >= d ? s[l - d] : Op::kNone;
    __syncthreads();
    v = Op::op(o, v);
    s[l] = v;
    __syncthreads();
  }
  return v;
}

// one workgroup per sequence of P tile values: tile[p] becomes the fold of the tiles before p (kNone for none).  Lane l owns the
// entries [l * per, (l + 1) * per).
template <class Op, class T = typename Op::T>
__global__ __launch_bounds__(kTsTile) void tile_scan_kernel(T* tiles, int64_t P) {
  __shared__ T s[kTsTile];
  T* tile = tiles + (size_t)blockIdx.x * P;
  const int64_t per = (P + kTsTile - 1) / kTsTile, lo = threadIdx.x * per, hi = lo + per < P ? lo + per : P;
  T m = Op::kNone;
  for (int64_t p = lo; p < hi; p++) m = Op::op(m, tile[p]);
  block_prefix<Op>(m, s);
  T run = threadIdx.x > 0 ? s[threadIdx.x - 1] : Op::kNone;
  for (int64_t p = lo; p < hi; p++) {
    const T own = tile[p];
    tile[p] = run;
    run = Op::op(run, own);
  }
}

}  // namespace mocap
