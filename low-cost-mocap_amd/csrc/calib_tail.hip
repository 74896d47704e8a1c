// calib_tail.hip -- the arithmetic of the reference's calibration tail over a whole capture, read in place from the frame
// path's outputs (xyz [F][K_max][3], n_pts [F], status [F]):
//   pair scale    `determine-scale` (computer_code/api/index.py:290-309): the distance of every frame that holds exactly two
//                 points, its sum and count (the mean and 0.15 / mean are taken by the final launch);
//   floor factor  `acquire-floor` (index.py:158-194): the R factor of the QR of [x y 1 | z] over every point (TSQR), from
//                 which mocap_floor_from_factor back-substitutes the plane z = a x + b y + c.
//
// Valid-slot rule (post_kernels.hip, locate_objects_kernel): a frame contributes when status[f] == 0 (if a status array is
// given) and 0 <= n_pts[f] <= K_max; slots >= n_pts[f] are never read.
//
// Determinism.  One lane per frame, kCalibThreads frames per workgroup, grid = ceil(F / kCalibThreads): a function of F alone.
// Every reduction has one shape: lane -> wave (__shfl_down, offsets 32 .. 1), wave -> workgroup (LDS, wave 0 .. 3 in order),
// workgroup -> slab in HBM, and a final launch of ONE wave whose lane l folds slab entries [l * ceil(P / 64), ...) in index order
// before the same __shfl_down tree.  No atomics, nothing depends on the CU count or on which workgroup ran first: the bits are
// the same from run to run and from machine to machine (sqrt and / are correctly rounded; -ffp-contract=off: no fused a*b+c).
//
// Both kernels are launch- and memory-bound (24 B per valid point).  The reads are NOT coalesced: a lane reads the contiguous run
// of its own frame's valid slots, neighbouring lanes are 24 * K_max bytes apart, a wave touches 64 lines per load.  Left so: with a
// handful of valid points per frame a cooperative read of one frame would idle most of the wave, and two launches over a few MB
// are launch-bound either way.
#include "kernels.hpp"

namespace mocap {

namespace {

constexpr int kT = kCalibThreads, kWaves = kCalibThreads / 64;

// points of frame f, -1 = the frame has no valid slot
__device__ __forceinline__ int valid_points(const CalibTailArgs& a, int64_t f) {
  if (a.status && a.status[f] != 0) return -1;
  const int n = a.n_pts[f];
  return (n < 0 || n > a.K_max) ? -1 : n;
}

// ------------------------------------------------------------------------------------------------------------- pair scale
__global__ __launch_bounds__(kT) void pair_scale_kernel(CalibTailArgs a) {
  __shared__ double s_sum[kWaves];
  __shared__ int s_pairs[kWaves], s_skipped[kWaves];
  const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
  double d = 0.0;
  int pairs = 0, skipped = 0;
  if (f < a.n_frames) {
    const int n = valid_points(a, f);
    skipped = n < 0 ? 1 : 0;
    double out = __builtin_nan("");
    if (n == 2) {
      const double* P = a.xyz + (size_t)f * a.K_max * 3;
      const double dx = P[0] - P[3], dy = P[1] - P[4], dz = P[2] - P[5];
      d = sqrt((dx * dx + dy * dy) + dz * dz);  // np.sqrt(np.sum((p0 - p1)**2)), index.py:303
      out = d;
      pairs = 1;
    }
    if (a.pair_dist) a.pair_dist[f] = out;
  }
  for (int off = 32; off; off >>= 1) {
    d = d + __shfl_down(d, off);
    pairs += __shfl_down(pairs, off);
    skipped += __shfl_down(skipped, off);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_sum[wave] = d;
    s_pairs[wave] = pairs;
    s_skipped[wave] = skipped;
  }
  block_sync_lds();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; w++) {
      d = d + s_sum[w];
      pairs += s_pairs[w];
      skipped += s_skipped[w];
    }
    double* out = a.slab + (size_t)blockIdx.x * kPairSlabDoubles;
    out[0] = d;
    out[1] = (double)pairs;
    out[2] = (double)skipped;
  }
}

// one wave: slab [P][3] -> result {scale factor, mean distance, pairs, frames skipped}
__global__ __launch_bounds__(64) void pair_scale_final_kernel(const double* slab, int64_t P, double actual_distance,
                                                              double* result) {
  const int64_t chunk = (P + 63) / 64, lo = threadIdx.x * chunk, hi = lo + chunk < P ? lo + chunk : P;
  double s = 0.0, pairs = 0.0, skipped = 0.0;
  for (int64_t i = lo; i < hi; i++) {
    s = s + slab[i * kPairSlabDoubles + 0];
    pairs += slab[i * kPairSlabDoubles + 1];
    skipped += slab[i * kPairSlabDoubles + 2];
  }
  for (int off = 32; off; off >>= 1) {
    s = s + __shfl_down(s, off);
    pairs += __shfl_down(pairs, off);
    skipped += __shfl_down(skipped, off);
  }
  if (threadIdx.x == 0) {
    const double mean = s / pairs;  // no pair: 0 / 0 = NaN, np.mean([]) (index.py:305)
    result[0] = actual_distance / mean;
    result[1] = mean;
    result[2] = pairs;
    result[3] = skipped;
  }
}

// ----------------------------------------------------------------------------------------------------------- floor factor
// 4 x 4 upper-triangular factor of the rows folded so far (the strict lower triangle is never touched)
struct Tri {
  double r[4][4];
};

__device__ __forceinline__ void tri_zero(Tri& T) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) T.r[i][j] = 0.0;
}

// QR update with one row whose first K0 entries are zero: a Givens rotation per remaining column.  The rotated diagonal is
// sqrt(r^2 + v^2) >= 0, so a factor built from zero has a non-negative diagonal throughout.
template <int K0>
__device__ __forceinline__ void fold_row(Tri& T, double (&v)[4]) {
#pragma unroll
  for (int k = K0; k < 4; k++) {
    if (v[k] != 0.0) {
      const double rkk = T.r[k][k];
      const double h = sqrt(rkk * rkk + v[k] * v[k]);
      const double c = rkk / h, s = v[k] / h;
      T.r[k][k] = h;
#pragma unroll
      for (int j = k + 1; j < 4; j++) {
        const double t = c * T.r[k][j] + s * v[j];
        v[j] = c * v[j] - s * T.r[k][j];
        T.r[k][j] = t;
      }
    }
  }
}

// QR of two stacked triangles: the rows of B folded into T, top row first
__device__ __forceinline__ void fold_tri(Tri& T, const Tri& B) {
  {
    double v[4] = {B.r[0][0], B.r[0][1], B.r[0][2], B.r[0][3]};
    fold_row<0>(T, v);
  }
  {
    double v[4] = {0.0, B.r[1][1], B.r[1][2], B.r[1][3]};
    fold_row<1>(T, v);
  }
  {
    double v[4] = {0.0, 0.0, B.r[2][2], B.r[2][3]};
    fold_row<2>(T, v);
  }
  {
    double v[4] = {0.0, 0.0, 0.0, B.r[3][3]};
    fold_row<3>(T, v);
  }
}

// lane 0 of the wave ends up with the factor and the point count of all 64 lanes
__device__ __forceinline__ void wave_fold(Tri& T, double& n) {
  for (int off = 32; off; off >>= 1) {
    Tri B;
    tri_zero(B);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = i; j < 4; j++) B.r[i][j] = __shfl_down(T.r[i][j], off);
    n += __shfl_down(n, off);
    fold_tri(T, B);
  }
}

// the 10 entries of the upper triangle, row-major, then the point count
__device__ __forceinline__ void tri_store(const Tri& T, double n, double* out) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = i; j < 4; j++) out[k++] = T.r[i][j];
  out[10] = n;
}

__device__ __forceinline__ double tri_load(Tri& T, const double* in) {
  tri_zero(T);
  int k = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = i; j < 4; j++) T.r[i][j] = in[k++];
  return in[10];
}

__global__ __launch_bounds__(kT) void floor_factor_kernel(CalibTailArgs a) {
  __shared__ double s_tri[kWaves][kFloorSlabDoubles];
  const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
  Tri T;
  tri_zero(T);
  double n = 0.0;
  if (f < a.n_frames) {
    const int np = valid_points(a, f);
    const double* P = a.xyz + (size_t)f * a.K_max * 3;
    for (int i = 0; i < np; i++) {
      double v[4] = {P[3 * i + 0], P[3 * i + 1], 1.0, P[3 * i + 2]};  // [x, y, 1 | z]: tmp_A, tmp_b of index.py:166-168
      fold_row<0>(T, v);
    }
    n = np > 0 ? (double)np : 0.0;
  }
  wave_fold(T, n);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) tri_store(T, n, s_tri[wave]);
  block_sync_lds();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; w++) {
      Tri B;
      n += tri_load(B, s_tri[w]);
      fold_tri(T, B);
    }
    tri_store(T, n, a.slab + (size_t)blockIdx.x * kFloorSlabDoubles);
  }
}

// one wave: slab [P][11] -> factor [17] = R row-major (zeros below the diagonal), then the point count
__global__ __launch_bounds__(64) void floor_factor_final_kernel(const double* slab, int64_t P, double* factor) {
  const int64_t chunk = (P + 63) / 64, lo = threadIdx.x * chunk, hi = lo + chunk < P ? lo + chunk : P;
  Tri T;
  tri_zero(T);
  double n = 0.0;
  for (int64_t i = lo; i < hi; i++) {
    Tri B;
    n += tri_load(B, slab + i * kFloorSlabDoubles);
    fold_tri(T, B);
  }
  wave_fold(T, n);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) factor[4 * i + j] = j >= i ? T.r[i][j] : 0.0;
    factor[16] = n;
  }
}

}  // namespace

hipError_t launch_pair_scale(const CalibTailArgs& a, double actual_distance, double* result, hipStream_t stream) {
  const int64_t P = calib_partials(a.n_frames);
  if (P > 0) {
    hipLaunchKernelGGL(pair_scale_kernel, dim3((unsigned)P), dim3(kT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(pair_scale_final_kernel, dim3(1), dim3(64), 0, stream, (const double*)a.slab, P, actual_distance, result);
  return hipGetLastError();
}

hipError_t launch_floor_factor(const CalibTailArgs& a, double* factor, hipStream_t stream) {
  const int64_t P = calib_partials(a.n_frames);
  if (P > 0) {
    hipLaunchKernelGGL(floor_factor_kernel, dim3((unsigned)P), dim3(kT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(floor_factor_final_kernel, dim3(1), dim3(64), 0, stream, (const double*)a.slab, P, factor);
  return hipGetLastError();
}

}  // namespace mocap
