// track_smooth.hip -- a recorded session as one time series per marker (include/mocap_core.h, "trajectories").
//   gather   xyz [F][K_max][3] + id [F][K_max] (the marker tracker's) -> traj [R][F][3], time contiguous within a row.  One lane per
//            frame: it writes NaN into its frame of every row, then walks its slots from the highest down and stores each qualifying
//            point into its row, so that the lowest slot is the store that stays (one lane's stores to one address keep their order).
//            Consecutive lanes write consecutive frames of a row: 24-byte stores side by side.  No atomics.
//   good     the good-time bit of every frame, a prefix maximum over t in three launches (the largest finite t per tile of 256 frames;
//            one workgroup turns the tile maxima into "largest before the tile"; the bits): block_scan.hpp's prefix and tile scan,
//            shared with the body trajectories' sign rule.  A maximum is exact in any order.
//   smooth   one workgroup of 256 lanes per 256 consecutive frames of one row, grid ceil(F / 256) x R.  The staging (t [320], x, y, z
//            [3][320] and one byte of bits per frame, 10.3 KB of LDS), the fit and the residual walk are window_fit.hpp's with three
//            channels, shared with the rotation smoother (body_session.hip); this kernel keeps what it makes of the coefficients:
//            pos, vel, acc and res (DESIGN.md 3.7n has the code object's figures).
// FP64 throughout, nothing fused (-ffp-contract=off is the build's rule), / and sqrt correctly rounded: the outputs are a function of
// the inputs alone, and equal to the scalar statement of the contract bit for bit.
#include "track_smooth.hpp"
#include "block_scan.hpp"
#include "mocap_device.hpp"
#include "window_fit.hpp"

namespace mocap {

namespace {

constexpr int kT = kTsTile;

// ------------------------------------------------------------------------------------------------------------------ gather
__global__ __launch_bounds__(kT) void ts_gather_kernel(GatherTracksArgs a) {
  const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (f >= a.n_frames) return;
  const double nan = __builtin_nan("");
  for (int r = 0; r < a.R; r++) {
    double* o = a.traj + ((size_t)r * a.n_frames + f) * 3;
    o[0] = nan;
    o[1] = nan;
    o[2] = nan;
  }
  int n = a.n_pts[f];
  if (n < 0 || n > a.K_max) n = 0;
  const int32_t* ids = a.id + (size_t)f * a.K_max;
  const int32_t* hits = a.hits ? a.hits + (size_t)f * a.K_max : nullptr;
  const double* P = a.xyz + (size_t)f * a.K_max * 3;
  for (int j = n - 1; j >= 0; j--) {  // descending: the lowest qualifying slot of a row is written last
    const int32_t i = ids[j];
    if (i < 0 || i >= a.n_ids) continue;
    const int32_t r = a.relabel[i];
    if (r < 0 || r >= a.R) continue;
    if (hits && hits[j] < a.min_hits) continue;
    if (!finiteN<3>(P + 3 * j)) continue;
    double* o = a.traj + ((size_t)r * a.n_frames + f) * 3;
    o[0] = P[3 * j];
    o[1] = P[3 * j + 1];
    o[2] = P[3 * j + 2];
  }
}

// ------------------------------------------------------------------------------------------------------------------ good times
__device__ __forceinline__ double finite_or_low(const GoodTimesArgs& a, int64_t f) {
  const double v = f < a.n_frames ? a.t[f] : -__builtin_inf();
  return finite1(v) ? v : -__builtin_inf();
}

__global__ __launch_bounds__(kT) void ts_tile_max_kernel(GoodTimesArgs a) {
  __shared__ double s[kT];
  const double m = block_prefix<OpMaxF64>(finite_or_low(a, (int64_t)blockIdx.x * kT + threadIdx.x), s);
  if (threadIdx.x == kT - 1) a.tile_max[blockIdx.x] = m;
}

__global__ __launch_bounds__(kT) void ts_good_kernel(GoodTimesArgs a) {
  __shared__ double s[kT];
  const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
  block_prefix<OpMaxF64>(finite_or_low(a, f), s);
  if (f >= a.n_frames) return;
  const double before_tile = a.tile_max[blockIdx.x], in_tile = threadIdx.x > 0 ? s[threadIdx.x - 1] : -__builtin_inf();
  const double before = in_tile > before_tile ? in_tile : before_tile, v = a.t[f];
  a.good[f] = finite1(v) && v > before ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------ smooth
template <int D>
__global__ __launch_bounds__(kT) void ts_smooth_kernel(SmoothTracksArgs a) {
  __shared__ WfStage<3> s;
  const int r = blockIdx.y;
  const int64_t F = a.n_frames, f0 = (int64_t)blockIdx.x * kT, f = f0 + threadIdx.x;
  wf_stage<3>(a, a.traj + (size_t)r * F * 3, f0, s);
  if (f >= F) return;

  const double nan = __builtin_nan("");
  const int c = threadIdx.x + a.W;  // this lane's frame among the staged ones
  double out[10];                   // pos, vel, acc, res
#pragma unroll
  for (int i = 0; i < 10; i++) out[i] = nan;
  int n;
  double h, cf[D + 1][3];
  const int flag = wf_fit<3, D>(a, s, c, n, h, cf);
  if (flag & (kTsSmoothed | kTsFilled)) {
    const double ss = wf_residual<3, D>(a, s, c, h, cf);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      out[k] = cf[0][k];
      out[3 + k] = cf[1][k] / h;
      if constexpr (D >= 2) out[6 + k] = ((2.0 * cf[2][k]) / h) / h;
    }
    out[9] = sqrt(ss / (double)(3 * n));
  }
  const size_t o = (size_t)r * F + f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    a.pos[3 * o + k] = out[k];
    a.vel[3 * o + k] = out[3 + k];
    a.acc[3 * o + k] = out[6 + k];
  }
  a.res[o] = out[9];
  a.n_used[o] = n;
  a.flag[o] = flag;
}

}  // namespace

hipError_t launch_gather_tracks(const GatherTracksArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(ts_gather_kernel, dim3((unsigned)ts_tiles(a.n_frames)), dim3(kT), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_good_times(const GoodTimesArgs& a, hipStream_t stream) {
  const int64_t P = ts_tiles(a.n_frames);
  const dim3 tiles((unsigned)P), block(kT), one(1);
  hipError_t e;
  hipLaunchKernelGGL(ts_tile_max_kernel, tiles, block, 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(tile_scan_kernel<OpMaxF64>, one, block, 0, stream, a.tile_max, P);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(ts_good_kernel, tiles, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_smooth_tracks(const SmoothTracksArgs& a, hipStream_t stream) {
  const dim3 block(kT), grid((unsigned)ts_tiles(a.n_frames), (unsigned)a.R);
  if (a.degree == 1) hipLaunchKernelGGL(ts_smooth_kernel<1>, grid, block, 0, stream, a);
  else if (a.degree == 2) hipLaunchKernelGGL(ts_smooth_kernel<2>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(ts_smooth_kernel<3>, grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
