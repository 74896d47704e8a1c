// track_smooth.hip -- a recorded session as one time series per marker (include/mocap_core.h, "trajectories").
//   gather   xyz [F][K_max][3] + id [F][K_max] (the marker tracker's) -> traj [R][F][3], time contiguous within a row.  One lane per
//            frame: it writes NaN into its frame of every row, then walks its slots from the highest down and stores each qualifying
//            point into its row, so that the lowest slot is the store that stays (one lane's stores to one address keep their order).
//            Consecutive lanes write consecutive frames of a row: 24-byte stores side by side.  No atomics.
//   good     the good-time bit of every frame, a prefix maximum over t in three launches (the largest finite t per tile of 256 frames;
//            one workgroup turns the tile maxima into "largest before the tile"; the bits).  A maximum is exact in any order.
//   smooth   one workgroup of 256 lanes per 256 consecutive frames of one row, grid ceil(F / 256) x R.  The tile and a halo of W frames
//            on either side are staged once in LDS as t [320], x, y, z [3][320] (planes: neighbouring lanes read neighbouring doubles,
//            no bank conflict) and one byte of bits per frame, 10.3 KB.  Each lane then walks its own window out of LDS three times:
//            count / h / the nearest present frames, the power sums and right-hand sides, the residual.  The 7 power sums, 12
//            right-hand sides, the Cholesky factor and the 12 coefficients are arrays indexed by unrolled loops over a template
//            parameter (the degree): registers, no scratch (DESIGN.md 3.7n has the code object's figures).
// FP64 throughout, nothing fused (-ffp-contract=off is the build's rule), / and sqrt correctly rounded: the outputs are a function of
// the inputs alone, and equal to the scalar statement of the contract bit for bit.
#include "track_smooth.hpp"
#include "mocap_device.hpp"

namespace mocap {

namespace {

constexpr int kT = kTsTile;
constexpr int kStage = kTsTile + 2 * kTsMaxHalfWindow;  // frames of a tile with its halo at the largest W
constexpr int kTsSmoothed = 1, kTsFilled = 2, kTsFew = 4, kTsSingular = 8, kTsBadTime = 16;  // mirrored from include/mocap_core.h (MOCAP_TS_*)
constexpr int kGood = 1, kPresent = 2;  // bits of a staged frame

__device__ __forceinline__ bool finite1(double v) { return fabs(v) < __builtin_inf(); }  // false for NaN
__device__ __forceinline__ bool finite3(const double* p) { return finite1(p[0]) && finite1(p[1]) && finite1(p[2]); }

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
    if (!finite3(P + 3 * j)) continue;
    double* o = a.traj + ((size_t)r * a.n_frames + f) * 3;
    o[0] = P[3 * j];
    o[1] = P[3 * j + 1];
    o[2] = P[3 * j + 2];
  }
}

// ------------------------------------------------------------------------------------------------------------------ good times
// inclusive prefix maximum over the workgroup's 256 values (Hillis-Steele through LDS); every lane calls it
__device__ __forceinline__ double block_prefix_max(double v, double* s) {
  const int l = threadIdx.x;
  s[l] = v;
  __syncthreads();
  for (int d = 1; d < kT; d <<= 1) {
    const double o = l >= d ? s[l - d] : v;
    __syncthreads();
    v = o > v ? o : v;
    s[l] = v;
    __syncthreads();
  }
  return v;
}

__device__ __forceinline__ double finite_or_low(const SmoothTracksArgs& a, int64_t f) {
  const double v = f < a.n_frames ? a.t[f] : -__builtin_inf();
  return finite1(v) ? v : -__builtin_inf();
}

__global__ __launch_bounds__(kT) void ts_tile_max_kernel(SmoothTracksArgs a) {
  __shared__ double s[kT];
  const double m = block_prefix_max(finite_or_low(a, (int64_t)blockIdx.x * kT + threadIdx.x), s);
  if (threadIdx.x == kT - 1) a.tile_max[blockIdx.x] = m;
}

// one workgroup: tile_max[p] becomes the largest finite t of the tiles before p (-inf for none).  Lane l owns the entries
// [l * per, (l + 1) * per).
__global__ __launch_bounds__(kT) void ts_tile_scan_kernel(SmoothTracksArgs a, int64_t P) {
  __shared__ double s[kT];
  const int64_t per = (P + kT - 1) / kT, lo = threadIdx.x * per, hi = lo + per < P ? lo + per : P;
  double m = -__builtin_inf();
  for (int64_t p = lo; p < hi; p++) m = a.tile_max[p] > m ? a.tile_max[p] : m;
  block_prefix_max(m, s);
  double run = threadIdx.x > 0 ? s[threadIdx.x - 1] : -__builtin_inf();
  for (int64_t p = lo; p < hi; p++) {
    const double own = a.tile_max[p];
    a.tile_max[p] = run;
    run = own > run ? own : run;
  }
}

__global__ __launch_bounds__(kT) void ts_good_kernel(SmoothTracksArgs a) {
  __shared__ double s[kT];
  const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
  block_prefix_max(finite_or_low(a, f), s);
  if (f >= a.n_frames) return;
  const double before_tile = a.tile_max[blockIdx.x], in_tile = threadIdx.x > 0 ? s[threadIdx.x - 1] : -__builtin_inf();
  const double before = in_tile > before_tile ? in_tile : before_tile, v = a.t[f];
  a.good[f] = finite1(v) && v > before ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------ smooth
template <int D>
__global__ __launch_bounds__(kT) void ts_smooth_kernel(SmoothTracksArgs a) {
  __shared__ double s_t[kStage];
  __shared__ double s_x[3][kStage];
  __shared__ uint8_t s_ok[kStage];
  const int W = a.W, lane = threadIdx.x, r = blockIdx.y;
  const int64_t F = a.n_frames, f0 = (int64_t)blockIdx.x * kT;
  const double* row = a.traj + (size_t)r * F * 3;
  for (int i = lane; i < kT + 2 * W; i += kT) {  // staged index i = frame f0 - W + i
    const int64_t g = f0 - W + i;
    double tv = 0.0, x[3] = {0.0, 0.0, 0.0};
    int bits = 0;
    if (g >= 0 && g < F) {
      tv = a.t[g];
      x[0] = row[3 * g];
      x[1] = row[3 * g + 1];
      x[2] = row[3 * g + 2];
      if (a.good[g]) bits = finite3(x) ? kGood | kPresent : kGood;
    }
    s_t[i] = tv;
    s_x[0][i] = x[0];
    s_x[1][i] = x[1];
    s_x[2][i] = x[2];
    s_ok[i] = (uint8_t)bits;
  }
  __syncthreads();
  const int64_t f = f0 + lane;
  if (f >= F) return;

  const double nan = __builtin_nan("");
  const int c = lane + W;  // this lane's frame among the staged ones; its window is the staged frames lane .. lane + 2 W
  const double tf = s_t[c];
  int n = 0, flag = 0;
  double out[10];          // pos, vel, acc, res
#pragma unroll
  for (int i = 0; i < 10; i++) out[i] = nan;
  double h = 0.0;
  if (!(s_ok[c] & kGood)) {
    flag = kTsBadTime;
  } else {
    int ja = 0, jb = 0;    // offsets of the nearest present frames below and above, 0 = none in the window
    bool sa = false, sb = false;
    for (int j = -W; j <= W; j++) {
      if (!(s_ok[c + j] & kPresent)) continue;
      const double as = fabs(s_t[c + j] - tf);
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
    const bool present = s_ok[c] & kPresent;
    const bool fillable = !present && a.max_gap > 0 && ja != 0 && jb != 0 && jb - ja - 1 <= a.max_gap && sa && sb;
    if (!present && !fillable) {
      flag = 0;
    } else if (n < a.n_min) {
      flag = kTsFew;
    } else {
      double S[2 * D + 1], B[D + 1][3];
#pragma unroll
      for (int i = 0; i <= 2 * D; i++) S[i] = 0.0;
#pragma unroll
      for (int i = 0; i <= D; i++) B[i][0] = B[i][1] = B[i][2] = 0.0;
      for (int j = -W; j <= W; j++) {
        if (!(s_ok[c + j] & kPresent)) continue;
        const double s = s_t[c + j] - tf;
        if (!(fabs(s) <= a.span)) continue;
        const double u = s / h, x0 = s_x[0][c + j], x1 = s_x[1][c + j], x2 = s_x[2][c + j];
        double p = 1.0;
#pragma unroll
        for (int i = 0; i <= 2 * D; i++) {
          S[i] = S[i] + p;
          if (i <= D) {
            B[i][0] = B[i][0] + p * x0;
            B[i][1] = B[i][1] + p * x1;
            B[i][2] = B[i][2] + p * x2;
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
          double s = S[i + j];
#pragma unroll
          for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k];
          if (j == i) {
            if (!(s > 0.0 && s < __builtin_inf())) ok = false;
            L[i][i] = sqrt(s);
          } else {
            L[i][j] = s / L[j][j];
          }
        }
      if (!ok) {
        flag = kTsSingular;
      } else {
        flag = present ? kTsSmoothed : kTsFilled;
        double cf[D + 1][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
          double y[D + 1];
#pragma unroll
          for (int i = 0; i <= D; i++) {
            double s = B[i][k];
#pragma unroll
            for (int m = 0; m < i; m++) s = s - L[i][m] * y[m];
            y[i] = s / L[i][i];
          }
#pragma unroll
          for (int i = D; i >= 0; i--) {
            double s = y[i];
#pragma unroll
            for (int m = i + 1; m <= D; m++) s = s - L[m][i] * cf[m][k];
            cf[i][k] = s / L[i][i];
          }
        }
        double ss = 0.0;
        for (int j = -W; j <= W; j++) {
          if (!(s_ok[c + j] & kPresent)) continue;
          const double s = s_t[c + j] - tf;
          if (!(fabs(s) <= a.span)) continue;
          const double u = s / h;
#pragma unroll
          for (int k = 0; k < 3; k++) {
            double q = cf[D][k];
#pragma unroll
            for (int i = D - 1; i >= 0; i--) q = q * u + cf[i][k];
            const double e = s_x[k][c + j] - q;
            ss = ss + e * e;
          }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
          out[k] = cf[0][k];
          out[3 + k] = cf[1][k] / h;
          if constexpr (D >= 2) out[6 + k] = ((2.0 * cf[2][k]) / h) / h;
        }
        out[9] = sqrt(ss / (double)(3 * n));
      }
    }
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

hipError_t launch_good_times(const SmoothTracksArgs& a, hipStream_t stream) {
  const int64_t P = ts_tiles(a.n_frames);
  const dim3 tiles((unsigned)P), block(kT), one(1);
  hipError_t e;
  hipLaunchKernelGGL(ts_tile_max_kernel, tiles, block, 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(ts_tile_scan_kernel, one, block, 0, stream, a, P);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(ts_good_kernel, tiles, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_smooth_tracks(const SmoothTracksArgs& a, hipStream_t stream) {
  const dim3 block(kT), grid((unsigned)ts_tiles(a.n_frames), (unsigned)a.R);
  if (hipError_t e = launch_good_times(a, stream)) return e;
  if (a.degree == 1) hipLaunchKernelGGL(ts_smooth_kernel<1>, grid, block, 0, stream, a);
  else if (a.degree == 2) hipLaunchKernelGGL(ts_smooth_kernel<2>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(ts_smooth_kernel<3>, grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
