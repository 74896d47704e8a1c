// resect.hip -- the kernels of the "camera resection" section of include/mocap_core.h: one camera's pose from 3-D points and where it
// saw them.  The arithmetic is csrc/resect_math.hpp, the same text the host check runs.
//   compact      the rows without a NaN or an infinity, in input order, as [n][5] = (X, u, v): count, scan, scatter
//   hypotheses   one lane per hypothesis: counter-based sample, Grunert's three-point solver -> up to four poses
//   score        one candidate pose per lane (12 doubles and K in registers); the rows go through LDS in tiles of 256 and every lane
//                reads the same LDS address (a broadcast: no bank conflict); grid = candidate tiles x point slices; a lane's integer
//                count is added to counts[h][s] (integer sums: the order cannot change them); lanes of absent solutions skip the walk
//   winner       one workgroup: most inliers, ties to the lower (hypothesis, solution); its pose into slot 0 -- the first linearisation
//                follows on the stream, the host has not seen anything yet
//   normal_eq    one lane per valid row: H, g, cost over the inliers of the mask (without a base: of the pose itself) and, for a
//                trial, the cost's change against its base from the increment, through the project's one tree
//                (csrc/tree_fold.hpp), then one wave folds the slab into the pinned record
//   finish       one lane per valid row: the final mask and the costs at the final, the winner's and the prior pose over it
// FP64 throughout, nothing fused, no floating-point atomics: every output is a function of the inputs alone.
#include "resect.hpp"

#include "mocap_device.hpp"
#include "tree_fold.hpp"

namespace mocap {

namespace {

constexpr int kT = kCalibThreads;
constexpr int kScanThreads = 512;
static_assert(kRsMaxPoints / kCalibThreads <= kScanThreads, "one workgroup scans the per-workgroup counts");

__device__ __forceinline__ bool rs_row_valid(const RsArgs& a, int64_t i) {
  const double* x = a.X + 3 * i;
  const double* o = a.obs + 2 * i;
  return rs_finite(x[0]) && rs_finite(x[1]) && rs_finite(x[2]) && rs_finite(o[0]) && rs_finite(o[1]);
}

// ----------------------------------------------------------------------------------------------------------------- compact
// three launches, 256 rows per workgroup: valid rows per workgroup (ballots), one workgroup scans those counts in place (at most
// kScanThreads of them: kRsMaxPoints / 256), then every workgroup writes its valid rows behind its offset, in input order
__global__ __launch_bounds__(kT) void resect_count_kernel(RsArgs a) {
  __shared__ int s_cnt[kFoldWaves];
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  const bool valid = i < a.N && rs_row_valid(a, i);
  const unsigned long long b = __ballot(valid);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int w = 0; w < kFoldWaves; w++) c += s_cnt[w];
    a.blk[blockIdx.x] = c;  // blockIdx.x < calib_partials(N) <= kScanThreads
  }
}

__global__ __launch_bounds__(kScanThreads) void resect_scan_kernel(RsArgs a, int P) {
  __shared__ int s_scan[kScanThreads];
  const int tid = threadIdx.x;
  const int v = tid < P ? a.blk[tid] : 0;
  s_scan[tid] = v;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {
    const int o = tid >= off ? s_scan[tid - off] : 0;
    __syncthreads();
    s_scan[tid] += o;
    __syncthreads();
  }
  if (tid < P) a.blk[tid] = s_scan[tid] - v;  // counts -> offsets
  if (tid == kScanThreads - 1) a.hdr[0] = s_scan[tid];
}

__global__ __launch_bounds__(kT) void resect_compact_kernel(RsArgs a) {
  __shared__ int s_cnt[kFoldWaves];
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  const bool valid = i < a.N && rs_row_valid(a, i);
  const unsigned long long b = __ballot(valid);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_cnt[wave] = __popcll(b);
  __syncthreads();
  int pos = a.blk[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; w++) pos += s_cnt[w];
  if (!valid) return;
  double* r = a.rows + 5 * (size_t)pos;  // pos < valid rows <= N: inside rows [N][5] and orig [N]
  r[0] = a.X[3 * i];
  r[1] = a.X[3 * i + 1];
  r[2] = a.X[3 * i + 2];
  r[3] = a.obs[2 * i];
  r[4] = a.obs[2 * i + 1];
  a.orig[pos] = (int32_t)i;
}

// -------------------------------------------------------------------------------------------------------------- hypotheses
__global__ __launch_bounds__(64) void resect_hypotheses_kernel(RsArgs a) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= a.H) return;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int n = a.hdr[0];
  double* out = a.poses + 48 * (size_t)h;
  int ns = 0, idx[3] = {-1, -1, -1};
#pragma unroll
  for (int s = 0; s < 4; s++) a.counts[4 * h + s] = 0;
  if (h == 0 && a.has_prior) {
    for (int k = 0; k < 12; k++) out[k] = a.pose[12 * kRsSlotPrior + k];
    ns = 1;
  } else if (n >= 4) {
    int pick[3];
    rs_sample(a.seed, (uint32_t)h, (uint32_t)n, pick);
    double P[3][3], uv[3][2];
    for (int k = 0; k < 3; k++) {
      const double* r = a.rows + 5 * (size_t)pick[k];  // pick[k] < n <= N
      P[k][0] = r[0];
      P[k][1] = r[1];
      P[k][2] = r[2];
      uv[k][0] = r[3];
      uv[k][1] = r[4];
      idx[k] = a.orig[pick[k]];
    }
    ns = rs_p3p(P, uv, a.k4, out);
  }
  for (int k = 12 * ns; k < 48; k++) out[k] = qnan;
  a.n_sol[h] = ns;
  a.samp[3 * h] = idx[0];
  a.samp[3 * h + 1] = idx[1];
  a.samp[3 * h + 2] = idx[2];
}

// ------------------------------------------------------------------------------------------------------------------- score
__global__ __launch_bounds__(kRsCandTile) void resect_score_kernel(RsArgs a) {
  __shared__ double s_rows[kRsTile * 5];
  const int n = a.hdr[0];
  const int lo = blockIdx.y * kRsSlice;
  if (lo >= n) return;  // the whole workgroup
  const int hi = lo + kRsSlice < n ? lo + kRsSlice : n;
  const int cand = blockIdx.x * kRsCandTile + threadIdx.x, h = cand >> 2, s = cand & 3;
  const bool active = h < a.H && s < a.n_sol[h];
  double p[12];
#pragma unroll
  for (int k = 0; k < 12; k++) p[k] = active ? a.poses[12 * (size_t)cand + k] : 0.0;
  const double k4[4] = {a.k4[0], a.k4[1], a.k4[2], a.k4[3]};
  const double thr2 = a.thr2;
  int count = 0;
  for (int base = lo; base < hi; base += kRsTile) {
    const int m = hi - base < kRsTile ? hi - base : kRsTile;
    const double* src = a.rows + 5 * (size_t)base;
    for (int e = threadIdx.x; e < 5 * m; e += kRsCandTile) s_rows[e] = src[e];  // base + m <= n: inside rows
    __syncthreads();
    if (active) {
      for (int i = 0; i < m; i++) {
        RsView w;
        rs_view(p, k4, s_rows[5 * i], s_rows[5 * i + 1], s_rows[5 * i + 2], s_rows[5 * i + 3], s_rows[5 * i + 4], w);
        count += rs_inlier(w, thr2) ? 1 : 0;
      }
    }
    __syncthreads();
  }
  if (active && count) atomicAdd(a.counts + cand, count);
}

// ------------------------------------------------------------------------------------------------------------------ winner
__global__ __launch_bounds__(256) void resect_winner_kernel(RsArgs a) {
  __shared__ unsigned long long s_key[256];
  __shared__ int s_nosol[256];
  const int tid = threadIdx.x;
  unsigned long long key = 0;  // (count, ~index): the maximum is the most inliers, then the lowest candidate index
  int nosol = 0;
  for (int c = tid; c < 4 * a.H; c += 256) {
    const int h = c >> 2, s = c & 3, ns = a.n_sol[h];
    if (s < ns) {
      const unsigned long long k = ((unsigned long long)(uint32_t)a.counts[c] << 32) | (unsigned long long)(0xffffffffu - (uint32_t)c);
      key = k > key ? k : key;
    }
    nosol += (s == 0 && ns == 0) ? 1 : 0;
  }
  s_key[tid] = key;
  s_nosol[tid] = nosol;
  __syncthreads();
  if (tid != 0) return;
  for (int l = 1; l < 256; l++) {
    key = s_key[l] > key ? s_key[l] : key;
    nosol += s_nosol[l];
  }
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int n = a.hdr[0];
  const bool any = key != 0;
  const int cand = any ? (int)(0xffffffffu - (uint32_t)(key & 0xffffffffull)) : -1;
  const int cnt = any ? (int)(key >> 32) : 0;
  const int status = n < 4 ? kRsTooFew : (!any || cnt < a.min_inliers) ? kRsNoModel : kRsOk;
  a.state[0] = (double)n;
  a.state[1] = (double)cnt;
  a.state[2] = any ? (double)(cand >> 2) : -1.0;
  a.state[3] = any ? (double)(cand & 3) : -1.0;
  a.state[4] = (double)nosol;
  a.state[5] = (double)status;
  for (int k = 0; k < 12; k++) {
    const double v = status == kRsOk ? a.poses[12 * (size_t)cand + k] : a.has_prior ? a.pose[12 * kRsSlotPrior + k] : qnan;
    a.pose[12 * kRsSlotCur + k] = v;
    a.pose[12 * kRsSlotWinner + k] = v;
  }
}

// --------------------------------------------------------------------------------------------------------------- normal_eq
__global__ __launch_bounds__(kT) void resect_normal_eq_kernel(RsArgs a, int with_base) {
  __shared__ double s_part[kFoldWaves][kRsSums];
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int n = a.hdr[0];
  double v[kRsSums];
#pragma unroll
  for (int k = 0; k < kRsSums; k++) v[k] = 0.0;
  if (i < n) {
    const double* r = a.rows + 5 * i;
    const ctab_t pose = as_ctab(a.pose + 12 * kRsSlotCur);
    RsView w;
    rs_view(pose, a.k4, r[0], r[1], r[2], r[3], r[4], w);
    bool in;
    if (!with_base) {
      in = rs_inlier(w, a.thr2);
      a.mask[i] = in ? 1 : 0;
    } else {
      in = a.mask[i] != 0;
    }
    if (in) {
      rs_row(w, a.k4, v);
      if (with_base) {
        RsView b;
        rs_view(as_ctab(a.pose + 12 * kRsSlotBase), a.k4, r[0], r[1], r[2], r[3], r[4], b);
        v[kRsDelta] = rs_delta_row(b, as_ctab(a.pose + 12 * kRsSlotInc), a.k4);
      }
    }
  }
  block_fold<kRsSums, -1>(v, s_part, a.slab + (size_t)blockIdx.x * kRsSums);
}

__global__ __launch_bounds__(64) void resect_fold_kernel(RsArgs a, int64_t P) {
  double v[kRsSums];
  slab_fold<kRsSums, -1>(a.slab, P, 0.0, v);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < kRsSums; k++) a.rec[k] = v[k];
  for (int k = 0; k < 12; k++) a.rec[kRsRecPose + k] = a.pose[12 * kRsSlotCur + k];
  for (int k = 0; k < 6; k++) a.rec[kRsRecState + k] = a.state[k];
}

// ------------------------------------------------------------------------------------------------------------------ finish
__global__ __launch_bounds__(kT) void resect_finish_kernel(RsArgs a) {
  __shared__ double s_part[kFoldWaves][4];
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int n = a.hdr[0];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < n) {
    const double* r = a.rows + 5 * i;
    RsView w;
    rs_view(as_ctab(a.pose + 12 * kRsSlotCur), a.k4, r[0], r[1], r[2], r[3], r[4], w);
    const bool in = rs_inlier(w, a.thr2);
    a.mask_out[a.orig[i]] = in ? 1 : 0;  // orig[i] < N
    if (in) {
      v[0] = 1.0;
      v[1] = w.s2;
      rs_view(as_ctab(a.pose + 12 * kRsSlotWinner), a.k4, r[0], r[1], r[2], r[3], r[4], w);
      v[2] = w.s2;
      if (a.has_prior) {
        rs_view(as_ctab(a.pose + 12 * kRsSlotPrior), a.k4, r[0], r[1], r[2], r[3], r[4], w);
        v[3] = w.s2;
      }
    }
  }
  block_fold<4, -1>(v, s_part, a.slab + (size_t)blockIdx.x * 4);
}

__global__ __launch_bounds__(64) void resect_finish_fold_kernel(RsArgs a, int64_t P) {
  double v[4];
  slab_fold<4, -1>(a.slab, P, 0.0, v);
  if (threadIdx.x != 0) return;
  for (int k = 0; k < 4; k++) a.rec[kRsRecFinish + k] = v[k];
  for (int k = 0; k < 12; k++) a.rec[kRsRecPose + k] = a.pose[12 * kRsSlotCur + k];
  for (int k = 0; k < 6; k++) a.rec[kRsRecState + k] = a.state[k];
}

}  // namespace

hipError_t launch_resect_search(const RsArgs& a, hipStream_t stream) {
  hipError_t e;
  const int P = (int)calib_partials(a.N);
  hipLaunchKernelGGL(resect_count_kernel, dim3((unsigned)P), dim3(kT), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(resect_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, a, P);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(resect_compact_kernel, dim3((unsigned)P), dim3(kT), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(resect_hypotheses_kernel, dim3((unsigned)((a.H + 63) / 64)), dim3(64), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const unsigned tiles = (unsigned)((4 * a.H + kRsCandTile - 1) / kRsCandTile), slices = (unsigned)((a.N + kRsSlice - 1) / kRsSlice);
  hipLaunchKernelGGL(resect_score_kernel, dim3(tiles, slices), dim3(kRsCandTile), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(resect_winner_kernel, dim3(1), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_resect_normal_eq(const RsArgs& a, int with_base, hipStream_t stream) {
  const int64_t P = calib_partials(a.N);
  hipLaunchKernelGGL(resect_normal_eq_kernel, dim3((unsigned)P), dim3(kT), 0, stream, a, with_base);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(resect_fold_kernel, dim3(1), dim3(64), 0, stream, a, P);
  return hipGetLastError();
}

hipError_t launch_resect_finish(const RsArgs& a, hipStream_t stream) {
  const int64_t P = calib_partials(a.N);
  hipLaunchKernelGGL(resect_finish_kernel, dim3((unsigned)P), dim3(kT), 0, stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(resect_finish_fold_kernel, dim3(1), dim3(64), 0, stream, a, P);
  return hipGetLastError();
}

}  // namespace mocap
