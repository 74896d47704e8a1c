// track_stitch.hip -- which rows of a gathered session are the same marker (include/mocap_core.h, "track stitching").
//   good     the good-time bits of t: track_smooth.hip's three launches, reused.
//   extents  ext [R][3] = (first present frame, last present frame, number present).  One lane seeds the row's entry; then one
//            workgroup of 256 lanes per (256-frame tile, row), grid ceil(F / 256) x R, reads its samples once (neighbouring lanes,
//            neighbouring 24-byte samples), each wave takes first / last / count from one ballot, lane 0 folds the four waves through
//            LDS and combines the tile into ext with 32-bit integer atomicMin / atomicMax / atomicAdd: exact in any order.
//   models   one wave per (row, end), grid R x 2: the at most 65 frames of the fit window are staged in LDS, then lane 0 walks them
//            in ascending frame order -- the contract's order of every sum -- and writes pos, vel and the end frame's time.  The tail's
//            wave also turns the seed of an empty row into (-1, -1, 0).
//   costs    one lane per (p, q), a workgroup of 64 q x 4 p, grid ceil(R / 64) x ceil(R / 4); the 4 tail and 64 head models of the
//            tile are staged in LDS; the lane writes c, or +inf for a pair that is not admissible, into table [R][R].
//   assoc    one workgroup of up to 1024 lanes (R rounded up to whole waves).  Rounds of mutually best pairs under the order
//            (c, p, q): every row keeps its best free successor and its best free predecessor; a row is scanned again only when that
//            partner was taken.  A scan is one wave's: 64 lanes stride over the row (or column) of the table and fold (c, index) by
//            six shuffles.  The loop ends with the first round that commits nothing (at most R - 1 rounds commit).  Then chain by
//            pointer jumping (10 rounds cover 1024 rows), row_of and n_chains by a prefix sum over the head flags.
// FP64 throughout, nothing fused (-ffp-contract=off is the build's rule), / correctly rounded, no sqrt, no floating-point atomics:
// the outputs are a function of the inputs alone, and equal to the scalar statement of the contract bit for bit.
#include "track_stitch.hpp"
#include "mocap_device.hpp"

namespace mocap {

namespace {

constexpr int kT = kTsTile;
constexpr int kWin = kStMaxFit + 1;  // frames of the widest fit window
constexpr int kCostQ = 64, kCostP = 4;
constexpr int kMaxLanes = kTsMaxRows;
constexpr int kJumpRounds = 10;      // 2^10 >= kTsMaxRows
static_assert((1 << kJumpRounds) >= kTsMaxRows, "pointer jumping must reach the head of the longest chain");

// ------------------------------------------------------------------------------------------------------------------ extents
__global__ __launch_bounds__(kT) void st_extent_seed_kernel(StitchTracksArgs a) {
  const int r = blockIdx.x * kT + threadIdx.x;
  if (r >= a.R) return;
  a.ext[3 * r] = 0x7fffffff;
  a.ext[3 * r + 1] = -1;
  a.ext[3 * r + 2] = 0;
}

__global__ __launch_bounds__(kT) void st_extent_kernel(StitchTracksArgs a) {
  __shared__ int s_lo[kT / 64], s_hi[kT / 64], s_n[kT / 64];
  const int lane = threadIdx.x, r = blockIdx.y;
  const int64_t f0 = (int64_t)blockIdx.x * kT, f = f0 + lane;
  bool present = false;
  if (f < a.n_frames && a.good[f]) present = finiteN<3>(a.traj + ((size_t)r * a.n_frames + f) * 3);
  const unsigned long long m = __ballot(present);
  if ((lane & 63) == 0) {
    const int w = lane >> 6;
    s_lo[w] = m ? w * 64 + __builtin_ctzll(m) : kT;
    s_hi[w] = m ? w * 64 + 63 - __builtin_clzll(m) : -1;
    s_n[w] = __builtin_popcountll(m);
  }
  __syncthreads();
  if (lane != 0) return;
  int lo = kT, hi = -1, n = 0;
#pragma unroll
  for (int w = 0; w < kT / 64; w++) {
    lo = s_lo[w] < lo ? s_lo[w] : lo;
    hi = s_hi[w] > hi ? s_hi[w] : hi;
    n += s_n[w];
  }
  if (n == 0) return;
  atomicMin(a.ext + 3 * r, (int)(f0 + lo));
  atomicMax(a.ext + 3 * r + 1, (int)(f0 + hi));
  atomicAdd(a.ext + 3 * r + 2, n);
}

// ------------------------------------------------------------------------------------------------------------------ end models
__global__ __launch_bounds__(64) void st_model_kernel(StitchTracksArgs a) {
  __shared__ double s_s[kWin];
  __shared__ double s_x[3][kWin];
  __shared__ uint8_t s_ok[kWin];
  const int lane = threadIdx.x, r = blockIdx.x, head = blockIdx.y;
  const int64_t F = a.n_frames;
  const int n = a.ext[3 * r + 2];
  double* out = a.model + ((size_t)r * 2 + head) * kStModel;
  if (n == 0) {  // an empty row: no model is ever read; the extent takes its final form
    if (lane < kStModel) out[lane] = __builtin_nan("");
    if (lane == 0 && !head) a.ext[3 * r] = -1;
    return;
  }
  const int64_t e = head ? a.ext[3 * r] : a.ext[3 * r + 1];  // the end frame: present, so inside 0 .. F-1
  const int64_t lo = head ? e : (e - a.fit_frames > 0 ? e - a.fit_frames : 0);
  const int64_t hi = head ? (e + a.fit_frames < F - 1 ? e + a.fit_frames : F - 1) : e;
  const int cnt = (int)(hi - lo + 1);  // 1 .. fit_frames + 1
  const double te = a.t[e];
  const double* row = a.traj + (size_t)r * F * 3;
  for (int i = lane; i < cnt; i += 64) {
    const int64_t g = lo + i;
    const double x[3] = {row[3 * g], row[3 * g + 1], row[3 * g + 2]};
    s_s[i] = a.t[g] - te;
    s_x[0][i] = x[0];
    s_x[1][i] = x[1];
    s_x[2][i] = x[2];
    s_ok[i] = a.good[g] && finiteN<3>(x);
  }
  __syncthreads();
  if (lane != 0) return;
  int m = 0;
  double h = 0.0;
  for (int i = 0; i < cnt; i++) {
    if (!s_ok[i]) continue;
    const double as = fabs(s_s[i]);
    m++;
    h = as > h ? as : h;
  }
  const int ie = (int)(e - lo);
  double pos[3] = {s_x[0][ie], s_x[1][ie], s_x[2][ie]}, vel[3] = {0.0, 0.0, 0.0};
  if (m >= 2) {
    double S0 = 0.0, S1 = 0.0, S2 = 0.0, B0[3] = {0.0, 0.0, 0.0}, B1[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < cnt; i++) {
      if (!s_ok[i]) continue;
      const double u = s_s[i] / h;
      S0 = S0 + 1.0;
      S1 = S1 + u;
      S2 = S2 + u * u;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        B0[k] = B0[k] + s_x[k][i];
        B1[k] = B1[k] + u * s_x[k][i];
      }
    }
    const double det = S0 * S2 - S1 * S1;
    if (det > 0.0 && det < __builtin_inf()) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        pos[k] = (S2 * B0[k] - S1 * B1[k]) / det;
        vel[k] = ((S0 * B1[k] - S1 * B0[k]) / det) / h;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    out[k] = pos[k];
    out[3 + k] = vel[k];
  }
  out[6] = te;
}

// ------------------------------------------------------------------------------------------------------------------ pair costs
__global__ __launch_bounds__(kCostQ* kCostP) void st_cost_kernel(StitchTracksArgs a) {
  __shared__ double s_tail[kCostP][kStModel], s_head[kCostQ][kStModel];
  __shared__ int s_b[kCostP], s_a[kCostQ];  // the last frame of p, the first frame of q; -1 = the row is empty or beyond R
  const int lx = threadIdx.x, ly = threadIdx.y, l = ly * kCostQ + lx;
  const int q0 = blockIdx.x * kCostQ, p0 = blockIdx.y * kCostP;
  for (int i = l; i < (kCostP + kCostQ) * kStModel; i += kCostQ * kCostP) {
    const bool tail = i < kCostP * kStModel;
    const int j = tail ? i : i - kCostP * kStModel, row = (tail ? p0 : q0) + j / kStModel;
    const double v = row < a.R ? a.model[((size_t)row * 2 + (tail ? 0 : 1)) * kStModel + j % kStModel] : 0.0;
    if (tail) s_tail[j / kStModel][j % kStModel] = v;
    else s_head[j / kStModel][j % kStModel] = v;
  }
  if (l < kCostP) s_b[l] = p0 + l < a.R && a.ext[3 * (p0 + l) + 2] != 0 ? a.ext[3 * (p0 + l) + 1] : -1;
  if (l >= kCostQ && l < 2 * kCostQ) {
    const int q = q0 + l - kCostQ;
    s_a[l - kCostQ] = q < a.R && a.ext[3 * q + 2] != 0 ? a.ext[3 * q] : -1;
  }
  __syncthreads();
  const int p = p0 + ly, q = q0 + lx;
  if (p >= a.R || q >= a.R) return;
  double c = __builtin_inf();
  const int bp = s_b[ly], aq = s_a[lx];
  if (p != q && bp >= 0 && aq >= 0 && bp < aq) {
    const double* T = s_tail[ly];
    const double* H = s_head[lx];
    const double dt = H[6] - T[6];
    const double g = a.gate + a.gate_rate * dt, g2 = g * g;
    double d[3], e[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      d[k] = H[k] - (T[k] + T[3 + k] * dt);
      e[k] = T[k] - (H[k] - H[3 + k] * dt);
    }
    const double d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    const double cc = 0.5 * (d2 + e2);
    if (dt <= a.max_dt && cc < g2) c = cc;
  }
  a.table[(size_t)p * a.R + q] = c;
}

// ------------------------------------------------------------------------------------------------------------------ association
// The smallest (c, j) over the free entries j of one row (stride 1) or column (stride R) of the table, c < +inf; every lane of the
// wave calls it and gets the result: j = -1 for none.
__device__ __forceinline__ int wave_best(const double* line, size_t stride, int R, const int* taken, double* c_out) {
  double c = __builtin_inf();
  int j = -1;
  for (int i = threadIdx.x & 63; i < R; i += 64) {
    const double v = line[(size_t)i * stride];
    if (v < c && taken[i] < 0) {  // strict: the lowest index of equal costs stays
      c = v;
      j = i;
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double oc = __shfl_xor(c, d, 64);
    const int oj = __shfl_xor(j, d, 64);
    if (oj >= 0 && (j < 0 || oc < c || (oc == c && oj < j))) {
      c = oc;
      j = oj;
    }
  }
  *c_out = c;
  return j;
}

__global__ __launch_bounds__(kMaxLanes) void st_assoc_kernel(StitchTracksArgs a) {
  __shared__ int s_next[kMaxLanes], s_prev[kMaxLanes];    // -1 = free
  __shared__ int s_succ[kMaxLanes], s_pred[kMaxLanes];    // a row's best free successor / predecessor; -1 = none; -2 = scan it
  __shared__ double s_succ_c[kMaxLanes];
  __shared__ int s_scan[kMaxLanes];
  const int R = a.R, lane = threadIdx.x, wave = lane >> 6, n_waves = blockDim.x >> 6;
  const bool mine = lane < R;
  double link_cost = __builtin_nan("");
  if (mine) {
    s_next[lane] = -1;
    s_prev[lane] = -1;
    s_succ[lane] = -2;
    s_pred[lane] = -2;
  }
  __syncthreads();
  for (;;) {
    // 1. the rows whose partner was taken (or that have none yet) look again, a wave per row
    for (int r = wave; r < R; r += n_waves) {
      if (s_succ[r] == -2) {
        double c;
        const int j = wave_best(a.table + (size_t)r * R, 1, R, s_prev, &c);
        if ((lane & 63) == 0) {
          s_succ[r] = j;
          s_succ_c[r] = c;
        }
      }
      if (s_pred[r] == -2) {
        double c;
        const int j = wave_best(a.table + r, (size_t)R, R, s_next, &c);
        if ((lane & 63) == 0) s_pred[r] = j;
      }
    }
    __syncthreads();
    // 2. mutually best pairs commit
    int q = -1;
    if (mine && s_next[lane] < 0) {
      q = s_succ[lane];
      if (q >= 0 && s_pred[q] != lane) q = -1;
    }
    const int any = __syncthreads_or(q >= 0);
    if (!any) break;
    if (q >= 0) {
      s_next[lane] = q;
      s_prev[q] = lane;
      link_cost = s_succ_c[lane];
    }
    __syncthreads();
    // 3. whoever lost its partner scans again
    if (mine) {
      if (s_next[lane] < 0 && s_succ[lane] >= 0 && s_prev[s_succ[lane]] >= 0) s_succ[lane] = -2;
      if (s_prev[lane] < 0 && s_pred[lane] >= 0 && s_next[s_pred[lane]] >= 0) s_pred[lane] = -2;
    }
    __syncthreads();
  }
  // chains: pointer jumping towards the head; s_succ and s_pred are free now and hold the two generations
  int* cur = s_succ;
  int* nxt = s_pred;
  if (mine) cur[lane] = s_prev[lane] < 0 ? lane : s_prev[lane];
  __syncthreads();
  for (int it = 0; it < kJumpRounds; it++) {
    if (mine) nxt[lane] = cur[cur[lane]];
    __syncthreads();
    int* t = cur;
    cur = nxt;
    nxt = t;
  }
  // row_of: an inclusive prefix sum over "non-empty head" (Hillis-Steele)
  const int head = mine ? cur[lane] : 0;
  const bool filled = mine && a.ext[3 * lane + 2] != 0;
  int v = filled && head == lane ? 1 : 0;
  s_scan[lane] = v;
  __syncthreads();
  for (int d = 1; d < (int)blockDim.x; d <<= 1) {
    const int o = lane >= d ? s_scan[lane - d] : 0;
    __syncthreads();
    v += o;
    s_scan[lane] = v;
    __syncthreads();
  }
  if (mine) {
    a.next[lane] = s_next[lane];
    a.prev[lane] = s_prev[lane];
    a.cost[lane] = link_cost;
    a.chain[lane] = head;
    a.row_of[lane] = filled ? s_scan[head] - 1 : -1;
  }
  if (lane == (int)blockDim.x - 1) *a.n_chains = v;
}

}  // namespace

hipError_t launch_stitch_tracks(const StitchTracksArgs& a, hipStream_t stream) {
  const GoodTimesArgs g{a.n_frames, a.t, a.tile_max, a.good};
  hipError_t e;
  if ((e = launch_good_times(g, stream)) != hipSuccess) return e;
  const unsigned R = (unsigned)a.R;
  hipLaunchKernelGGL(st_extent_seed_kernel, dim3((R + kT - 1) / kT), dim3(kT), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(st_extent_kernel, dim3((unsigned)ts_tiles(a.n_frames), R), dim3(kT), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(st_model_kernel, dim3(R, 2), dim3(64), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(st_cost_kernel, dim3((R + kCostQ - 1) / kCostQ, (R + kCostP - 1) / kCostP), dim3(kCostQ, kCostP), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(st_assoc_kernel, dim3(1), dim3((R + 63) / 64 * 64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
