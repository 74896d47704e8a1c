// rigid_groups.hip -- which rows of a gathered session keep their mutual distances (include/mocap_core.h, "rigid groups").
//   bounds   one lane seeds a row's six keys; then one workgroup of 256 lanes per (256-frame tile, row), grid ceil(F / 256) x R, reads
//            its samples once (neighbouring lanes, neighbouring 24-byte samples), each wave folds min and max per axis by shuffles and
//            its lane 0 combines them into bounds [R][6] with 64-bit INTEGER atomicMin / atomicMax on an order-preserving key of the
//            double: exact in any order.
//   pairs    lanes are frames: one workgroup of 256 lanes per (256-frame tile, block pair), a block pair = 8 rows p x 8 rows q with
//            block(p) <= block(q).  A lane holds its frame's sample of the 8 q rows in registers, takes the p rows in turn and forms
//            the 64 values D (pass 0) or (D - dist)^2 (pass 1), +0.0 where a row is absent.  Each wave folds its 64 values over its
//            64 lanes TRANSPOSED: at offset 32 the lower lanes keep values 0 .. 31 and the upper ones 32 .. 63, each sends the other
//            half, and so on down to offset 1 -- 63 exchanges instead of 384, and lane l ends with the wave sum of value l in the
//            association order of tree_fold.hpp's wave_fold (v[l] + v[l + off], off = 32 .. 1; IEEE + commutes).  The counts come
//            from the lanes' presence bits, staged in LDS: lane l counts pair l over its wave's 64 frames.  Wave 0 then adds the four wave sums in wave order (block_fold's order) and writes one slab
//            entry per (tile, pair): slab [slot][tile].
//   fold     one wave per pair: tree_fold.hpp's slab_fold over the pair's P tile sums; pass 0 writes cnt and dist, pass 1 spread,
//            both [p][q] and [q][p] from the one value computed with p <= q.
//   groups   one workgroup of 256 lanes, a row per lane: travel from the bounds, eligibility, the edge matrix as 256 x 256 bits in
//            LDS (8 KB), min-label propagation with pointer jumping until a round changes nothing, the groups numbered by a prefix
//            sum over "lowest row of a component with an edge", the per-group figures by a second walk over the bit rows (32-bit
//            integer LDS atomics; the largest spread as the integer maximum of the bits of non-negative doubles).
// FP64 throughout, nothing fused (-ffp-contract=off is the build's rule), / and sqrt correctly rounded, no floating-point atomics:
// the outputs are a function of the input alone, and equal to the scalar statement of the contract bit for bit.
#include "rigid_groups.hpp"

#include "mocap_device.hpp"
#include "track_smooth.hpp"
#include "tree_fold.hpp"

namespace mocap {

namespace {

constexpr int kT = kRgTile, kB = kRgBlock, kS = kRgSlots;
constexpr int kWords = kRgMaxRows / 32;  // words of a row of the edge matrix
constexpr int kJumps = 8;                // 2^8 >= kRgMaxRows
static_assert(kT == kCalibThreads && kS == 64 && (1 << kJumps) >= kRgMaxRows, "the tile is tree_fold.hpp's, a block pair is one wave wide");

// an unsigned key that orders like the double (finite values only reach it)
__device__ __forceinline__ unsigned long long key_of(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return b >> 63 ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double value_of(unsigned long long k) {
  return __longlong_as_double((long long)(k >> 63 ? k & 0x7fffffffffffffffull : ~k));
}

// the k-th block pair (bp, bq), bp <= bq, counted row by row of the upper triangle of nb x nb blocks
__device__ __forceinline__ void block_pair(int k, int nb, int* bp, int* bq) {
  int p = 0;
  while (k >= nb - p) {
    k -= nb - p;
    p++;
  }
  *bp = p;
  *bq = p + k;
}

// ------------------------------------------------------------------------------------------------------------------ bounds
__global__ __launch_bounds__(kT) void rg_bounds_seed_kernel(RigidGroupsArgs a) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= a.R * 6) return;
  a.bounds[i] = i % 6 < 3 ? ~0ull : 0ull;
}

__global__ __launch_bounds__(kT) void rg_bounds_kernel(RigidGroupsArgs a) {
  const int r = blockIdx.y;
  const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
  unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
  if (f < a.n_frames) {
    const double* s = a.traj + ((size_t)r * a.n_frames + f) * 3;
    const double x[3] = {s[0], s[1], s[2]};
    if (finite1(x[0]) && finite1(x[1]) && finite1(x[2])) {
#pragma unroll
      for (int k = 0; k < 3; k++) lo[k] = hi[k] = key_of(x[k]);
    }
  }
  for (int off = 32; off; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const unsigned long long ol = __shfl_xor(lo[k], off, 64), oh = __shfl_xor(hi[k], off, 64);
      lo[k] = ol < lo[k] ? ol : lo[k];
      hi[k] = oh > hi[k] ? oh : hi[k];
    }
  }
  if ((threadIdx.x & 63) != 0 || hi[0] == 0ull) return;  // (no finite value has the key 0)
#pragma unroll
  for (int k = 0; k < 3; k++) {
    atomicMin(a.bounds + 6 * r + k, lo[k]);
    atomicMax(a.bounds + 6 * r + 3 + k, hi[k]);
  }
}

// ------------------------------------------------------------------------------------------------------------------ pairs
template <int PASS>
__global__ __launch_bounds__(kT) void rg_pair_kernel(RigidGroupsArgs a, int k0) {
  __shared__ double s_sum[kFoldWaves][kS];
  __shared__ int s_cnt[kFoldWaves][kS];
  __shared__ unsigned s_mask[kT];  // pass 0: a lane's presence bits, bit j = row q0 + j, bit 8 + i = row p0 + i
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, R = a.R;
  const int64_t F = a.n_frames, P = rg_tiles(F), f = (int64_t)blockIdx.x * kT + threadIdx.x;
  int bp, bq;
  block_pair(k0 + blockIdx.y, rg_blocks(R), &bp, &bq);
  const int p0 = bp * kB, q0 = bq * kB;
  // presence as lane masks in VGPRs (all ones or zero), not as 64 wave masks in SGPRs: the value is ANDed, not selected
  double xq[kB][3];
  int okq[kB];
  unsigned mask = 0;
#pragma unroll
  for (int j = 0; j < kB; j++) {
    okq[j] = 0;
    xq[j][0] = xq[j][1] = xq[j][2] = 0.0;
    if (q0 + j < R && f < F) {
      const double* s = a.traj + ((size_t)(q0 + j) * F + f) * 3;
      xq[j][0] = s[0];
      xq[j][1] = s[1];
      xq[j][2] = s[2];
      okq[j] = finite1(xq[j][0]) && finite1(xq[j][1]) && finite1(xq[j][2]) ? -1 : 0;
      mask |= (unsigned)okq[j] & 1u << j;
    }
  }
  if (PASS == 1) {  // the block's 64 means through LDS: every lane reads them as it goes (64 uniform doubles do not fit the SGPRs)
    if (threadIdx.x < kS) {
      const int p = p0 + threadIdx.x / kB, q = q0 + threadIdx.x % kB;
      s_sum[0][threadIdx.x] = p < R && q < R ? a.dist[(size_t)p * R + q] : 0.0;  // (a pair beyond R is never present)
    }
    block_sync_lds();
  }
  double v[kS];
#pragma unroll
  for (int i = 0; i < kB; i++) {
    int okp = 0;
    double xp[3] = {0.0, 0.0, 0.0};
    if (p0 + i < R && f < F) {
      const double* s = a.traj + ((size_t)(p0 + i) * F + f) * 3;
      xp[0] = s[0];
      xp[1] = s[1];
      xp[2] = s[2];
      okp = finite1(xp[0]) && finite1(xp[1]) && finite1(xp[2]) ? -1 : 0;
      mask |= (unsigned)okp & 1u << (kB + i);
    }
#pragma unroll
    for (int j = 0; j < kB; j++) {
      const int both = okp & okq[j];
      const double dx = xp[0] - xq[j][0], dy = xp[1] - xq[j][1], dz = xp[2] - xq[j][2];
      double d = sqrt((dx * dx + dy * dy) + dz * dz);
      if (PASS == 1) {
        const double e = d - s_sum[0][i * kB + j];
        d = e * e;
      }
      const unsigned long long keep = (unsigned long long)(unsigned)both << 32 | (unsigned)both;
      v[i * kB + j] = __longlong_as_double((long long)((unsigned long long)__double_as_longlong(d) & keep));  // absent: +0.0
    }
  }
  if (PASS == 1) block_sync_lds();  // the means are read: s_sum is free for the wave sums
  // the counts: lane l answers for pair l of the block and walks the presence bits of its wave's 64 frames (the wave reads one
  // address at a time: an LDS broadcast) -- exact, and no wave mask has to live in an SGPR
  int n = 0;
  if (PASS == 0) {
    s_mask[threadIdx.x] = mask;
    block_sync_lds();
    const int at_p = kB + lane / kB, at_q = lane % kB;
#pragma unroll 8
    for (int k = 0; k < 64; k++) {
      const unsigned m = s_mask[wave * 64 + k];
      n += (int)(m >> at_p & m >> at_q & 1u);
    }
  }
  // the transposed wave fold: after the step at `half`, slot i of a lane holds value i + (lane & ~(half - 1) & 63)
#pragma unroll
  for (int half = 32; half >= 1; half >>= 1) {
    const bool upper = (lane & half) != 0;
#pragma unroll
    for (int i = 0; i < half; i++) {
      const double send = upper ? v[i] : v[i + half], keep = upper ? v[i + half] : v[i];
      v[i] = keep + __shfl_xor(send, half, 64);
    }
  }
  s_sum[wave][lane] = v[0];
  if (PASS == 0) s_cnt[wave][lane] = n;
  block_sync_lds();
  if (wave != 0) return;
  double t = s_sum[0][lane];
#pragma unroll
  for (int w = 1; w < kFoldWaves; w++) t = t + s_sum[w][lane];
  const size_t at = ((size_t)blockIdx.y * kS + lane) * (size_t)P + blockIdx.x;
  a.slab[at] = t;
  if (PASS == 0) {
    int c = s_cnt[0][lane];
#pragma unroll
    for (int w = 1; w < kFoldWaves; w++) c += s_cnt[w][lane];
    a.cslab[at] = c;
  }
}

template <int PASS>
__global__ __launch_bounds__(64) void rg_fold_kernel(RigidGroupsArgs a, int k0) {
  const int slot = blockIdx.x, lane = threadIdx.x, R = a.R;
  int bp, bq;
  block_pair(k0 + slot / kS, rg_blocks(R), &bp, &bq);
  const int p = bp * kB + slot % kS / kB, q = bq * kB + slot % kB;
  if (p >= R || q >= R || p > q) return;
  const int64_t P = rg_tiles(a.n_frames);
  double v[1];
  slab_fold<1, -1>(a.slab + (size_t)slot * P, P, 0.0, v);
  const size_t pq = (size_t)p * R + q, qp = (size_t)q * R + p;
  if (PASS == 0) {
    int c = 0;
    for (int64_t e = lane; e < P; e += 64) c += a.cslab[(size_t)slot * P + e];
    for (int off = 32; off; off >>= 1) c += __shfl_down(c, off);
    if (lane != 0) return;
    const double mean = c ? v[0] / (double)c : __builtin_nan("");
    a.cnt[pq] = c;
    a.cnt[qp] = c;
    a.dist[pq] = mean;
    a.dist[qp] = mean;
  } else {
    if (lane != 0) return;
    const int c = a.cnt[pq];
    const double s = c ? sqrt(v[0] / (double)c) : __builtin_nan("");
    a.spread[pq] = s;
    a.spread[qp] = s;
  }
}

// ------------------------------------------------------------------------------------------------------------------ groups
__global__ __launch_bounds__(kRgMaxRows) void rg_group_kernel(RigidGroupsArgs a) {
  __shared__ unsigned s_edge[kRgMaxRows][kWords];
  __shared__ int s_label[kRgMaxRows], s_scan[kRgMaxRows];
  __shared__ unsigned char s_elig[kRgMaxRows];
  __shared__ int s_size[kRgMaxRows], s_conf[kRgMaxRows];     // per component, at its lowest row
  __shared__ unsigned long long s_worst[kRgMaxRows];         // the bits of the largest spread over its edges
  __shared__ int s_changed;
  const int R = a.R, r = threadIdx.x;
  const bool mine = r < R;
  // travel, eligibility
  if (mine) {
    const int n = a.cnt[(size_t)r * R + r];
    double tr = __builtin_nan("");
    if (n > 0) {
      double e[3];
#pragma unroll
      for (int k = 0; k < 3; k++) e[k] = value_of(a.bounds[6 * r + 3 + k]) - value_of(a.bounds[6 * r + k]);
      tr = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    }
    a.travel[r] = tr;
    s_elig[r] = n >= a.min_common && tr >= a.min_travel;
  }
  s_label[r] = r;
  s_size[r] = 0;
  s_conf[r] = 0;
  s_worst[r] = 0ull;
  if (r == 0) s_changed = 0;
  block_sync_lds();
  // edges: lane r walks column r of the symmetric tables (neighbouring lanes, neighbouring entries)
  bool has_edge = false;
#pragma unroll
  for (int w = 0; w < kWords; w++) {
    unsigned bits = 0;
    if (mine && s_elig[r]) {
      for (int q = 32 * w; q < 32 * w + 32 && q < R; q++) {
        if (q == r || !s_elig[q]) continue;
        const size_t at = (size_t)q * R + r;
        if (a.cnt[at] >= a.min_common && a.spread[at] <= a.tol && a.dist[at] <= a.max_dist) bits |= 1u << (q - 32 * w);
      }
    }
    s_edge[r][w] = bits;
    has_edge |= bits != 0;
  }
  block_sync_lds();
  // components: the lowest label among a row and its neighbours, then pointer jumping; until a round changes nothing
  for (;;) {
    int m = s_label[r];
    if (has_edge) {
#pragma unroll
      for (int w = 0; w < kWords; w++) {
        for (unsigned bits = s_edge[r][w]; bits; bits &= bits - 1) {
          const int l = s_label[32 * w + __builtin_ctz(bits)];
          m = l < m ? l : m;
        }
      }
    }
    block_sync_lds();
    if (m != s_label[r]) {
      s_label[r] = m;
      s_changed = 1;
    }
    block_sync_lds();
    const bool again = s_changed != 0;
    for (int it = 0; it < kJumps; it++) {
      const int l = s_label[s_label[r]];
      block_sync_lds();
      s_label[r] = l;
      if (r == 0) s_changed = 0;
      block_sync_lds();
    }
    if (!again) break;
  }
  // group numbers: an inclusive prefix sum over "lowest row of a component that has an edge" (Hillis-Steele)
  const int comp = s_label[r];
  int v = has_edge && comp == r ? 1 : 0;
  s_scan[r] = v;
  block_sync_lds();
  for (int d = 1; d < kRgMaxRows; d <<= 1) {
    const int o = r >= d ? s_scan[r - d] : 0;
    block_sync_lds();
    v += o;
    s_scan[r] = v;
    block_sync_lds();
  }
  const int n_groups = s_scan[kRgMaxRows - 1];
  // the per-group figures: row r answers for its pairs (r, q), q > r, inside its component
  if (has_edge) {
    atomicAdd(&s_size[comp], 1);
    int conflicts = 0;
    unsigned long long worst = 0ull;
    for (int q = r + 1; q < R; q++) {
      if (s_label[q] != comp) continue;  // (a row without an edge keeps its own label, and q > r >= comp)
      const size_t at = (size_t)q * R + r;
      const double s = a.spread[at];
      if (a.cnt[at] >= a.min_common && !(s <= a.tol)) conflicts++;
      if (s_edge[r][q >> 5] >> (q & 31) & 1u) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(s);  // an edge's spread is finite and >= 0
        worst = b > worst ? b : worst;
      }
    }
    if (conflicts) atomicAdd(&s_conf[comp], conflicts);
    if (worst) atomicMax(&s_worst[comp], worst);
  }
  block_sync_lds();
  if (mine) {
    a.group_of[r] = has_edge ? s_scan[comp] - 1 : -1;
    if (has_edge && comp == r) {
      const int g = v - 1;
      a.gsize[g] = s_size[r];
      a.ghead[g] = r;
      a.gconf[g] = s_conf[r];
      a.gspread[g] = __longlong_as_double((long long)s_worst[r]);
    }
    if (r >= n_groups) {
      a.gsize[r] = -1;
      a.ghead[r] = -1;
      a.gconf[r] = -1;
      a.gspread[r] = __builtin_nan("");
    }
  }
  if (r == 0) *a.n_groups = n_groups;
}

}  // namespace

hipError_t launch_rigid_groups(const RigidGroupsArgs& a, hipStream_t stream) {
  const unsigned R = (unsigned)a.R, P = (unsigned)rg_tiles(a.n_frames);
  hipError_t e;
  hipLaunchKernelGGL(rg_bounds_seed_kernel, dim3((R * 6 + kT - 1) / kT), dim3(kT), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(rg_bounds_kernel, dim3(P, R), dim3(kT), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int pairs = rg_block_pairs(a.R);
  for (int k0 = 0; k0 < pairs; k0 += a.round_pairs) {
    const unsigned n = (unsigned)(pairs - k0 < a.round_pairs ? pairs - k0 : a.round_pairs);
    hipLaunchKernelGGL(rg_pair_kernel<0>, dim3(P, n), dim3(kT), 0, stream, a, k0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(rg_fold_kernel<0>, dim3(n * kS), dim3(64), 0, stream, a, k0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(rg_pair_kernel<1>, dim3(P, n), dim3(kT), 0, stream, a, k0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(rg_fold_kernel<1>, dim3(n * kS), dim3(64), 0, stream, a, k0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(rg_group_kernel, dim3(1), dim3(kRgMaxRows), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
