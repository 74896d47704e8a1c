// joints.hip -- which bodies of a session are joined, where and how, and a joint's motion per frame (include/mocap_core.h, "joints").
//   pairs    lanes are frames: one workgroup of 256 lanes per (block pair, 256-frame tile), a block pair = 4 bodies a x 4 bodies b
//            with block(a) <= block(b); the grid runs over the block pairs first, so the workgroups in flight share a tile's poses
//            in L2 (64 bodies x 256 frames x 96 B = 1.5 MB).  A lane holds its frame's pose of the 4 b bodies in registers, takes
//            the a bodies in turn and forms the 4 x 16 values Rel (9), d (3), g (3), d.d -- +0.0 where either body is absent.  Each
//            wave folds its 64 values over its 64 lanes TRANSPOSED, as rigid_groups.hip does: 63 exchanges, and lane l ends with the
//            wave sum of value l in the association order of tree_fold.hpp's wave_fold (IEEE + commutes).  The counts are the
//            population of the wave's presence ballot, exact.  All 256 lanes then add the four wave sums of one slot each in wave
//            order (block_fold's order) and write one slab entry per (tile, slot): slab [slot][tile].
//   fold     one wave per slot: tree_fold.hpp's slab_fold over the slot's P tile sums -> sums [a][b][16], cnt.
//   solve    one lane per pair a < b (2 016 at most): Rbar, M, rhs; jacobi6.hpp; the order of the eigenvalues by rank, every
//            index a constant after unrolling; kind, the three smallest eigenvalues, the minimum-norm centres, the hinge axis, both
//            halves of every table; the lanes of the diagonal write its constants.
//   residual the pair pass once more with one value per pair, e.e from the rounded centres (staged in LDS: 96 uniform doubles
//            do not fit the SGPRs); the fold's first two steps keep all 16 values, the last four halve them.  Its fold writes sep
//            and accepted.
//   skeleton one workgroup of 256 lanes: the accepted pairs listed in LDS, each ranked by counting the keys (bits of sep, a, b) below
//            its own; lane 0 runs Kruskal over the ranked list with a union-find that keeps the lowest body on top, so a root is its
//            component's lowest body; the parents by a sweep over the tree edges per level, one lane per edge.
//   series   one lane per (joint, frame), frames along the lanes, the joint's table entry uniform per workgroup.
// FP64 throughout, nothing fused (-ffp-contract=off is the build's rule), / and sqrt correctly rounded, no floating-point atomics
// (one 32-bit integer counter in LDS, whose order no output depends on): the outputs are a function of the input alone.
#include "joints.hpp"

#include "body_session.hpp"
#include "jacobi6.hpp"
#include "mocap_device.hpp"
#include "track_smooth.hpp"
#include "tree_fold.hpp"

namespace mocap {

namespace {

constexpr int kT = kJtTile, kB = kJtBlock, kMaxEdges = kJtMaxBodies * (kJtMaxBodies - 1) / 2;
static_assert(kT == kCalibThreads && kJtSlots == kT && kB * kJtSums == 64, "the tile is tree_fold.hpp's; a body a and its 4 b fill one wave's fold");
static_assert(kJtMaxBodies == kBpMaxBodies && sizeof(JtJoint) == 128, "limits");

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

// the pose of (body, f): Rm row-major in p[0 .. 9), t_pose in p[9 .. 12); -> POSED and twelve finite values
__device__ __forceinline__ bool load_pose(const FindJointsArgs& a, int body, int64_t f, double (&p)[12]) {
#pragma unroll
  for (int k = 0; k < 12; k++) p[k] = 0.0;
  if (body >= a.B || f >= a.n_frames) return false;
  const size_t at = (size_t)body * (size_t)a.n_frames + (size_t)f;
  if (a.flag[at] != kBpPosed) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    p[k] = a.Rm[at * 9 + k];
    ok = ok && finite1(p[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    p[9 + k] = a.t_pose[at * 3 + k];
    ok = ok && finite1(p[9 + k]);
  }
  return ok;
}

__device__ __forceinline__ double keep_if(double v, bool keep) { return keep ? v : 0.0; }  // absent: +0.0

// N values per lane -> lane l holds the wave sum of value l & (N - 1), in wave_fold's association order
template <int N>
__device__ __forceinline__ void transposed_fold(double (&v)[N], int lane) {
#pragma unroll
  for (int half = 32; half >= 1; half >>= 1) {
    if (half >= N) {
#pragma unroll
      for (int i = 0; i < N; i++) v[i] = v[i] + __shfl_xor(v[i], half, 64);
    } else {
      const bool upper = (lane & half) != 0;
#pragma unroll
      for (int i = 0; i < half; i++) {
        const double lo = v[i], hi = v[i + half];  // (values first: a conditional between two elements is one between addresses)
        const double send = upper ? lo : hi, keep = upper ? hi : lo;
        v[i] = keep + __shfl_xor(send, half, 64);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ pair sums
__global__ __launch_bounds__(kT) void jt_sums_kernel(FindJointsArgs a, int k0) {
  __shared__ double s_sum[kFoldWaves][kJtSlots];
  __shared__ int s_cnt[kFoldWaves][kJtPairs];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t P = jt_tiles(a.n_frames), f = (int64_t)blockIdx.y * kT + threadIdx.x;
  int bp, bq;
  block_pair(k0 + blockIdx.x, jt_blocks(a.B), &bp, &bq);
  const int a0 = bp * kB, b0 = bq * kB;
  double pb[kB][12];
  bool okb[kB];
#pragma unroll
  for (int j = 0; j < kB; j++) okb[j] = load_pose(a, b0 + j, f, pb[j]);
#pragma unroll
  for (int i = 0; i < kB; i++) {
    double pa[12];
    const bool oka = load_pose(a, a0 + i, f, pa);
    double v[64];
#pragma unroll
    for (int j = 0; j < kB; j++) {
      const bool both = oka && okb[j];
      const int n = __popcll(__ballot(both));
      if (lane == 0) s_cnt[wave][i * kB + j] = n;
      double rel[9], d[3];
      const double dt0 = pb[j][9] - pa[9], dt1 = pb[j][10] - pa[10], dt2 = pb[j][11] - pa[11];
#pragma unroll
      for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) rel[3 * r + c] = (pa[r] * pb[j][c] + pa[3 + r] * pb[j][3 + c]) + pa[6 + r] * pb[j][6 + c];
        d[r] = (pa[r] * dt0 + pa[3 + r] * dt1) + pa[6 + r] * dt2;
      }
#pragma unroll
      for (int k = 0; k < 9; k++) v[16 * j + k] = keep_if(rel[k], both);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        v[16 * j + 9 + k] = keep_if(d[k], both);
        v[16 * j + 12 + k] = keep_if((rel[k] * d[0] + rel[3 + k] * d[1]) + rel[6 + k] * d[2], both);
      }
      v[16 * j + 15] = keep_if((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], both);
    }
    transposed_fold<64>(v, lane);
    s_sum[wave][64 * i + lane] = v[0];
  }
  block_sync_lds();
  double t = s_sum[0][threadIdx.x];
#pragma unroll
  for (int w = 1; w < kFoldWaves; w++) t = t + s_sum[w][threadIdx.x];
  a.slab[((size_t)blockIdx.x * kJtSlots + threadIdx.x) * (size_t)P + blockIdx.y] = t;
  if (threadIdx.x < kJtPairs) {
    int c = s_cnt[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kFoldWaves; w++) c += s_cnt[w][threadIdx.x];
    a.cslab[((size_t)blockIdx.x * kJtPairs + threadIdx.x) * (size_t)P + blockIdx.y] = c;
  }
}

// one wave per slot of the round: sums [a][b][16] for a < b, cnt for a <= b (both halves)
__global__ __launch_bounds__(64) void jt_sums_fold_kernel(FindJointsArgs a, int k0) {
  const int slot = blockIdx.x % kJtSlots, local = blockIdx.x / kJtSlots, lane = threadIdx.x, B = a.B;
  int bp, bq;
  block_pair(k0 + local, jt_blocks(B), &bp, &bq);
  const int pair = slot / kJtSums, s = slot % kJtSums;
  const int p = bp * kB + pair / kB, q = bq * kB + pair % kB;
  if (p >= B || q >= B || p > q || (p == q && s != 0)) return;
  const int64_t P = jt_tiles(a.n_frames);
  if (s == 0) {
    const int32_t* cs = a.cslab + ((size_t)local * kJtPairs + pair) * (size_t)P;
    int c = 0;
    for (int64_t e = lane; e < P; e += 64) c += cs[e];
    for (int off = 32; off; off >>= 1) c += __shfl_down(c, off);
    if (lane == 0) {
      a.cnt[(size_t)p * B + q] = c;
      a.cnt[(size_t)q * B + p] = c;
    }
  }
  if (p == q) return;
  double v[1];
  slab_fold<1, -1>(a.slab + (size_t)blockIdx.x * (size_t)P, P, 0.0, v);
  if (lane == 0) a.sums[((size_t)p * B + q) * kJtSums + s] = v[0];
}

// ------------------------------------------------------------------------------------------------------------------ solve
__device__ __forceinline__ void put3(double* table, int B, int p, int q, double x, double y, double z) {
  double* o = table + ((size_t)p * B + q) * 3;
  o[0] = x;
  o[1] = y;
  o[2] = z;
}

__global__ __launch_bounds__(64) void jt_solve_kernel(FindJointsArgs a) {
  const int B = a.B, id = blockIdx.x * 64 + threadIdx.x;
  if (id >= B * B) return;
  const int p = id / B, q = id % B;
  if (p > q) return;
  const size_t pq = (size_t)p * B + q, qp = (size_t)q * B + p;
  const double nan = __builtin_nan("");
  int kind = kJtUnseen;
  double lam3[3] = {nan, nan, nan}, ca[3] = {nan, nan, nan}, cb[3] = {nan, nan, nan}, xa[3] = {nan, nan, nan}, xb[3] = {nan, nan, nan};
  const int n = a.cnt[pq];
  if (p != q && n >= a.min_common) {
    const double dn = (double)n;
    double m[kJtSums];
#pragma unroll
    for (int k = 0; k < kJtSums; k++) m[k] = a.sums[pq * kJtSums + k] / dn;
    double A[6][6], V[6][6];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        A[i][j] = A[3 + i][3 + j] = i == j ? 1.0 : 0.0;
        A[i][3 + j] = A[3 + j][i] = -m[3 * i + j];
      }
    const double rhs[6] = {m[9], m[10], m[11], -m[12], -m[13], -m[14]};
    jacobi6(A, V);
    bool finite = true;
    int small = 0, rank[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
      finite = finite && finite1(A[k][k]);
      small += A[k][k] <= a.tol_rank ? 1 : 0;
      rank[k] = 0;
#pragma unroll
      for (int i = 0; i < 6; i++) {
        finite = finite && finite1(V[i][k]);
        if (i != k) rank[k] += A[i][i] < A[k][k] || (A[i][i] == A[k][k] && i < k) ? 1 : 0;
      }
    }
    if (!finite) {
      kind = kJtSingular;
    } else {
      kind = small >= 2 ? kJtFixed : small == 1 ? kJtHinge : kJtBall;
      double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, v0[6];
#pragma unroll
      for (int r = 0; r < 6; r++) {
        double lam = 0.0, col[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 6; k++) {
          if (rank[k] == r) {
            lam = A[k][k];
#pragma unroll
            for (int i = 0; i < 6; i++) col[i] = V[i][k];
          }
        }
        if (r < 3) lam3[r] = lam;
        if (r == 0) {
#pragma unroll
          for (int i = 0; i < 6; i++) v0[i] = col[i];
        }
        if (lam > a.tol_rank) {
          double h = 0.0;
#pragma unroll
          for (int i = 0; i < 6; i++) h = h + col[i] * rhs[i];
          h = h / lam;
#pragma unroll
          for (int i = 0; i < 6; i++) x[i] = x[i] + h * col[i];
        }
      }
#pragma unroll
      for (int k = 0; k < 3; k++) {
        ca[k] = x[k];
        cb[k] = x[3 + k];
      }
      if (kind == kJtHinge) {
        const double na = sqrt((v0[0] * v0[0] + v0[1] * v0[1]) + v0[2] * v0[2]);
        const double nb = sqrt((v0[3] * v0[3] + v0[4] * v0[4]) + v0[5] * v0[5]);
        if (!(na > 0.0) || !(nb > 0.0)) {
          kind = kJtSingular;
        } else {
#pragma unroll
          for (int k = 0; k < 3; k++) {
            xa[k] = v0[k] / na;
            xb[k] = v0[3 + k] / nb;
          }
          const double lead = xa[0] != 0.0 ? xa[0] : xa[1] != 0.0 ? xa[1] : xa[2];
          if (lead < 0.0) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
              xa[k] = -xa[k];
              xb[k] = -xb[k];
            }
          }
        }
      }
    }
    if (kind == kJtSingular) {  // (the axes are still NaN)
#pragma unroll
      for (int k = 0; k < 3; k++) lam3[k] = ca[k] = cb[k] = nan;
    }
  }
  a.kind[pq] = kind;
  a.kind[qp] = kind;
  put3(a.lam, B, p, q, lam3[0], lam3[1], lam3[2]);
  put3(a.lam, B, q, p, lam3[0], lam3[1], lam3[2]);
  put3(a.centre, B, p, q, ca[0], ca[1], ca[2]);
  put3(a.centre, B, q, p, cb[0], cb[1], cb[2]);
  put3(a.axis, B, p, q, xa[0], xa[1], xa[2]);
  put3(a.axis, B, q, p, xb[0], xb[1], xb[2]);
  if (kind < kJtFixed) {  // no residual pass will write these (the diagonal included)
    a.sep[pq] = nan;
    a.sep[qp] = nan;
    a.accepted[pq] = 0;
    a.accepted[qp] = 0;
  }
}

// ------------------------------------------------------------------------------------------------------------------ residual
__global__ __launch_bounds__(kT) void jt_residual_kernel(FindJointsArgs a, int k0) {
  __shared__ double s_c[kJtPairs][6];  // c_a, c_b of the block pair's pairs; then the wave sums
  __shared__ double s_sum[kFoldWaves][kJtPairs];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, B = a.B;
  const int64_t P = jt_tiles(a.n_frames), f = (int64_t)blockIdx.y * kT + threadIdx.x;
  int bp, bq;
  block_pair(k0 + blockIdx.x, jt_blocks(B), &bp, &bq);
  const int a0 = bp * kB, b0 = bq * kB;
  if (threadIdx.x < kJtPairs * 6) {
    const int pair = threadIdx.x / 6, k = threadIdx.x % 6;
    const int p = a0 + pair / kB, q = b0 + pair % kB;
    double c = 0.0;  // (a pair beyond B, or not a < b, is never folded)
    if (p < B && q < B && p < q) c = k < 3 ? a.centre[((size_t)p * B + q) * 3 + k] : a.centre[((size_t)q * B + p) * 3 + (k - 3)];
    s_c[pair][k] = c;
  }
  block_sync_lds();
  double pb[kB][12];
  bool okb[kB];
#pragma unroll
  for (int j = 0; j < kB; j++) okb[j] = load_pose(a, b0 + j, f, pb[j]);
  double v[kJtPairs];
#pragma unroll
  for (int i = 0; i < kB; i++) {
    double pa[12];
    const bool oka = load_pose(a, a0 + i, f, pa);
#pragma unroll
    for (int j = 0; j < kB; j++) {
      const double* c = s_c[i * kB + j];
      double e[3];
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const double wa = ((pa[3 * r] * c[0] + pa[3 * r + 1] * c[1]) + pa[3 * r + 2] * c[2]) + pa[9 + r];
        const double wb = ((pb[j][3 * r] * c[3] + pb[j][3 * r + 1] * c[4]) + pb[j][3 * r + 2] * c[5]) + pb[j][9 + r];
        e[r] = wa - wb;
      }
      v[i * kB + j] = keep_if((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], oka && okb[j]);
    }
  }
  transposed_fold<kJtPairs>(v, lane);
  if (lane < kJtPairs) s_sum[wave][lane] = v[0];
  block_sync_lds();
  if (threadIdx.x >= kJtPairs) return;
  double t = s_sum[0][threadIdx.x];
#pragma unroll
  for (int w = 1; w < kFoldWaves; w++) t = t + s_sum[w][threadIdx.x];
  a.slab[((size_t)blockIdx.x * kJtPairs + threadIdx.x) * (size_t)P + blockIdx.y] = t;
}

__global__ __launch_bounds__(64) void jt_residual_fold_kernel(FindJointsArgs a, int k0) {
  const int pair = blockIdx.x % kJtPairs, local = blockIdx.x / kJtPairs, lane = threadIdx.x, B = a.B;
  int bp, bq;
  block_pair(k0 + local, jt_blocks(B), &bp, &bq);
  const int p = bp * kB + pair / kB, q = bq * kB + pair % kB;
  if (p >= B || q >= B || p >= q) return;
  const size_t pq = (size_t)p * B + q, qp = (size_t)q * B + p;
  const int kind = a.kind[pq];
  if (kind < kJtFixed) return;  // the solve wrote NaN and 0
  const int64_t P = jt_tiles(a.n_frames);
  double v[1];
  slab_fold<1, -1>(a.slab + (size_t)blockIdx.x * (size_t)P, P, 0.0, v);
  if (lane != 0) return;
  const double sep = sqrt(v[0] / (double)a.cnt[pq]);
  const int acc = (kind == kJtHinge || kind == kJtBall) && sep <= a.max_sep ? 1 : 0;
  a.sep[pq] = sep;
  a.sep[qp] = sep;
  a.accepted[pq] = acc;
  a.accepted[qp] = acc;
}

// ------------------------------------------------------------------------------------------------------------------ skeleton
__global__ __launch_bounds__(kT) void jt_skeleton_kernel(FindJointsArgs a) {
  __shared__ unsigned long long s_key[kMaxEdges];  // the bits of sep (finite or +inf, >= 0: they order like the value)
  __shared__ unsigned short s_id[kMaxEdges], s_order[kMaxEdges];  // 64 a + b; the edge of each rank
  __shared__ unsigned char s_top[kJtMaxBodies], s_seen[kJtMaxBodies], s_u[kJtMaxBodies], s_v[kJtMaxBodies];
  __shared__ int s_parent[kJtMaxBodies];
  __shared__ int s_n, s_tree;
  const int B = a.B, t = threadIdx.x;
  if (t == 0) s_n = s_tree = 0;
  block_sync_lds();
  for (int id = t; id < B * B; id += kT) {
    const int p = id / B, q = id % B;
    if (p < q && a.accepted[id]) {
      const int e = atomicAdd(&s_n, 1);  // (the list's order does not matter: the ranks below are a function of the keys)
      s_key[e] = (unsigned long long)__double_as_longlong(a.sep[id]);
      s_id[e] = (unsigned short)(p * kJtMaxBodies + q);
    }
  }
  block_sync_lds();
  const int n = s_n;
  for (int e = t; e < n; e += kT) {
    const unsigned long long key = s_key[e];
    const unsigned id = s_id[e];
    int r = 0;
    for (int o = 0; o < n; o++) r += s_key[o] < key || (s_key[o] == key && s_id[o] < id) ? 1 : 0;
    s_order[r] = (unsigned short)e;
  }
  if (t < kJtMaxBodies) {
    s_top[t] = (unsigned char)t;
    s_parent[t] = -1;
  }
  block_sync_lds();
  if (t == 0) {
    int tree = 0;
    for (int r = 0; r < n; r++) {
      const unsigned id = s_id[s_order[r]];
      const int p = (int)(id / kJtMaxBodies), q = (int)(id % kJtMaxBodies);
      int x = p, y = q;
      while (s_top[x] != x) x = s_top[x];
      while (s_top[y] != y) y = s_top[y];
      if (x == y) continue;
      if (x < y) s_top[y] = (unsigned char)x; else s_top[x] = (unsigned char)y;
      s_u[tree] = (unsigned char)p;
      s_v[tree] = (unsigned char)q;
      tree++;
    }
    s_tree = tree;
  }
  block_sync_lds();
  if (t < kJtMaxBodies) s_seen[t] = s_top[t] == t;  // the top of a set is its lowest body: a root (or a body of no pair)
  block_sync_lds();
  const int tree = s_tree;
  for (int level = 1; level < B; level++) {  // (a tree of B bodies is at most B - 1 deep; every step is uniform)
    int child = -1, par = -1;
    if (t < tree) {
      const int u = s_u[t], v = s_v[t];
      if (s_seen[u] && !s_seen[v]) {
        child = v;
        par = u;
      } else if (s_seen[v] && !s_seen[u]) {
        child = u;
        par = v;
      }
    }
    block_sync_lds();
    if (child >= 0) {  // (in a tree one edge alone leads from the seen part to a body)
      s_parent[child] = par;
      s_seen[child] = 1;
    }
    block_sync_lds();
  }
  if (t < B) a.parent[t] = s_parent[t];
  if (t == 0) *a.n_joints = tree;
}

// ------------------------------------------------------------------------------------------------------------------ series
__global__ __launch_bounds__(64) void jt_put_kernel(JtJointChunk c, int count, JtJoint* dst) {
  constexpr int kWords = (int)(sizeof(JtJoint) / sizeof(unsigned long long));
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&c);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(dst);
  for (int i = threadIdx.x; i < count * kWords; i += 64) out[i] = src[i];
}

// the Hamilton product p (x) q, term by term
__device__ __forceinline__ void hamilton(const double (&p)[4], const double (&q)[4], double (&o)[4]) {
  o[0] = ((p[0] * q[0] - p[1] * q[1]) - p[2] * q[2]) - p[3] * q[3];
  o[1] = ((p[0] * q[1] + p[1] * q[0]) + p[2] * q[3]) - p[3] * q[2];
  o[2] = ((p[0] * q[2] - p[1] * q[3]) + p[2] * q[0]) + p[3] * q[1];
  o[3] = ((p[0] * q[3] + p[1] * q[2]) - p[2] * q[1]) + p[3] * q[0];
}

__global__ __launch_bounds__(kT) void jt_series_kernel(JointSeriesArgs a) {
  const int j = blockIdx.y;
  const int64_t F = a.n_frames, f = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (f >= F) return;
  const JtJoint& jt = a.joints[j];
  const size_t at_a = (size_t)jt.a * (size_t)F + (size_t)f, at_b = (size_t)jt.b * (size_t)F + (size_t)f, at = (size_t)j * (size_t)F + (size_t)f;
  const double nan = __builtin_nan("");
  const bool present = a.flag[at_a] == kBpPosed && a.flag[at_b] == kBpPosed;
  double centre[3] = {nan, nan, nan}, gap = nan, qr[4] = {nan, nan, nan, nan}, tw[2] = {nan, nan};
  if (present) {
    double e[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const double* ra = a.Rm + at_a * 9 + 3 * r;
      const double* rb = a.Rm + at_b * 9 + 3 * r;
      const double wa = ((ra[0] * jt.c_a[0] + ra[1] * jt.c_a[1]) + ra[2] * jt.c_a[2]) + a.t_pose[at_a * 3 + r];
      const double wb = ((rb[0] * jt.c_b[0] + rb[1] * jt.c_b[1]) + rb[2] * jt.c_b[2]) + a.t_pose[at_b * 3 + r];
      centre[r] = (wa + wb) * 0.5;
      e[r] = wa - wb;
    }
    gap = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    const double* qa = a.quat + at_a * 4;
    const double* qb = a.quat + at_b * 4;
    const double ca[4] = {qa[0], -qa[1], -qa[2], -qa[3]}, b4[4] = {qb[0], qb[1], qb[2], qb[3]};
    const double cr[4] = {jt.q_ref[0], -jt.q_ref[1], -jt.q_ref[2], -jt.q_ref[3]};
    double ab[4];
    hamilton(ca, b4, ab);
    hamilton(cr, ab, qr);
    if (jt.kind == kJtHinge) {
      const double s = (qr[1] * jt.axis_b[0] + qr[2] * jt.axis_b[1]) + qr[3] * jt.axis_b[2];
      const double m = sqrt(qr[0] * qr[0] + s * s);
      if (m > 0.0) {
        tw[0] = qr[0] / m;
        tw[1] = s / m;
      }
    }
  }
  a.present[at] = present ? 1 : 0;
  a.gap[at] = gap;
#pragma unroll
  for (int k = 0; k < 3; k++) a.centre[at * 3 + k] = centre[k];
#pragma unroll
  for (int k = 0; k < 4; k++) a.quat_rel[at * 4 + k] = qr[k];
  a.twist[at * 2] = tw[0];
  a.twist[at * 2 + 1] = tw[1];
}

}  // namespace

hipError_t launch_find_joints(const FindJointsArgs& a, hipStream_t stream) {
  const unsigned P = (unsigned)jt_tiles(a.n_frames);
  const int pairs = jt_block_pairs(a.B);
  hipError_t e;
  for (int k0 = 0; k0 < pairs; k0 += a.round_pairs) {
    const unsigned n = (unsigned)(pairs - k0 < a.round_pairs ? pairs - k0 : a.round_pairs);
    hipLaunchKernelGGL(jt_sums_kernel, dim3(n, P), dim3(kT), 0, stream, a, k0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jt_sums_fold_kernel, dim3(n * kJtSlots), dim3(64), 0, stream, a, k0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(jt_solve_kernel, dim3((unsigned)((a.B * a.B + 63) / 64)), dim3(64), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (int k0 = 0; k0 < pairs; k0 += a.round_pairs) {
    const unsigned n = (unsigned)(pairs - k0 < a.round_pairs ? pairs - k0 : a.round_pairs);
    hipLaunchKernelGGL(jt_residual_kernel, dim3(n, P), dim3(kT), 0, stream, a, k0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jt_residual_fold_kernel, dim3(n * kJtPairs), dim3(64), 0, stream, a, k0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(jt_skeleton_kernel, dim3(1), dim3(kT), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_put_joints(const JtJoint* host, int J, JtJoint* dev, hipStream_t stream) {
  for (int j0 = 0; j0 < J; j0 += kJtPutJoints) {
    JtJointChunk c{};
    const int count = J - j0 < kJtPutJoints ? J - j0 : kJtPutJoints;
    for (int i = 0; i < count; i++) c.j[i] = host[j0 + i];
    hipLaunchKernelGGL(jt_put_kernel, dim3(1), dim3(64), 0, stream, c, count, dev + j0);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

hipError_t launch_joint_series(const JointSeriesArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(jt_series_kernel, dim3((unsigned)jt_tiles(a.n_frames), (unsigned)a.J), dim3(kT), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
