// point_consolidate.hip -- the "point consolidation" section of include/mocap_core.h: a frame's points compacted in place to
// the set in which no two share a blob, chosen by the walk in ascending key = (-views, bits(err), index).
//
// One workgroup per frame: ONE wave while K_max <= 64, 256 lanes up to the 256 slots the stage takes, lane = point.  (The body is
// written for lanes that stride over the points, PPT of them per lane; only PPT = 1 is built.)  A point's decision state, its rank
// and the coordinates it may have to move stay in registers.
//
// The walk, in rounds.  rank(k) = the number of keys below key(k): the position of the point in the sorted list.  The owner
// table [C][256] (LDS) holds, per blob, the smallest rank among the UNDECIDED points that use the blob.  Per round
//   (a) every undecided point sets the entries of its blobs to "none"       (b) ... and posts its rank to them with atomicMin
//   (c) a point that owns all its entries is KEPT: every conflicting point below it in the list is decided already, and none of
//       them was kept (it would have dropped this point in the round that kept it)
//   (d) an undecided point that finds a point kept in this round on one of its entries is DROPPED
// until no point is undecided.  A dropped point posts nothing any more, so it suppresses nothing: the chain A-B-C keeps A and C.
// The undecided point of the smallest rank owns all its entries, so every round decides a point; the round count is the longest
// chain of the frame.  Only entries that a point of the frame uses are ever read, so the table is never cleared as a whole.
//
// The compaction.  Rows move towards lower slots only, and in ascending order; other lanes still have to read them.  xyz and err
// of every point are in registers, and the corr rows in LDS (the row buffer: the whole frame while n * C fits it, else one group of
// consecutive rows at a time), before the first store of a slot that may be read; a barrier stands between the two phases.  A
// group's stores go to slots below the group's end, the next group reads at and above it.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace mocap {

namespace {

using u64 = unsigned long long;

// key(j) < key(k): more views first, then the smaller error bits, then the smaller index
__device__ __forceinline__ bool pc_key_less(int vj, u64 ej, int j, int vk, u64 ek, int k) {
  if (vj != vk) return vj > vk;
  if (ej != ek) return ej < ek;
  return j < k;
}

template <int T, int PPT>
__global__ __launch_bounds__(T) void point_consolidate_kernel(ConsolidateArgs a) {
  extern __shared__ __align__(16) unsigned char pc_lds[];
  const int C = a.C, K_max = a.K_max;
  u64* sErr = reinterpret_cast<u64*>(pc_lds);                                   // [K_max] bits(err)
  unsigned* sTab = reinterpret_cast<unsigned*>(sErr + K_max);                   // [C][256] owner table
  int* sViews = reinterpret_cast<int*>(sTab + (size_t)C * kPcBlobs);            // [K_max]
  int* sKept = sViews + K_max;                                                  // [K_max] by RANK: kept in the current round or before
  int* sChunk = sKept + K_max;                                                  // [16] points kept per 64 consecutive slots
  int16_t* sRows = reinterpret_cast<int16_t*>(sChunk + 16);                     // [pc_row_entries] corr rows
  constexpr int kWaves = T / 64;
  static_assert(PPT * kWaves <= 16, "sChunk holds 16 chunk counts");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t f = blockIdx.x;
  const int n = a.n_pts[f];
  const int st = a.status ? a.status[f] : 0;
  if ((st & kPcStatusSkip) != 0 || n < 0 || n > K_max) {  // (uniform) not processed: byte for byte as it is
    if (tid == 0 && a.n_in) a.n_in[f] = -1;
    return;
  }
  double* gx = a.xyz + (size_t)f * K_max * 3;
  double* ge = a.err + (size_t)f * K_max;
  int16_t* gc = a.corr + (size_t)f * K_max * C;

  // the coordinates and errors this lane may have to move (every slot of the buffers is readable)
  double px[PPT][3], pe[PPT];
#pragma unroll
  for (int i = 0; i < PPT; i++) {
    const int k = i * T + tid;
    px[i][0] = px[i][1] = px[i][2] = pe[i] = 0.0;
    if (k < n) {
      px[i][0] = gx[k * 3 + 0];
      px[i][1] = gx[k * 3 + 1];
      px[i][2] = gx[k * 3 + 2];
      pe[i] = ge[k];
    }
  }
  // the rows: checked, and staged whole where the buffer holds them
  const int rows_cap = pc_row_entries(C, K_max) / C;  // rows the buffer holds (>= 1)
  const bool staged = n <= rows_cap;
  int bad = 0;
  for (int e = tid; e < n * C; e += T) {
    const int v = gc[e];
    if (v < -1 || v >= kPcBlobs) bad = 1;
    if (staged) sRows[e] = (int16_t)v;
  }
  if (__syncthreads_or(bad)) {  // an entry outside -1 .. 255: not processed
    if (tid == 0 && a.n_in) a.n_in[f] = -1;
    return;
  }
  const int16_t* rows = staged ? sRows : gc;  // (LDS or global: a generic pointer)

  // ---- views and error bits, then the rank
  int state[PPT], rank[PPT];  // state: 0 undecided, 1 kept, 2 dropped (slots >= n: 2)
#pragma unroll
  for (int i = 0; i < PPT; i++) {
    const int k = i * T + tid;
    state[i] = k < n ? 0 : 2;
    rank[i] = 0;
    if (k < n) {
      int v = 0;
      for (int c = 0; c < C; c++) v += rows[k * C + c] >= 0 ? 1 : 0;
      sViews[k] = v;
      sErr[k] = (u64)__double_as_longlong(pe[i]);
      sKept[k] = 0;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PPT; i++) {
    const int k = i * T + tid;
    if (k < n) {
      const int vk = sViews[k];
      const u64 ek = sErr[k];
      int r = 0;
      for (int j = 0; j < n; j++) r += pc_key_less(sViews[j], sErr[j], j, vk, ek, k) ? 1 : 0;
      rank[i] = r;
    }
  }

  // ---- the rounds
  for (;;) {
#pragma unroll
    for (int i = 0; i < PPT; i++) {  // (a)
      const int k = i * T + tid;
      if (state[i] == 0)
        for (int c = 0; c < C; c++) {
          const int b = rows[k * C + c];
          if (b >= 0) sTab[c * kPcBlobs + b] = 0xFFFFFFFFu;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PPT; i++) {  // (b)
      const int k = i * T + tid;
      if (state[i] == 0)
        for (int c = 0; c < C; c++) {
          const int b = rows[k * C + c];
          if (b >= 0) atomicMin(&sTab[c * kPcBlobs + b], (unsigned)rank[i]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PPT; i++) {  // (c)
      const int k = i * T + tid;
      if (state[i] == 0) {
        bool own = true;
        for (int c = 0; c < C; c++) {
          const int b = rows[k * C + c];
          if (b >= 0 && sTab[c * kPcBlobs + b] != (unsigned)rank[i]) own = false;
        }
        if (own) {
          state[i] = 1;
          sKept[rank[i]] = 1;
        }
      }
    }
    __syncthreads();
    int undecided = 0;
#pragma unroll
    for (int i = 0; i < PPT; i++) {  // (d)
      const int k = i * T + tid;
      if (state[i] == 0) {
        bool drop = false;
        for (int c = 0; c < C; c++) {
          const int b = rows[k * C + c];
          if (b >= 0 && sKept[sTab[c * kPcBlobs + b]] != 0) drop = true;  // (the entry holds the rank of a point of this frame: < n)
        }
        if (drop) state[i] = 2; else undecided = 1;
      }
    }
    if (!__syncthreads_or(undecided)) break;
  }

  // ---- new slots: the kept points below this one
  const u64 lt = (1ull << lane) - 1;
  int below[PPT];
#pragma unroll
  for (int i = 0; i < PPT; i++) {
    const u64 m = __ballot(state[i] == 1);  // the 64 consecutive slots (i * kWaves + wave) * 64 ...
    below[i] = __popcll(m & lt);
    if (lane == 0) sChunk[i * kWaves + wave] = __popcll(m);
  }
  __syncthreads();
  int n_new = 0, dst[PPT];
#pragma unroll
  for (int i = 0; i < PPT; i++) dst[i] = below[i];
  for (int ch = 0; ch < PPT * kWaves; ch++) {
    const int cnt = sChunk[ch];
    n_new += cnt;
#pragma unroll
    for (int i = 0; i < PPT; i++)
      if (ch < i * kWaves + wave) dst[i] += cnt;
  }
  if (tid == 0 && a.n_in) a.n_in[f] = n;
  if (a.src) {
#pragma unroll
    for (int i = 0; i < PPT; i++)
      if (state[i] == 1) a.src[(size_t)f * K_max + dst[i]] = i * T + tid;
  }
  if (n_new == n) return;  // (uniform) nothing dropped: every row is where it belongs

  // ---- the compaction: every load of xyz and err has come back before the first store of the frame
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PPT; i++) {
    const int k = i * T + tid, d = dst[i];
    if (state[i] == 1 && d != k) {
      gx[d * 3 + 0] = px[i][0];
      gx[d * 3 + 1] = px[i][1];
      gx[d * 3 + 2] = px[i][2];
      ge[d] = pe[i];
    }
  }
  if (tid == 0) a.n_pts[f] = n_new;
  // the rows, a group of consecutive slots at a time through the row buffer; the new slot of a row travels in sViews (free by now)
#pragma unroll
  for (int i = 0; i < PPT; i++) {
    const int k = i * T + tid;
    if (k < n) sViews[k] = state[i] == 1 ? dst[i] : -1;
  }
  for (int r0 = 0; r0 < n; r0 += rows_cap) {
    const int r1 = r0 + rows_cap < n ? r0 + rows_cap : n;
    if (!staged) {  // (staged: the buffer holds rows 0 .. n since the start)
      __syncthreads();  // the previous group's rows have been written out
      for (int e = tid; e < (r1 - r0) * C; e += T) sRows[e] = gc[r0 * C + e];
    }
    __syncthreads();  // (also: sViews)
    for (int e = tid; e < (r1 - r0) * C; e += T) {
      const int k = r0 + e / C, d = sViews[k];
      if (d >= 0 && d != k) gc[d * C + (e - (k - r0) * C)] = sRows[e];
    }
  }
}

}  // namespace

hipError_t launch_point_consolidate(const ConsolidateArgs& a, hipStream_t stream) {
  if (a.n_frames <= 0) return hipSuccess;
  if (a.C < 1 || a.C > 64 || a.K_max < 1 || a.K_max > kPcMaxPoints || a.n_frames > 0x7fffffffll) return hipErrorInvalidValue;
  void (*k)(ConsolidateArgs);
  int T;
  if (a.K_max <= 64) {
    k = point_consolidate_kernel<64, 1>;
    T = 64;
  } else {
    k = point_consolidate_kernel<256, 1>;
    T = 256;
  }
  const size_t lds = pc_lds_bytes(a.C, a.K_max);
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k, dim3((unsigned)a.n_frames), dim3(T), lds, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
