// marker_track.hip -- the "marker tracker" section of include/mocap_core.h: which point of this frame is the marker that was
// which point of the last one.  Constant-velocity prediction, a gate, the greedy global nearest neighbour, births and
// retirement; the contract's steps 1-6 are quoted at the code that implements them.
//
// The recurrence is serial in the frames: ONE wave walks a call's frames (one workgroup of 64 lanes: its barriers are wave
// barriers).  Inside a frame lane l plays two roles, track slot l and point l.  The track state stays in registers across
// the frame loop and is written back once; a frame's points and the predictions sit in LDS, where every lane reads the
// entry the wave's loop is at (one address per read: a broadcast).  The next frame's inputs are fetched one frame ahead --
// they do not depend on the state.
//
// Association.  The contract's "admissible pairs in ascending (d2, slot, point) order, commit when both are free" is
// evaluated as rounds over two 64-bit masks (free tracks, free points): every free track lane finds its best free point by
// (d2, j), every free point lane its best free track by (d2, i), and the pairs that chose each other are committed.  The
// smallest remaining pair is always such a pair, and a pair that chose each other cannot be pre-empted by an earlier pair of
// the sorted list, so the rounds commit exactly the sorted list's pairs (tests/marker_track_reference.py states both forms;
// the CPU tests compare them).  A round commits at least one pair: at most min(tracks, points) rounds, one in nearly
// every frame of a real session.  d2 comes out of ONE function for both roles (same operands, same order, no fused operation:
// the library is built with -ffp-contract=off), so a track lane and a point lane hold the same bits for the same pair.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace mocap {

namespace {

using u64 = unsigned long long;

struct MtFrameIn {  // a frame's inputs as lane j (< K_max) holds them, as loaded (n is checked by the consumer)
  double t, x, y, z;
  int n;
};

__device__ __forceinline__ MtFrameIn mt_load_frame(const MarkerTrackArgs& a, int64_t f, int lane) {
  MtFrameIn r;
  r.t = a.t[f];
  r.n = a.n_pts[f];
  r.x = r.y = r.z = 0.0;
  if (lane < a.K_max) {  // (every slot of the buffer is readable; slots >= n are masked by the consumer)
    const double* q = a.xyz + ((size_t)f * a.K_max + lane) * 3;
    r.x = q[0];
    r.y = q[1];
    r.z = q[2];
  }
  return r;
}

__device__ __forceinline__ bool mt_finite(double v) { return __builtin_isfinite(v); }

// d2_ij of the contract: d = x_j - pred_i, summed in x, y, z order
__device__ __forceinline__ double mt_d2(double xx, double xy, double xz, double px, double py, double pz) {
  const double dx = xx - px, dy = xy - py, dz = xz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

}  // namespace

__global__ __launch_bounds__(64) void marker_track_kernel(MarkerTrackArgs a) {
  __shared__ double sX[3][64];  // the frame's points
  __shared__ double sQ[3][64];  // the live slots' predictions
  __shared__ int sBorn[64];     // r-th unmatched point of the frame
  const int lane = threadIdx.x;
  const u64 lt = (1ull << lane) - 1;  // the lanes below this one
  const u64 slots = a.T_max >= 64 ? ~0ull : (1ull << a.T_max) - 1;
  MarkerTrackState* st = a.state;
  bool live = lane < a.T_max && st->live[lane] != 0;
  int id = st->id[lane], missed = st->missed[lane], hits = st->hits[lane];
  double p0 = st->p[lane][0], p1 = st->p[lane][1], p2 = st->p[lane][2];
  double v0 = st->v[lane][0], v1 = st->v[lane][1], v2 = st->v[lane][2];
  double t_seen = st->t_seen[lane];
  int next_id = st->next_id;

  MtFrameIn nxt = mt_load_frame(a, 0, lane);
  for (int64_t f = 0; f < a.n_frames; f++) {
    const MtFrameIn in = nxt;
    if (f + 1 < a.n_frames) nxt = mt_load_frame(a, f + 1, lane);  // (inputs do not depend on the state: one frame ahead)
    const size_t fk = (size_t)f * a.K_max + lane;
    if (!mt_finite(in.t)) {  // uniform: outputs -1 / 0, the state untouched
      if (lane < a.K_max) {
        a.id[fk] = -1;
        a.hits[fk] = 0;
      }
      if (lane == 0) {
        a.n_tracks[f] = 0;
        a.status[f] = MT_ST_BAD_TIME_;
      }
      continue;
    }
    // ---- step 1: prediction
    const double dt = in.t - t_seen;
    double q0 = p0, q1 = p1, q2 = p2;
    if (dt > 0.0) {
      q0 = p0 + v0 * dt;
      q1 = p1 + v1 * dt;
      q2 = p2 + v2 * dt;
    }
    const int n = (in.n < 0 || in.n > a.K_max) ? 0 : in.n;  // the "no valid slot" rule of mocap_locate_objects
    const bool fin = lane < n && mt_finite(in.x) && mt_finite(in.y) && mt_finite(in.z);
    sX[0][lane] = in.x;
    sX[1][lane] = in.y;
    sX[2][lane] = in.z;
    sQ[0][lane] = q0;
    sQ[1][lane] = q1;
    sQ[2][lane] = q2;
    __syncthreads();
    // ---- steps 2-3: admissible pairs, association by mutual-best rounds
    u64 FT = __ballot(live), FP = __ballot(fin);  // free tracks, free points
    int my_pt = -1, my_tr = -1;                   // the point this lane's track took; the track this lane's point took
    while (FT != 0 && FP != 0) {
      double bd = a.g2, cd = a.g2;  // (admissible = strictly inside the gate: the running minimum starts at g2)
      int bj = -1, bi = -1;
      // four table entries per step, so that their LDS reads and their arithmetic overlap; an entry whose mask bit is clear is
      // computed and not used
      for (int k0 = 0; k0 < 64; k0 += 4) {
        const unsigned mp = (unsigned)(FP >> k0) & 15u, mq = (unsigned)(FT >> k0) & 15u;  // (uniform)
        if (mp != 0) {  // track role: best free point by (d2, j) -- ascending j, strict <
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int j = k0 + u;
            const double d2 = mt_d2(sX[0][j], sX[1][j], sX[2][j], q0, q1, q2);
            if (((mp >> u) & 1u) && d2 < bd) {
              bd = d2;
              bj = j;
            }
          }
        }
        if (mq != 0) {  // point role: best free track by (d2, i)
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int i = k0 + u;
            const double d2 = mt_d2(in.x, in.y, in.z, sQ[0][i], sQ[1][i], sQ[2][i]);
            if (((mq >> u) & 1u) && d2 < cd) {
              cd = d2;
              bi = i;
            }
          }
        }
      }
      if (!((FT >> lane) & 1ull)) bj = -1;
      if (!((FP >> lane) & 1ull)) bi = -1;
      const int back_tr = __shfl(bi, bj < 0 ? 0 : bj);  // the best track of this track's best point
      const int back_pt = __shfl(bj, bi < 0 ? 0 : bi);  // the best point of this point's best track
      const bool tc = bj >= 0 && back_tr == lane, pc = bi >= 0 && back_pt == lane;
      if (tc) my_pt = bj;
      if (pc) my_tr = bi;
      const u64 ct = __ballot(tc), cp = __ballot(pc);
      if (ct == 0) break;  // no admissible pair is left
      FT &= ~ct;
      FP &= ~cp;
    }
    // ---- step 4: matched slot
    if (my_pt >= 0) {
      const double x0 = sX[0][my_pt], x1 = sX[1][my_pt], x2 = sX[2][my_pt];
      if (dt > 0.0) {
        const double u0 = (x0 - p0) / dt, u1 = (x1 - p1) / dt, u2 = (x2 - p2) / dt;
        v0 = v0 + a.vel_alpha * (u0 - v0);
        v1 = v1 + a.vel_alpha * (u1 - v1);
        v2 = v2 + a.vel_alpha * (u2 - v2);
      }
      p0 = x0;
      p1 = x1;
      p2 = x2;
      t_seen = in.t;
      missed = 0;
      hits += 1;
    } else if (live) {  // ---- step 5: unmatched live slot
      missed += 1;
      if (missed > a.max_missed) live = false;  // retired: the slot is free from this moment
    }
    // ---- step 6: births -- the r-th unmatched finite point takes the r-th free slot
    const u64 free_slots = ~__ballot(live) & slots, U = FP;
    const int n_free = __popcll(free_slots), n_u = __popcll(U);
    int out_id = -1, out_hits = 0;
    if ((U >> lane) & 1ull) {
      const int r = __popcll(U & lt);
      sBorn[r] = lane;
      if (r < n_free) {
        out_id = next_id + r;
        out_hits = 1;
      }
    }
    __syncthreads();
    if ((free_slots >> lane) & 1ull) {
      const int s = __popcll(free_slots & lt);
      if (s < n_u) {
        const int j = sBorn[s];
        live = true;
        id = next_id + s;
        p0 = sX[0][j];
        p1 = sX[1][j];
        p2 = sX[2][j];
        v0 = v1 = v2 = 0.0;
        t_seen = in.t;
        missed = 0;
        hits = 1;
      }
    }
    next_id += n_u < n_free ? n_u : n_free;
    // ---- outputs
    const int m_id = __shfl(id, my_tr < 0 ? 0 : my_tr), m_hits = __shfl(hits, my_tr < 0 ? 0 : my_tr);
    if (my_tr >= 0) {
      out_id = m_id;
      out_hits = m_hits;
    }
    if (lane < a.K_max) {
      a.id[fk] = out_id;
      a.hits[fk] = out_hits;
    }
    const int n_live = __popcll(__ballot(live));
    if (lane == 0) {
      a.n_tracks[f] = n_live;
      a.status[f] = n_u > n_free ? MT_ST_FULL_ : 0;
    }
    __syncthreads();  // (the next frame overwrites the LDS tables)
  }

  st->live[lane] = live ? 1 : 0;
  st->id[lane] = id;
  st->missed[lane] = missed;
  st->hits[lane] = hits;
  st->p[lane][0] = p0;
  st->p[lane][1] = p1;
  st->p[lane][2] = p2;
  st->v[lane][0] = v0;
  st->v[lane][1] = v1;
  st->v[lane][2] = v2;
  st->t_seen[lane] = t_seen;
  if (lane == 0) st->next_id = next_id;
}

hipError_t launch_marker_tracker(const MarkerTrackArgs& a, hipStream_t stream) {
  if (a.n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(marker_track_kernel, dim3(1), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
