// body_track.hip -- the "body tracker" section of include/mocap_core.h: the registered rigid bodies followed from frame to
// frame.  Per body and frame: the pose predicted from the slot's state, the greedy association of the frame's points to the
// predicted markers (two rounds), else the per-frame search's result for the same frame (rigid_body.hip, run over the whole
// batch before this kernel), else coasting; the contract's steps 1-4 are quoted at the code that implements them.
//
// The recurrence is serial in the frames and, through the claimed points, in the bodies: ONE wave walks a call's frames (one
// workgroup of 64 lanes, no workgroup barrier inside the loop, no atomics), lane = point.  The state stays in registers across
// the frame loop -- lane b holds the slot of body b, the body at work reads it with v_readlane -- and is written back once.
// The registration (markers, posable tables) is copied into LDS once per launch.  The next frame's points, time stamp and
// search results are fetched one frame ahead: they do not depend on the state, and the chain of frames is latency-bound.
//
// Association.  Lane i (< 8) forms predicted marker i; every lane takes the eight markers by v_readlane (they are
// wave-uniform: broadcast, not re-loaded) and keeps its point's d2 to each in registers.  The contract's "admissible pairs in
// ascending (d2, marker, point), commit when both are free" is at most N commits, each the wave-wide lexicographic minimum of
// (bits(d2), i, j) over the pairs still free: d2 is finite and >= 0, so its bit pattern orders like its value.  A lane first
// takes the minimum over its own markers (ascending i, strict <), then three 32-bit minima across the wave (high word, low
// word, marker; DPP inside a row of 16, v_readlane across the four rows) and one ballot name the pair; its marker's bit is
// struck in every lane, its point's lane strikes all of its own.
//
// The pose of an assignment is rb_pose (rb_pose.hpp), the per-frame search's arithmetic operation for operation; its centred
// points sit in a small LDS block of this kernel's.  FP64 throughout, no fused operations (-ffp-contract=off is the build's rule).
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "rb_pose.hpp"

namespace mocap {

namespace {

using u64 = unsigned long long;

struct BtFrameIn {  // a frame's inputs as loaded (n is checked by the consumer)
  double t, x, y, z;  // lane j < K_max: point j
  int n;
  int found;  // lane b < B: the search's found[b]
  int asg;    // lane 8 b + m, b < B: the search's assign[b][m]
};

__device__ __forceinline__ BtFrameIn bt_load_frame(const BodyTrackArgs& a, int64_t f, int lane) {
  BtFrameIn r;
  r.t = a.t[f];
  r.n = a.n_pts[f];
  r.x = r.y = r.z = 0.0;
  if (lane < a.K_max) {  // (every slot of the buffer is readable; slots >= n are masked by the consumer)
    const double* q = a.xyz + ((size_t)f * a.K_max + lane) * 3;
    r.x = q[0];
    r.y = q[1];
    r.z = q[2];
  }
  const size_t fb = (size_t)f * a.B_max;
  r.found = lane < a.B ? a.rb_found[fb + lane] : 0;
  r.asg = lane < a.B * kRbMaxMarkers ? (int)a.rb_assign[fb * kRbMaxMarkers + lane] : -1;
  return r;
}

__device__ __forceinline__ bool bt_finite(double v) { return __builtin_isfinite(v); }
__device__ __forceinline__ int bt_lane_int(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ unsigned bt_min(unsigned a, unsigned b) { return a < b ? a : b; }

// the minimum of v over the wave's 64 lanes, in every lane (all lanes active): quad, half row and row of 16 by DPP, the four
// rows by v_readlane
__device__ __forceinline__ unsigned bt_wave_umin(unsigned v) {
  v = bt_min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xf, 0xf, false));   // quad_perm [1, 0, 3, 2]
  v = bt_min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false));   // quad_perm [2, 3, 0, 1]
  v = bt_min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xf, 0xf, false));  // row_half_mirror
  v = bt_min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xf, 0xf, false));  // row_mirror
  const unsigned r0 = (unsigned)bt_lane_int((int)v, 0), r1 = (unsigned)bt_lane_int((int)v, 16);
  const unsigned r2 = (unsigned)bt_lane_int((int)v, 32), r3 = (unsigned)bt_lane_int((int)v, 48);
  return bt_min(bt_min(r0, r1), bt_min(r2, r3));
}

// step 2 of the contract, one round: the greedy association of the free points (lane = point; `free_pt`: j < n, finite, not
// claimed) to the N markers predicted from (Rc, pc).  qm: marker (lane & 7) of the body.  -> the tuple in the search's form
// (rb_pose.hpp): one byte per marker, point + 1, 0 = unassigned, marker 0 in the top byte
__device__ __forceinline__ u64 bt_associate(const int lane, const int N, const double g2, const bool free_pt, const double x,
                                            const double y, const double z, const double qm[3], const double Rc[9],
                                            const double pc[3]) {
  // predicted marker (lane & 7): ((Rc[3r] q0 + Rc[3r+1] q1) + Rc[3r+2] q2) + pc[r]
  double mh[3];
#pragma unroll
  for (int r = 0; r < 3; r++) mh[r] = ((Rc[3 * r] * qm[0] + Rc[3 * r + 1] * qm[1]) + Rc[3 * r + 2] * qm[2]) + pc[r];
  double d2[kRbMaxMarkers];
  unsigned adm = 0;  // bit i: (marker i, this lane's point) is admissible and neither is taken
#pragma unroll
  for (int i = 0; i < kRbMaxMarkers; i++) {
    const double dx = x - rb_bcast(mh[0], i), dy = y - rb_bcast(mh[1], i), dz = z - rb_bcast(mh[2], i);
    d2[i] = (dx * dx + dy * dy) + dz * dz;
    if (i < N && free_pt && d2[i] < g2) adm |= 1u << i;  // (strict; a NaN passes no gate)
  }
  u64 tup = 0;
  for (int c = 0; c < N; c++) {
    u64 bk = ~0ull;  // the lane's own minimum over its markers: ascending i, strict <
    unsigned bi = 0xffu;
#pragma unroll
    for (int i = 0; i < kRbMaxMarkers; i++) {
      const u64 k = (u64)__double_as_longlong(d2[i]);
      if (((adm >> i) & 1u) && k < bk) {
        bk = k;
        bi = (unsigned)i;
      }
    }
    const unsigned hi = (unsigned)(bk >> 32), lo = (unsigned)(bk & 0xffffffffull);
    const unsigned m_hi = bt_wave_umin(hi);
    if (m_hi == 0xffffffffu) break;  // no admissible pair is left (the bits of a finite d2 never start with 0xffffffff)
    const unsigned m_lo = bt_wave_umin(hi == m_hi ? lo : 0xffffffffu);
    const bool tie = hi == m_hi && lo == m_lo;
    const unsigned m_i = bt_wave_umin(tie ? bi : 0xffu);
    const int j = __builtin_ctzll(__ballot(tie && bi == m_i));  // the lowest point among the pairs (d2, marker) of the minimum
    tup |= (u64)(j + 1) << (8 * (kRbMaxMarkers - 1 - m_i));
    adm &= ~(1u << m_i);
    if (lane == j) adm = 0;
  }
  return tup;
}

__device__ __forceinline__ void bt_zero_slot(const BodyTrackArgs& a, size_t o) {
  a.tracked[o] = 0;
  a.source[o] = 0;
  a.n_used[o] = 0;
  a.rms[o] = 0.0;
  a.hits[o] = 0;
  a.missed[o] = 0;
  for (int m = 0; m < kRbMaxMarkers; m++) a.assign[o * kRbMaxMarkers + m] = 0;
  for (int k = 0; k < 9; k++) a.R[o * 9 + k] = 0.0;
  for (int k = 0; k < 3; k++) a.p[o * 3 + k] = 0.0;
}

}  // namespace

__global__ __launch_bounds__(64) void body_track_kernel(BodyTrackArgs a) {
  __shared__ RigidBodyModel sM[kRbMaxBodies];      // the registration
  __shared__ double sPose[2][kRbMaxMarkers][3];    // rb_pose: the assigned model points and their world points
  static_assert(sizeof(RigidBodyModel) % 8 == 0, "copied as 64-bit words");
  const int lane = threadIdx.x;
  for (int i = lane; i < a.B * (int)(sizeof(RigidBodyModel) / 8); i += 64)
    reinterpret_cast<u64*>(sM)[i] = reinterpret_cast<const u64*>(a.models)[i];
  // lane b holds the slot of body b (the lanes from 8 on a copy of slot 0 that is never stored)
  BodyTrackState* st = a.state;
  const int sb = lane < kRbMaxBodies ? lane : 0;
  int live = st->live[sb], missed = st->missed[sb], hits = st->hits[sb];
  double sR[9], sp[3], sv[3];
#pragma unroll
  for (int k = 0; k < 9; k++) sR[k] = st->R[sb][k];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    sp[k] = st->p[sb][k];
    sv[k] = st->v[sb][k];
  }
  double t_seen = st->t_seen[sb];
  __syncthreads();

  BtFrameIn nxt = bt_load_frame(a, 0, lane);
  for (int64_t f = 0; f < a.n_frames; f++) {
    const BtFrameIn in = nxt;
    if (f + 1 < a.n_frames) nxt = bt_load_frame(a, f + 1, lane);  // (inputs do not depend on the state: one frame ahead)
    const size_t fb = (size_t)f * a.B_max;
    // body slots beyond the registered bodies: zero-filled
    for (int b = a.B + lane; b < a.B_max; b += 64) bt_zero_slot(a, fb + b);
    if (!bt_finite(in.t)) {  // uniform: outputs zero, the state untouched
      if (lane < a.B) bt_zero_slot(a, fb + lane);
      if (lane == 0) a.status[f] = BT_ST_BAD_TIME_;
      continue;
    }
    const int n = (in.n < 0 || in.n > a.K_max) ? 0 : in.n;  // the "no valid slot" rule of mocap_locate_objects
    const bool fin = lane < n && bt_finite(in.x) && bt_finite(in.y) && bt_finite(in.z);
    u64 Cl = 0;  // the points claimed so far in this frame
    for (int b = 0; b < a.B; b++) {
      const RigidBodyModel* mdl = &sM[b];
      const int N = __builtin_amdgcn_readfirstlane(mdl->n);
      const double qm[3] = {mdl->q[lane & 7][0], mdl->q[lane & 7][1], mdl->q[lane & 7][2]};
      const bool was_live = bt_lane_int(live, b) != 0;
      const int b_missed = bt_lane_int(missed, b), b_hits = bt_lane_int(hits, b);
      double bR[9], bp[3], bv[3];
#pragma unroll
      for (int k = 0; k < 9; k++) bR[k] = rb_bcast(sR[k], b);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        bp[k] = rb_bcast(sp[k], b);
        bv[k] = rb_bcast(sv[k], b);
      }
      // ---- step 1: prediction (orientation is held)
      const double dt = in.t - rb_bcast(t_seen, b);
      double ph[3] = {bp[0], bp[1], bp[2]};
      if (was_live && dt > 0.0) {
#pragma unroll
        for (int k = 0; k < 3; k++) ph[k] = bp[k] + bv[k] * dt;
      }
      // ---- steps 2-3: guided association, round 1 from the prediction and round 2 from round 1's pose; else the search's
      // assignment when none of its points is claimed.  One walk over the stages, so that the pose arithmetic stands once.
      int src = BT_SRC_NONE_, o_used = 0;
      u64 o_tup = 0, o_pts = 0;
      double oR[9], op[3], o_rms = 0.0;
#pragma unroll
      for (int k = 0; k < 9; k++) oR[k] = 0.0;
      op[0] = op[1] = op[2] = 0.0;
      double Rc[9], pc[3];
#pragma unroll
      for (int k = 0; k < 9; k++) Rc[k] = bR[k];
#pragma unroll
      for (int k = 0; k < 3; k++) pc[k] = ph[k];
      const bool free_pt = fin && !((Cl >> lane) & 1ull);
      int stage = was_live ? 0 : 2;  // 0, 1: guided rounds 1 and 2; 2: the search's result
      while (stage < 3) {
        u64 tup = 0;
        if (stage < 2) {
          tup = bt_associate(lane, N, a.g2, free_pt, in.x, in.y, in.z, qm, Rc, pc);
        } else if (bt_lane_int(in.found, b) == 1) {
#pragma unroll
          for (int m = 0; m < kRbMaxMarkers; m++) {
            const int q = bt_lane_int(in.asg, b * kRbMaxMarkers + m);
            if (m < N && q >= 0 && q < 64) tup |= (u64)(q + 1) << (8 * (kRbMaxMarkers - 1 - m));
          }
        }
        unsigned sub = 0;
        u64 pts = 0;
#pragma unroll
        for (int m = 0; m < kRbMaxMarkers; m++) {
          const int q = (int)((tup >> (8 * (kRbMaxMarkers - 1 - m))) & 0xffull) - 1;
          if (q >= 0) {
            sub |= 1u << m;
            pts |= 1ull << q;
          }
        }
        const int cnt = __popc(sub);
        // guided: the assigned subset is posable (the body's table: it has >= 3 markers then); search: found, nothing claimed
        bool ok = stage < 2 ? ((mdl->posable[sub >> 6] >> (sub & 63)) & 1ull) != 0 : (cnt >= 3 && (pts & Cl) == 0);
        double Rn[9], pn[3], rn = 0.0;
        if (ok) {
          int asg[kRbMaxMarkers];
          rb_pose(mdl, tup, asg, cnt, in.x, in.y, in.z, sPose[0], sPose[1], Rn, pn, rn);
          if (stage < 2) ok = rn <= a.max_rms;  // (the search's own fit has passed this test with the same arithmetic)
        }
        if (ok) {
          src = stage < 2 ? BT_SRC_GUIDED_ : BT_SRC_SEARCH_;
          o_used = cnt;
          o_tup = tup;
          o_pts = pts;
          o_rms = rn;
#pragma unroll
          for (int k = 0; k < 9; k++) oR[k] = Rn[k];
#pragma unroll
          for (int k = 0; k < 3; k++) op[k] = pn[k];
        }
        if (stage == 0 && ok) {  // round 2 repeats association and fit from round 1's pose; round 1's points are free again
#pragma unroll
          for (int k = 0; k < 9; k++) Rc[k] = Rn[k];
#pragma unroll
          for (int k = 0; k < 3; k++) pc[k] = pn[k];
          stage = 1;
        } else {
          stage = stage == 0 ? 2 : 3;  // round 1 failed: guided fails; round 2 or the search: done either way
        }
      }
      // ---- outcome and update
      int o_tracked = 0, o_hits = 0, o_missed = 0;
      if (src != BT_SRC_NONE_) {  // GUIDED / SEARCH
        double nv[3] = {0.0, 0.0, 0.0};
        if (was_live) {
#pragma unroll
          for (int k = 0; k < 3; k++) {
            nv[k] = bv[k];
            if (dt > 0.0) {
              const double u = (op[k] - bp[k]) / dt;
              nv[k] = bv[k] + a.vel_alpha * (u - bv[k]);
            }
          }
        }
        o_tracked = 1;
        o_hits = (was_live ? b_hits : 0) + 1;
        if (lane == b) {
#pragma unroll
          for (int k = 0; k < 9; k++) sR[k] = oR[k];
#pragma unroll
          for (int k = 0; k < 3; k++) {
            sp[k] = op[k];
            sv[k] = nv[k];
          }
          t_seen = in.t;
          missed = 0;
          hits = o_hits;
          live = 1;
        }
        Cl |= o_pts;
      } else if (was_live) {  // COAST: R, p, v and t_seen are kept, nothing is claimed
        const int mm = b_missed + 1;
        const bool retire = mm > a.max_missed;
        if (lane == b) {
          missed = mm;
          if (retire) live = 0;
        }
        if (!retire) {
          src = BT_SRC_COAST_;
          o_tracked = 1;
          o_hits = b_hits;
          o_missed = mm;
#pragma unroll
          for (int k = 0; k < 9; k++) oR[k] = bR[k];
#pragma unroll
          for (int k = 0; k < 3; k++) op[k] = ph[k];
        }
      }
      if (lane == 0) {
        const size_t o = fb + b;
        a.tracked[o] = o_tracked;
        a.source[o] = src;
        a.n_used[o] = o_used;
        a.rms[o] = o_rms;
        a.hits[o] = o_hits;
        a.missed[o] = o_missed;
#pragma unroll
        for (int m = 0; m < kRbMaxMarkers; m++)
          a.assign[o * kRbMaxMarkers + m] = (int8_t)(src == BT_SRC_NONE_ ? 0 : (int)((o_tup >> (8 * (kRbMaxMarkers - 1 - m))) & 0xffull) - 1);
#pragma unroll
        for (int k = 0; k < 9; k++) a.R[o * 9 + k] = oR[k];
#pragma unroll
        for (int k = 0; k < 3; k++) a.p[o * 3 + k] = op[k];
      }
    }
    if (lane == 0) a.status[f] = 0;
  }

  if (lane < kRbMaxBodies) {
    st->live[lane] = live;
    st->missed[lane] = missed;
    st->hits[lane] = hits;
#pragma unroll
    for (int k = 0; k < 9; k++) st->R[lane][k] = sR[k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      st->p[lane][k] = sp[k];
      st->v[lane][k] = sv[k];
    }
    st->t_seen[lane] = t_seen;
  }
}

hipError_t launch_body_tracker(const BodyTrackArgs& a, hipStream_t stream) {
  if (a.n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(body_track_kernel, dim3(1), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
