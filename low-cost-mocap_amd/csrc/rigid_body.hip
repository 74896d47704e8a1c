// rigid_body.hip -- 6-DoF poses of user-defined marker sets among a frame's 3-D points (include/mocap_core.h, "rigid bodies").
//
// One WAVE per frame, lane = point (a frame holds at most 64 points, a wave has 64 lanes); every lane keeps its point in
// registers.  Several waves per workgroup each take their own frame; they share nothing, so the kernel has no barrier.  The
// bodies of a frame are taken in index order by the same wave, because a found body removes its points from the later ones.
//
// The search for one (frame, body) is a depth-first walk over the markers m = 0 .. N-1 whose control flow is wave-uniform
// (scalar branches over 64-bit masks):
//   - when marker i is put on point p, every lane computes its own distance to p once (dv[i][lane]: one broadcast of p by
//     v_readlane, one distance per lane); the entry at index q is D(p, q), the number the gate and the score need for the pair
//     (i, m) when marker m goes to q -- read back, never recomputed
//   - the candidates of marker m are one 64-bit mask: the free points, ANDed with one __ballot(|dv[i] - d_im| < tol) per
//     assigned marker i < m.  No K x K table
//   - the walk takes the set bits in ascending order, then the "marker m unassigned" branch
//   - a complete tuple is scored by summing the stored (D - d_ij)^2 in (i, j) lexicographic order and compared with the
//     best so far on the whole key (-count, score, tuple): the winner is the optimum over the search space, whatever the
//     order of the walk
//   - the only pruning beyond the gates is "this branch cannot reach the task's own best count" -- exact, and a function of
//     the task's input alone, like the number of gate-passing extensions the work cap counts
// Only what is indexed by the level and differs per lane (dv) and the per-level candidate masks live in LDS, 4.2 KB per wave;
// the rest of the walk's state is scalar (see RbWaveState).  A first version kept all of it in LDS: every node then paid some
// thirty dependent LDS round trips (44 ms per 100 000 bench frames with two bodies, 0.25 ms added to a live call); one
// before that, with a template instantiation per level and everything in registers, compiled to 512 VGPRs and 2.2 KB of scratch.
// The pose of the winner (centroids, cross-covariance, Horn's 4 x 4 matrix, cyclic Jacobi, quaternion -> R, t, rms) is a few
// hundred wave-uniform operations evaluated redundantly by every lane; lane 0 stores.  FP64 throughout, no fused operations
// (-ffp-contract=off is the build's rule).
#include "kernels.hpp"

namespace mocap {
namespace {

constexpr int kRbWaves = 4;  // waves (= frames in flight) per workgroup

// v of lane `lane` (wave-uniform) in every lane
__device__ __forceinline__ double rb_bcast(double v, int lane) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffull), lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// orders a wave's LDS stores before its later LDS loads of other lanes' entries for the compiler (no instruction: the hardware
// executes a wave's LDS accesses in order)
__device__ __forceinline__ void rb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int rb_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long rb_uni(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v & 0xffffffffull));
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double rb_uni(double v) { return __longlong_as_double((long long)rb_uni((unsigned long long)__double_as_longlong(v))); }

// The walk's state.  What is indexed by the level AND per lane -- dv -- and the per-level candidate masks live in one record
// per wave in LDS (a wave's LDS accesses are executed in order, no barrier is involved).  Everything else is kept where a
// dependent LDS round trip per access would otherwise set the pace of the walk: the partial tuple is eight bytes of one
// scalar register, the assigned markers and their points are two masks, the model distances and the score terms sit one per
// lane in two vector registers and are read with v_readlane.
struct RbWaveState {
  double dv[kRbMaxMarkers][64];            // D(the lane's point, the point of marker i)
  unsigned long long cand[kRbMaxMarkers];  // per level: candidates not yet taken
};

struct RbBest {
  int bc;                  // count, score, tuple (one byte per marker, a + 1, marker 0 in the top byte) of the best so far
  double bs;
  unsigned long long bt;
  bool capped;
};

__device__ __forceinline__ RbBest rb_search(RbWaveState& w, const double x, const double y, const double z, const int lane, const int N,
                                            const double tol, const double dl /* d[lane], lane < 28 */, const unsigned long long posable[4],
                                            const unsigned long long unclaimed, const long long cap) {
  RbBest r;
  r.bc = 0;
  r.bs = __longlong_as_double(0x7ff0000000000000ll);
  r.bt = ~0ull;
  r.capped = false;
  long long work = 0;
  // byte m of tupb: 0 = marker m unassigned, q + 1 = on point q, 0xff = level entered, nothing decided yet
  unsigned long long tupb = 0, used = 0;  // used: the points of the markers above the current level
  unsigned sub = 0;                       // ... and those markers
  double e2v = 0.0;                       // lane rb_pair(i, j): (D - d_ij)^2 of the pair as last assigned
  int m = 0;
  bool enter = true;
  while (m >= 0) {
    unsigned long long cand;
    if (enter) {
      enter = false;
      const int c = __popc(sub);
      if (m == N) {  // a complete tuple: whole key against the best so far
        if (c >= 3 && c >= r.bc && ((posable[sub >> 6] >> (sub & 63)) & 1ull)) {
          unsigned long long tup = 0;
          for (int i = 0; i < kRbMaxMarkers; i++) tup = (tup << 8) | (i < N ? (tupb >> (8 * i)) & 0xffull : 0ull);
          double sc = 0.0;
          for (int i = 0; i < N; i++)
            for (int j = i + 1; j < N; j++)
              if ((sub >> i & 1u) && (sub >> j & 1u)) sc = sc + rb_bcast(e2v, rb_pair(i, j));
          if (c > r.bc || sc < r.bs || (sc == r.bs && tup < r.bt)) {  // (c == bc from the second test on)
            r.bc = c;
            r.bs = sc;
            r.bt = tup;
          }
        }
        m--;
        continue;
      }
      const int left = N - m;
      if (c + left < 3 || c + left < r.bc) {  // cannot reach three markers / the task's own best count
        m--;
        continue;
      }
      cand = unclaimed & ~used;
      double dvi[kRbMaxMarkers - 1];
#pragma unroll
      for (int i = 0; i < kRbMaxMarkers - 1; i++) dvi[i] = w.dv[i][lane];  // (rows >= m hold old values: not used)
#pragma unroll
      for (int i = 0; i < kRbMaxMarkers - 1; i++)
        if (i < m && (sub >> i & 1u)) cand &= __ballot(fabs(dvi[i] - rb_bcast(dl, rb_pair(i, m))) < tol);
      tupb |= 0xffull << (8 * m);
    } else {  // back at level m: take its current choice out of the masks
      cand = rb_uni(w.cand[m]);
      const unsigned b = (unsigned)(tupb >> (8 * m)) & 0xffu;
      if (b != 0 && b != 0xffu) {
        used &= ~(1ull << (b - 1));
        sub &= ~(1u << m);
      }
    }
    if (cand) {
      const int q = __builtin_ctzll(cand);
      w.cand[m] = cand & (cand - 1);
      work++;
      if (work > cap) {
        r.capped = true;
        break;
      }
      tupb = (tupb & ~(0xffull << (8 * m))) | ((unsigned long long)(q + 1) << (8 * m));
      double dvq[kRbMaxMarkers - 1];
#pragma unroll
      for (int i = 0; i < kRbMaxMarkers - 1; i++) dvq[i] = w.dv[i][q];
#pragma unroll
      for (int i = 0; i < kRbMaxMarkers - 1; i++)
        if (i < m) {  // (the term of an unassigned marker i is never read)
          const double e = dvq[i] - rb_bcast(dl, rb_pair(i, m));
          e2v = lane == rb_pair(i, m) ? e * e : e2v;
        }
      const double dx = x - rb_bcast(x, q), dy = y - rb_bcast(y, q), dz = z - rb_bcast(z, q);
      w.dv[m][lane] = sqrt((dx * dx + dy * dy) + dz * dz);
      rb_wave_sync();
      used |= 1ull << q;
      sub |= 1u << m;
      m++;
      enter = true;
    } else if ((tupb >> (8 * m)) & 0xffull) {  // candidates exhausted: marker m unassigned
      w.cand[m] = 0;
      tupb &= ~(0xffull << (8 * m));
      m++;
      enter = true;
    } else {
      m--;
    }
  }
  return r;
}

// cyclic Jacobi on a symmetric 4 x 4 matrix: A -> diagonal, V = the rotations' product (columns = eigenvectors).  Every
// rotation annihilates one off-diagonal pair exactly as stated; an entry that no longer changes either of its diagonal
// neighbours is set to zero instead (the classical rule: it compares with the diagonal, not with a gap).  Quadratic
// convergence: the off-diagonal sum reaches exactly 0 within a dozen sweeps, 40 is a cap that is never reached.
__device__ __forceinline__ void rb_jacobi4(double A[4][4], double V[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; sweep++) {
    const double off = ((((fabs(A[0][1]) + fabs(A[0][2])) + fabs(A[0][3])) + fabs(A[1][2])) + fabs(A[1][3])) + fabs(A[2][3]);
    if (off == 0.0) break;
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double g = 100.0 * fabs(apq);
        if (sweep > 3 && fabs(A[p][p]) + g == fabs(A[p][p]) && fabs(A[q][q]) + g == fabs(A[q][q])) {
          A[p][q] = A[q][p] = 0.0;
          continue;
        }
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        t = theta < 0.0 ? -t : t;
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
        A[p][p] = A[p][p] - t * apq;
        A[q][q] = A[q][q] + t * apq;
        A[p][q] = A[q][p] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (k != p && k != q) {
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = A[p][k] = cs * akp - sn * akq;
            A[k][q] = A[q][k] = sn * akp + cs * akq;
          }
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = cs * vkp - sn * vkq;
          V[k][q] = sn * vkp + cs * vkq;
        }
      }
  }
}

// Four waves per SIMD (128 VGPRs): the walk is a chain of dependent LDS reads, cross-lane reads and scalar branches, so what
// sets a batch's time is how many frames are in flight.  The pose arithmetic does not fit 128 registers and spills 552 B of
// scratch -- once per found body, outside the walk.  Measured per 100 000 bench frames with two planted bodies: 34.8 ms
// uncapped (272 VGPRs, one wave per SIMD), 18.3 ms at two waves per SIMD, 11.1 ms at four; the live call is the same in all three.
__global__ __launch_bounds__(64 * kRbWaves) __attribute__((amdgpu_waves_per_eu(4, 4))) void rigid_body_kernel(RigidBodyArgs a) {
  __shared__ RbWaveState sh[kRbWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int64_t f = (int64_t)blockIdx.x * kRbWaves + wave; f < a.n_frames; f += (int64_t)gridDim.x * kRbWaves) {
    int n = a.n_pts[f];
    n = (n < 0 || n > a.K_max) ? 0 : n;  // the "no valid slot" rule of mocap_locate_objects (K_max <= 64: checked by the host)
    RbWaveState& w = sh[wave];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double* gP = a.xyz + ((size_t)f * a.K_max + (size_t)lane) * 3;
    const double px = lane < n ? gP[0] : nan;  // a point that is not there passes no gate
    const double py = lane < n ? gP[1] : nan;
    const double pz = lane < n ? gP[2] : nan;
    unsigned long long unclaimed = __ballot(lane < n);
    for (int b = 0; b < a.B; b++) {
      const RigidBodyModel* mdl = a.models + b;
      const int N = mdl->n;
      const double dl = mdl->d[lane < kRbPairs ? lane : 0];
      const unsigned long long posable[4] = {mdl->posable[0], mdl->posable[1], mdl->posable[2], mdl->posable[3]};
      const RbBest s = rb_search(w, px, py, pz, lane, N, a.tol, dl, posable, unclaimed, a.work_cap);
      rb_wave_sync();

      int found = 0, n_used = 0, status = 0;
      int asg[kRbMaxMarkers];
      double R[9], t[3], rms = 0.0, score = 0.0;
#pragma unroll
      for (int m = 0; m < kRbMaxMarkers; m++) asg[m] = 0;
#pragma unroll
      for (int k = 0; k < 9; k++) R[k] = 0.0;
      t[0] = t[1] = t[2] = 0.0;
      if (s.capped) {
        status = RB_ST_WORK_CAP_;
      } else if (s.bc >= 3) {
        // ---- pose of the winner: centred coordinates, Horn's matrix, its dominant eigenvector
        const double inv_c = 1.0 / (double)s.bc;
        // (the assigned model points and their world points are indexed by the marker: kept in the walk's dv rows, which are free now)
        double(*mq)[3] = reinterpret_cast<double(*)[3]>(&w.dv[0][0]);
        double(*wp)[3] = reinterpret_cast<double(*)[3]>(&w.dv[1][0]);
        double qb[3] = {0, 0, 0}, pb[3] = {0, 0, 0};
        unsigned long long pts = 0;
#pragma unroll
        for (int m = 0; m < kRbMaxMarkers; m++) {
          asg[m] = (int)((s.bt >> (8 * (kRbMaxMarkers - 1 - m))) & 0xff) - 1;
          const int q = asg[m] < 0 ? 0 : asg[m];
          wp[m][0] = rb_bcast(px, q);
          wp[m][1] = rb_bcast(py, q);
          wp[m][2] = rb_bcast(pz, q);
          if (asg[m] >= 0) {
            pts |= 1ull << q;
#pragma unroll
            for (int k = 0; k < 3; k++) {
              mq[m][k] = mdl->q[m][k];
              qb[k] = qb[k] + mq[m][k];
              pb[k] = pb[k] + wp[m][k];
            }
          } else {
#pragma unroll
            for (int k = 0; k < 3; k++) mq[m][k] = 0.0;
          }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
          qb[k] = qb[k] * inv_c;
          pb[k] = pb[k] * inv_c;
        }
        double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // S[i][j] = sum (q - qb)_i (p - pb)_j
#pragma unroll
        for (int m = 0; m < kRbMaxMarkers; m++)
          if (asg[m] >= 0) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
              mq[m][k] = mq[m][k] - qb[k];
              wp[m][k] = wp[m][k] - pb[k];
            }
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
              for (int j = 0; j < 3; j++) S[i][j] = S[i][j] + mq[m][i] * wp[m][j];
          }
        double A[4][4], V[4][4];
        A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
        A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
        A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
        A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
        A[0][1] = A[1][0] = S[1][2] - S[2][1];
        A[0][2] = A[2][0] = S[2][0] - S[0][2];
        A[0][3] = A[3][0] = S[0][1] - S[1][0];
        A[1][2] = A[2][1] = S[0][1] + S[1][0];
        A[1][3] = A[3][1] = S[2][0] + S[0][2];
        A[2][3] = A[3][2] = S[1][2] + S[2][1];
        rb_jacobi4(A, V);
        double lam = A[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
#pragma unroll
        for (int k = 1; k < 4; k++)
          if (A[k][k] > lam) {
            lam = A[k][k];
            qw = V[0][k];
            qx = V[1][k];
            qy = V[2][k];
            qz = V[3][k];
          }
        const double qn = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
        qw = qw / qn;
        qx = qx / qn;
        qy = qy / qn;
        qz = qz / qn;
        R[0] = ((qw * qw + qx * qx) - qy * qy) - qz * qz;
        R[1] = 2.0 * (qx * qy - qw * qz);
        R[2] = 2.0 * (qx * qz + qw * qy);
        R[3] = 2.0 * (qx * qy + qw * qz);
        R[4] = ((qw * qw - qx * qx) + qy * qy) - qz * qz;
        R[5] = 2.0 * (qy * qz - qw * qx);
        R[6] = 2.0 * (qx * qz - qw * qy);
        R[7] = 2.0 * (qy * qz + qw * qx);
        R[8] = ((qw * qw - qx * qx) - qy * qy) + qz * qz;
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = pb[i] - ((R[3 * i] * qb[0] + R[3 * i + 1] * qb[1]) + R[3 * i + 2] * qb[2]);
        // residuals in centred coordinates: R q_i + t - p_i = R (q_i - qb) - (p_i - pb)
        double ss = 0.0;
#pragma unroll
        for (int m = 0; m < kRbMaxMarkers; m++)
          if (asg[m] >= 0) {
#pragma unroll
            for (int i = 0; i < 3; i++) {
              const double r = ((R[3 * i] * mq[m][0] + R[3 * i + 1] * mq[m][1]) + R[3 * i + 2] * mq[m][2]) - wp[m][i];
              ss = ss + r * r;
            }
          }
        rms = sqrt(ss * inv_c);
        if (rms > a.max_rms) {
          status = RB_ST_RMS_;
        } else {
          found = 1;
          n_used = s.bc;
          score = s.bs;
          unclaimed &= ~pts;
        }
      }
      if (lane == 0) {
        const size_t o = (size_t)f * a.B_max + b;
        a.found[o] = found;
        a.n_used[o] = n_used;
        a.status[o] = status;
        a.rms[o] = found ? rms : 0.0;
        a.score[o] = score;
#pragma unroll
        for (int m = 0; m < kRbMaxMarkers; m++) a.assign[o * kRbMaxMarkers + m] = (int8_t)(found ? asg[m] : 0);
#pragma unroll
        for (int k = 0; k < 9; k++) a.R[o * 9 + k] = found ? R[k] : 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) a.t[o * 3 + k] = found ? t[k] : 0.0;
      }
    }
    // body slots beyond the registered bodies: zero-filled
    for (int b = a.B + lane; b < a.B_max; b += 64) {
      const size_t o = (size_t)f * a.B_max + b;
      a.found[o] = 0;
      a.n_used[o] = 0;
      a.status[o] = 0;
      a.rms[o] = 0.0;
      a.score[o] = 0.0;
      for (int m = 0; m < kRbMaxMarkers; m++) a.assign[o * kRbMaxMarkers + m] = 0;
      for (int k = 0; k < 9; k++) a.R[o * 9 + k] = 0.0;
      for (int k = 0; k < 3; k++) a.t[o * 3 + k] = 0.0;
    }
  }
}

}  // namespace

hipError_t launch_rigid_bodies(const RigidBodyArgs& a, hipStream_t stream) {
  if (a.n_frames <= 0 || a.B_max <= 0) return hipSuccess;
  int64_t blocks = (a.n_frames + kRbWaves - 1) / kRbWaves;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(rigid_body_kernel, dim3((unsigned)blocks), dim3(64 * kRbWaves), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
