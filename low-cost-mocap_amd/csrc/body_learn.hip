// body_learn.hip -- a rigid body's marker set learned from a resident capture (include/mocap_core.h, "rigid-body learning"):
// xyz [F][K_max][3], n_pts [F] as the frame path leaves them, id [F][K_max] as the marker tracker leaves them, read in place.
//   gather   per frame the slot each selected marker is present at (8 bytes per frame, kept for the later passes); the valid
//            frames, the lowest complete frame, and per marker pair the count and the sum of the distances
//   spread   the second pass of the pair statistics, sum (D - d_ij)^2 with d_ij known
//   round    the frame posed against the template on its present subset (centroids, cross-covariance and residual as rb_pose()
//            has them, operation for operation, with one lane per frame instead of one wave; Horn's matrix, the Jacobi sweep, the
//            top eigenvector and quaternion -> R are rb_pose.hpp's functions), its markers mapped back, summed per marker
// and behind each a final launch of one wave that folds the workgroups' partials and writes what the next launch reads: the
// template of the next round never visits the host.
//
// Determinism: the tree of calib_tail.hip (csrc/tree_fold.hpp).  One lane per frame, kCalibThreads frames per workgroup, lane -> wave by __shfl_down
// (offsets 32 .. 1), wave -> workgroup through LDS in wave order, one partial per workgroup into the slab, one wave whose lane l
// folds the entries [l * ceil(P / 64), ...) in index order before the same shuffle tree.  No atomics: every value is a function of
// the inputs and F alone.  FP64 throughout, nothing fused (-ffp-contract=off is the build's rule).
//
// Cost: FP64 VALU work per frame is a few thousand operations per round (a dozen Jacobi sweeps at most), but the kernels are
// launch- and latency-bound like the calibration tail: a lane reads its own frame's id row and a handful of 24-byte points,
// neighbouring lanes are 4 * K_max / 24 * K_max bytes apart.  One workgroup of 256 lanes may take up to 512 VGPRs per lane;
// occupancy is not what limits a grid of ceil(F / 256) workgroups.
#include "body_learn.hpp"
#include "mocap_device.hpp"
#include "rb_pose.hpp"
#include "tree_fold.hpp"

namespace mocap {

namespace {

constexpr int kT = kCalibThreads, kWaves = kCalibThreads / 64, kM = kRbMaxMarkers;
constexpr int kLbNoRef = 1, kLbMarkerUnseen = 2;  // mirrored from include/mocap_core.h (MOCAP_LB_ST_*)

__device__ __forceinline__ bool finite3(const double* p) {
  return fabs(p[0]) < __builtin_inf() && fabs(p[1]) < __builtin_inf() && fabs(p[2]) < __builtin_inf();  // false for NaN
}

// D(p, q) of the rigid-body section
__device__ __forceinline__ double dist3(const double* p, const double* q) {
  const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

__device__ __forceinline__ int slot_of(unsigned long long w, int m) { return (int)(signed char)((w >> (8 * m)) & 0xff); }

// the present markers' points of frame f (absent: zeros); -> the number present among the first N
__device__ __forceinline__ int load_present(const BodyLearnArgs& a, int64_t f, double (&p)[kM][3], bool (&has)[kM]) {
  const unsigned long long w = *(const unsigned long long*)(a.slot + (size_t)f * kM);
  const double* P = a.xyz + (size_t)f * a.K_max * 3;
  int cnt = 0;
#pragma unroll
  for (int m = 0; m < kM; m++) {
    const int j = slot_of(w, m);
    has[m] = m < a.N && j >= 0;
    cnt += has[m] ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 3; k++) p[m][k] = has[m] ? P[3 * j + k] : 0.0;
  }
  return cnt;
}

// ------------------------------------------------------------------------------------------------------------------ gather
__global__ __launch_bounds__(kT) void lb_gather_kernel(BodyLearnArgs a) {
  __shared__ double s_part[kWaves][kLbGatherSlab];
  const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
  double v[kLbGatherSlab];
#pragma unroll
  for (int i = 0; i < kLbGatherSlab; i++) v[i] = 0.0;
  v[1] = (double)a.n_frames;  // "no complete frame here"
  if (f < a.n_frames) {
    int n = a.n_pts[f];
    const bool valid = !(a.status && a.status[f] != 0) && n >= 0 && n <= a.K_max;
    int slot[kM];
#pragma unroll
    for (int m = 0; m < kM; m++) slot[m] = -1;
    const double* P = a.xyz + (size_t)f * a.K_max * 3;
    if (valid) {
      v[0] = 1.0;
      const int32_t* ids = a.id + (size_t)f * a.K_max;
      for (int j = 0; j < n; j++) {
        const int32_t idj = ids[j];
#pragma unroll
        for (int m = 0; m < kM; m++)
          if (m < a.N && slot[m] < 0 && idj == a.sel[m] && finite3(P + 3 * j)) slot[m] = j;  // the lowest such slot
      }
    }
    unsigned long long w = 0;
    bool complete = true;
#pragma unroll
    for (int m = 0; m < kM; m++) {
      w |= (unsigned long long)(unsigned char)(signed char)slot[m] << (8 * m);
      if (m < a.N && slot[m] < 0) complete = false;
    }
    *(unsigned long long*)(a.slot + (size_t)f * kM) = w;
    if (valid && complete) v[1] = (double)f;
#pragma unroll
    for (int i = 0; i < kM; i++)
#pragma unroll
      for (int j = i + 1; j < kM; j++)
        if (slot[i] >= 0 && slot[j] >= 0) {
          v[2 + rb_pair(i, j)] = 1.0;
          v[2 + kRbPairs + rb_pair(i, j)] = dist3(P + 3 * slot[i], P + 3 * slot[j]);
        }
  }
  block_fold<kLbGatherSlab, 1>(v, s_part, a.slab + (size_t)blockIdx.x * kLbGatherSlab);
}

// one wave: the reference frame, the template Q0, d_ij; or "no reference frame"
__global__ __launch_bounds__(64) void lb_gather_final_kernel(BodyLearnArgs a, int64_t P) {
  double v[kLbGatherSlab];
  slab_fold<kLbGatherSlab, 1>(a.slab, P, (double)a.n_frames, v);
  if (threadIdx.x != 0) return;
  double* res = a.result;
  for (int i = 0; i < kLbResult; i++) res[i] = 0.0;
  int64_t ref = a.ref_frame >= 0 ? a.ref_frame : (v[1] < (double)a.n_frames ? (int64_t)v[1] : -1);
  int slot[kM];
  if (ref >= 0) {
    const unsigned long long w = *(const unsigned long long*)(a.slot + (size_t)ref * kM);
    for (int m = 0; m < kM; m++) {
      slot[m] = slot_of(w, m);
      if (m < a.N && slot[m] < 0) ref = -1;  // the given frame is not valid and complete
    }
  }
  BodyLearnState* st = a.state;
  st->flags = 0;
  for (int m = 0; m < kM; m++)
    for (int k = 0; k < 3; k++) st->Q[m][k] = 0.0;
  if (ref < 0) {
    st->no_ref = 1;
    res[126] = -1.0;
    res[128] = (double)kLbNoRef;
    return;
  }
  st->no_ref = 0;
  const double* Pr = a.xyz + (size_t)ref * a.K_max * 3;
  const double inv_n = 1.0 / (double)a.N;
  double c[3] = {0.0, 0.0, 0.0};
  for (int m = 0; m < a.N; m++)
    for (int k = 0; k < 3; k++) c[k] = c[k] + Pr[3 * slot[m] + k];
  for (int k = 0; k < 3; k++) c[k] = c[k] * inv_n;
  for (int m = 0; m < a.N; m++)
    for (int k = 0; k < 3; k++) st->Q[m][k] = Pr[3 * slot[m] + k] - c[k];
  for (int i = 0; i < kRbPairs; i++) {
    const double cnt = v[2 + i], d = cnt > 0.0 ? v[2 + kRbPairs + i] / cnt : 0.0;
    st->d[i] = d;
    res[40 + i] = d;
    res[96 + i] = cnt;
  }
  res[125] = v[0];
  res[126] = (double)ref;
}

// ------------------------------------------------------------------------------------------------------------------ spread
__global__ __launch_bounds__(kT) void lb_spread_kernel(BodyLearnArgs a) {
  __shared__ double s_part[kWaves][kLbSpreadSlab];
  if (a.state->no_ref) return;
  const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
  double v[kLbSpreadSlab];
#pragma unroll
  for (int i = 0; i < kLbSpreadSlab; i++) v[i] = 0.0;
  if (f < a.n_frames) {
    double p[kM][3];
    bool has[kM];
    if (load_present(a, f, p, has) >= 2) {
#pragma unroll
      for (int i = 0; i < kM; i++)
#pragma unroll
        for (int j = i + 1; j < kM; j++)
          if (has[i] && has[j]) {
            const double e = dist3(p[i], p[j]) - a.state->d[rb_pair(i, j)];
            v[rb_pair(i, j)] = e * e;
          }
    }
  }
  block_fold<kLbSpreadSlab, -1>(v, s_part, a.slab + (size_t)blockIdx.x * kLbSpreadSlab);
}

__global__ __launch_bounds__(64) void lb_spread_final_kernel(BodyLearnArgs a, int64_t P) {
  if (a.state->no_ref) return;
  double v[kLbSpreadSlab];
  slab_fold<kLbSpreadSlab, -1>(a.slab, P, 0.0, v);
  if (threadIdx.x != 0) return;
  for (int i = 0; i < kRbPairs; i++) {
    const double cnt = a.result[96 + i];
    a.result[68 + i] = cnt > 0.0 ? sqrt(v[i] / cnt) : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------------------------- round
__global__ __launch_bounds__(kT) void lb_round_kernel(BodyLearnArgs a) {
  __shared__ double s_part[kWaves][kLbRoundSlab];
  if (a.state->no_ref) return;
  const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
  double v[kLbRoundSlab];
#pragma unroll
  for (int i = 0; i < kLbRoundSlab; i++) v[i] = 0.0;
  if (f < a.n_frames) {
    double p[kM][3];
    bool has[kM];
    const int count = load_present(a, f, p, has);
    if (count >= 3) {
      double Q[kM][3];  // wave-uniform
#pragma unroll
      for (int m = 0; m < kM; m++)
#pragma unroll
        for (int k = 0; k < 3; k++) Q[m][k] = a.state->Q[m][k];
      // the pose of rb_pose() on the present subset, operation for operation
      const double inv_c = 1.0 / (double)count;
      double qb[3] = {0, 0, 0}, pb[3] = {0, 0, 0};
#pragma unroll
      for (int m = 0; m < kM; m++)
        if (has[m]) {
#pragma unroll
          for (int k = 0; k < 3; k++) {
            qb[k] = qb[k] + Q[m][k];
            pb[k] = pb[k] + p[m][k];
          }
        }
#pragma unroll
      for (int k = 0; k < 3; k++) {
        qb[k] = qb[k] * inv_c;
        pb[k] = pb[k] * inv_c;
      }
      double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
      for (int m = 0; m < kM; m++)
        if (has[m]) {
          double mq[3], wp[3];
#pragma unroll
          for (int k = 0; k < 3; k++) {
            mq[k] = Q[m][k] - qb[k];
            wp[k] = p[m][k] - pb[k];
          }
#pragma unroll
          for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) S[i][j] = S[i][j] + mq[i] * wp[j];
        }
      double A[4][4], V[4][4];
      rb_horn_matrix(S, A);
      rb_jacobi4(A, V);
      double qw, qx, qy, qz;
      rb_top_quat(A, V, qw, qx, qy, qz);
      double R[9], t[3];
      rb_quat_to_R(qw, qx, qy, qz, R);
#pragma unroll
      for (int i = 0; i < 3; i++) t[i] = pb[i] - ((R[3 * i] * qb[0] + R[3 * i + 1] * qb[1]) + R[3 * i + 2] * qb[2]);
      double ss = 0.0;
#pragma unroll
      for (int m = 0; m < kM; m++)
        if (has[m]) {
#pragma unroll
          for (int i = 0; i < 3; i++) {
            const double r = ((R[3 * i] * (Q[m][0] - qb[0]) + R[3 * i + 1] * (Q[m][1] - qb[1])) + R[3 * i + 2] * (Q[m][2] - qb[2])) -
                             (p[m][i] - pb[i]);
            ss = ss + r * r;
          }
        }
      const double rms = sqrt(ss * inv_c);
      if (rms <= a.max_rms) {  // the frame is used
        v[5 * kM] = 1.0;
        v[5 * kM + 1] = rms * rms;
#pragma unroll
        for (int m = 0; m < kM; m++)
          if (has[m]) {
            const double d0 = p[m][0] - t[0], d1 = p[m][1] - t[1], d2 = p[m][2] - t[2];
            double e2 = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
              const double y = (R[k] * d0 + R[3 + k] * d1) + R[6 + k] * d2;  // row k of R^T
              const double e = y - Q[m][k];
              v[5 * m + k] = y;
              e2 = k == 0 ? e * e : e2 + e * e;
            }
            v[5 * m + 3] = 1.0;
            v[5 * m + 4] = e2;
          }
      }
    }
  }
  block_fold<kLbRoundSlab, -1>(v, s_part, a.slab + (size_t)blockIdx.x * kLbRoundSlab);
}

// one wave: the template of the next round into the state, the round's figures into the result (the last round's stay)
__global__ __launch_bounds__(64) void lb_round_final_kernel(BodyLearnArgs a, int64_t P) {
  if (a.state->no_ref) return;
  double v[kLbRoundSlab];
  slab_fold<kLbRoundSlab, -1>(a.slab, P, 0.0, v);
  if (threadIdx.x != 0) return;
  BodyLearnState* st = a.state;
  double* res = a.result;
  double Qn[kM][3], c[3] = {0.0, 0.0, 0.0};
  int flags = st->flags;
  for (int m = 0; m < a.N; m++) {
    const double cnt = v[5 * m + 3];
    for (int k = 0; k < 3; k++) Qn[m][k] = cnt > 0.0 ? v[5 * m + k] / cnt : st->Q[m][k];
    if (!(cnt > 0.0)) flags |= kLbMarkerUnseen;
    res[24 + m] = cnt > 0.0 ? sqrt(v[5 * m + 4] / cnt) : 0.0;
    res[32 + m] = cnt;
    for (int k = 0; k < 3; k++) c[k] = c[k] + Qn[m][k];
  }
  const double inv_n = 1.0 / (double)a.N;
  for (int k = 0; k < 3; k++) c[k] = c[k] * inv_n;
  for (int m = 0; m < a.N; m++)
    for (int k = 0; k < 3; k++) {
      const double q = Qn[m][k] - c[k];
      st->Q[m][k] = q;
      res[3 * m + k] = q;
    }
  st->flags = flags;
  const double used = v[5 * kM];
  res[124] = used;
  res[127] = used > 0.0 ? sqrt(v[5 * kM + 1] / used) : 0.0;
  res[128] = (double)flags;
}

}  // namespace

hipError_t launch_body_learn(const BodyLearnArgs& a, int iters, hipStream_t stream) {
  const int64_t P = calib_partials(a.n_frames);
  const dim3 grid((unsigned)P), block(kT), one(1), wave(64);
  hipError_t e;
  hipLaunchKernelGGL(lb_gather_kernel, grid, block, 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(lb_gather_final_kernel, one, wave, 0, stream, a, P);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(lb_spread_kernel, grid, block, 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(lb_spread_final_kernel, one, wave, 0, stream, a, P);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (int r = 0; r < iters; r++) {
    hipLaunchKernelGGL(lb_round_kernel, grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(lb_round_final_kernel, one, wave, 0, stream, a, P);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mocap
