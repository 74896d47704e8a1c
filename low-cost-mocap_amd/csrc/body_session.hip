// body_session.hip -- a session's rigid bodies as 6-DoF series (include/mocap_core.h, "body trajectories").
//   put      the host's body table into device memory: a chunk of 8 bodies per launch travels as a kernel argument, so a "_dev" call
//            needs neither a host buffer that outlives it nor a wait.
//   pose     one lane per (body, frame), grid ceil(F / 256) x B, frames along the lanes: the 24-byte samples of a row lie side by
//            side.  The body -- rows, model, posable mask -- is the same for the whole workgroup: scalar loads.  The present markers'
//            points are read three times (centroid, cross-covariance, residual) instead of being kept: 48 doubles less beside the
//            64 of A and V, which is what keeps the kernel out of scratch.  Centroids, cross-covariance and
//            residual are rb_pose()'s operation for operation, with the points taken from the rows; Horn's matrix, the Jacobi sweep,
//            the top eigenvector and quaternion -> R are rb_pose.hpp's own functions.
//   sign     the previous POSED frame of every frame as a prefix maximum (the tile's last POSED frame from the pose kernel, one
//            workgroup per body over the tiles, then within the tile), the flip against it, and the flips' prefix parity the same
//            way: four small launches behind the pose kernel, no walk over frames (sign_walk.hpp, shared with "joint poses", over
//            block_scan.hpp's prefix and tile scan, the good-time launches' own).  Maximum and XOR are exact in any order.
//   smooth   track_smooth.hip's layout with four doubles per sample: 256 frames and a halo of W on either side in LDS (t, four
//            planes, one byte of bits: 13.1 KB), each lane walks its window three times.  Staging, fit and residual walk are
//            window_fit.hpp's with four channels, the marker smoother's own; this kernel keeps the n2 test between the solve and
//            the residual walk, the normalisation and omega.
//   fill     one lane per (row, frame), grid ceil(F / 256) x R; the row's (body, marker) comes from a table built on the device.
// FP64 throughout, nothing fused (-ffp-contract=off is the build's rule), / and sqrt correctly rounded.
#include "body_session.hpp"
#include "block_scan.hpp"
#include "mocap_device.hpp"
#include "rb_pose.hpp"
#include "sign_walk.hpp"
#include "window_fit.hpp"

namespace mocap {

namespace {

constexpr int kT = kTsTile;

// ------------------------------------------------------------------------------------------------------------------ body table
__global__ __launch_bounds__(64) void bp_put_kernel(BpBodyChunk c, int count, BpBody* dst) {
  constexpr int kWords = (int)(sizeof(BpBody) / sizeof(unsigned long long));
  static_assert(sizeof(BpBody) % sizeof(unsigned long long) == 0, "copied as 64-bit words");
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&c);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(dst);
  for (int i = threadIdx.x; i < count * kWords; i += 64) out[i] = src[i];
}

// ------------------------------------------------------------------------------------------------------------------ poses
__global__ __launch_bounds__(kT) void bp_pose_kernel(PoseRowsArgs a) {
  __shared__ int s_last;
  const int b = blockIdx.y, lane = threadIdx.x;
  const int64_t F = a.n_frames, f = (int64_t)blockIdx.x * kT + lane;
  if (lane == 0) s_last = -1;
  __syncthreads();
  const BpBody* __restrict__ body = a.bodies + b;
  const int N = body->n;
  bool posed = false;
  if (f < F) {
    const double nan = __builtin_nan("");
    const double* __restrict__ P = a.traj + (size_t)f * 3;
    const size_t rs = (size_t)F * 3;  // doubles per row
    double qb[3] = {0, 0, 0}, pb[3] = {0, 0, 0};
    unsigned pres = 0;
    int count = 0;
#pragma unroll
    for (int m = 0; m < kBpMaxMarkers; m++)
      if (m < N) {
        const double* p = P + (size_t)body->rows[m] * rs;
        const double x = p[0], y = p[1], z = p[2];
        if (finite1(x) && finite1(y) && finite1(z)) {
          pres |= 1u << m;
          count++;
          qb[0] = qb[0] + body->q[m][0];
          qb[1] = qb[1] + body->q[m][1];
          qb[2] = qb[2] + body->q[m][2];
          pb[0] = pb[0] + x;
          pb[1] = pb[1] + y;
          pb[2] = pb[2] + z;
        }
      }
    int flag;
    double quat[4] = {nan, nan, nan, nan}, R[9], t[3] = {nan, nan, nan}, rms = nan;
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = nan;
    if (count < 3) {
      flag = kBpFew;
    } else if (!((body->posable[pres >> 6] >> (pres & 63)) & 1ull)) {
      flag = kBpDegenerate;
    } else {
      const double inv_c = 1.0 / (double)count;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        qb[k] = qb[k] * inv_c;
        pb[k] = pb[k] * inv_c;
      }
      double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // S[i][j] = sum (q - qb)_i (p - pb)_j
#pragma unroll
      for (int m = 0; m < kBpMaxMarkers; m++)
        if (m < N && (pres >> m & 1u)) {
          const double* p = P + (size_t)body->rows[m] * rs;
          double mq[3], wp[3];
#pragma unroll
          for (int k = 0; k < 3; k++) {
            mq[k] = body->q[m][k] - qb[k];
            wp[k] = p[k] - pb[k];
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
      rb_quat_to_R(qw, qx, qy, qz, R);
#pragma unroll
      for (int i = 0; i < 3; i++) t[i] = pb[i] - ((R[3 * i] * qb[0] + R[3 * i + 1] * qb[1]) + R[3 * i + 2] * qb[2]);
      // residuals in centred coordinates: R q_i + t - p_i = R (q_i - qb) - (p_i - pb)
      double ss = 0.0;
#pragma unroll
      for (int m = 0; m < kBpMaxMarkers; m++)
        if (m < N && (pres >> m & 1u)) {
          const double* p = P + (size_t)body->rows[m] * rs;
          double mq[3];
#pragma unroll
          for (int k = 0; k < 3; k++) mq[k] = body->q[m][k] - qb[k];
#pragma unroll
          for (int i = 0; i < 3; i++) {
            const double r = ((R[3 * i] * mq[0] + R[3 * i + 1] * mq[1]) + R[3 * i + 2] * mq[2]) - (p[i] - pb[i]);
            ss = ss + r * r;
          }
        }
      rms = sqrt(ss * inv_c);
      if (rms > a.max_rms) {
        flag = kBpRms;
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = nan;
        t[0] = t[1] = t[2] = nan;
      } else {
        flag = kBpPosed;
        posed = true;
        quat[0] = qw;
        quat[1] = qx;
        quat[2] = qy;
        quat[3] = qz;
      }
    }
    const size_t o = (size_t)b * F + f;
    a.n_used[o] = count;
    a.present[o] = (int32_t)pres;
    a.flag[o] = flag;
    a.rms[o] = rms;
#pragma unroll
    for (int i = 0; i < 4; i++) a.quat[4 * o + i] = quat[i];
#pragma unroll
    for (int i = 0; i < 9; i++) a.Rm[9 * o + i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) a.t_pose[3 * o + i] = t[i];
  }
  if (posed) atomicMax(&s_last, lane);  // (an integer maximum in LDS: exact in any order)
  __syncthreads();
  if (lane == 0) a.tile_i32[(size_t)b * gridDim.x + blockIdx.x] = s_last < 0 ? -1 : (int32_t)(blockIdx.x * kT + s_last);
}

// ------------------------------------------------------------------------------------------------------------------ sign continuity
struct BpOnPosed {  // the frames that carry a quaternion (sign_walk.hpp)
  __device__ static bool on(int32_t flag) { return flag == kBpPosed; }
};

// ------------------------------------------------------------------------------------------------------------------ rotations
template <int D>
__global__ __launch_bounds__(kT) void bp_smooth_kernel(SmoothRotationsArgs a) {
  __shared__ WfStage<4> s;
  const int r = blockIdx.y;
  const int64_t F = a.n_frames, f0 = (int64_t)blockIdx.x * kT, f = f0 + threadIdx.x;
  wf_stage<4>(a, a.quat + (size_t)r * F * 4, f0, s);
  if (f >= F) return;

  const double nan = __builtin_nan("");
  const int c = threadIdx.x + a.W;  // this lane's frame among the staged ones
  double out[8];                    // quat_s, omega, res
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = nan;
  int n;
  double h, cf[D + 1][4];
  int flag = wf_fit<4, D>(a, s, c, n, h, cf);
  if (flag & (kTsSmoothed | kTsFilled)) {
    const double pw = cf[0][0], px = cf[0][1], py = cf[0][2], pz = cf[0][3];
    const double n2 = ((pw * pw + px * px) + py * py) + pz * pz;
    if (!(n2 > 0.0 && n2 < __builtin_inf())) {
      flag = kTsSingular;
    } else {
      const double ss = wf_residual<4, D>(a, s, c, h, cf);
      const double nq = sqrt(n2);
      const double dw = cf[1][0] / h, dx = cf[1][1] / h, dy = cf[1][2] / h, dz = cf[1][3] / h;
      out[0] = pw / nq;
      out[1] = px / nq;
      out[2] = py / nq;
      out[3] = pz / nq;
      out[4] = (2.0 * ((pw * dx - dw * px) - (dy * pz - dz * py))) / n2;
      out[5] = (2.0 * ((pw * dy - dw * py) - (dz * px - dx * pz))) / n2;
      out[6] = (2.0 * ((pw * dz - dw * pz) - (dx * py - dy * px))) / n2;
      out[7] = sqrt(ss / (double)(4 * n));
    }
  }
  const size_t o = (size_t)r * F + f;
#pragma unroll
  for (int k = 0; k < 4; k++) a.quat_s[4 * o + k] = out[k];
#pragma unroll
  for (int k = 0; k < 3; k++) a.omega[3 * o + k] = out[4 + k];
  a.res[o] = out[7];
  a.n_used[o] = n;
  a.flag[o] = flag;
}

// ------------------------------------------------------------------------------------------------------------------ fill
__global__ __launch_bounds__(kT) void bp_row_table_kernel(FillRowsArgs a) {  // one workgroup
  for (int r = threadIdx.x; r < a.R; r += kT) a.row_of[r] = -1;
  __syncthreads();
  for (int i = threadIdx.x; i < a.B * kBpMaxMarkers; i += kT) {
    const int b = i / kBpMaxMarkers, m = i % kBpMaxMarkers;
    if (m >= a.bodies[b].n) continue;
    const int r = a.bodies[b].rows[m];
    if (r >= 0 && r < a.R) a.row_of[r] = i;  // (the host has checked the range and that no row appears twice)
  }
}

__global__ __launch_bounds__(kT) void bp_fill_kernel(FillRowsArgs a) {
  const int r = blockIdx.y;
  const int64_t F = a.n_frames, f = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (f >= F) return;
  const size_t o = (size_t)r * F + f;
  const double nan = __builtin_nan("");
  double x[3] = {a.traj[3 * o], a.traj[3 * o + 1], a.traj[3 * o + 2]};
  int src = kBpSrcMeasured;
  if (!(finite1(x[0]) && finite1(x[1]) && finite1(x[2]))) {
    x[0] = x[1] = x[2] = nan;
    src = kBpSrcNone;
    const int bm = a.row_of[r];
    if (bm >= 0) {
      const int b = bm / kBpMaxMarkers, m = bm % kBpMaxMarkers;
      const double* q = a.bodies[b].q[m];
      const size_t p = (size_t)b * F + f;
      if (a.flag[p] == kBpPosed) {
        const double* R = a.Rm + 9 * p;
#pragma unroll
        for (int i = 0; i < 3; i++) x[i] = ((R[3 * i] * q[0] + R[3 * i + 1] * q[1]) + R[3 * i + 2] * q[2]) + a.t_pose[3 * p + i];
        src = kBpSrcRigid;
      } else if (a.flag_s && a.flag_s[p] == kTsFilled) {
        const double qw = a.quat_s[4 * p], qx = a.quat_s[4 * p + 1], qy = a.quat_s[4 * p + 2], qz = a.quat_s[4 * p + 3];
        double R[9];
        rb_quat_to_R(qw, qx, qy, qz, R);
#pragma unroll
        for (int i = 0; i < 3; i++) x[i] = ((R[3 * i] * q[0] + R[3 * i + 1] * q[1]) + R[3 * i + 2] * q[2]) + a.pos_s[3 * p + i];
        src = kBpSrcRigidFilled;
      }
    }
  }
  a.filled[3 * o] = x[0];
  a.filled[3 * o + 1] = x[1];
  a.filled[3 * o + 2] = x[2];
  a.src[o] = src;
}

}  // namespace

hipError_t launch_put_bodies(const BpBody* host, int B, BpBody* dev, hipStream_t stream) {
  for (int b0 = 0; b0 < B; b0 += kBpPutBodies) {
    BpBodyChunk c{};
    const int count = B - b0 < kBpPutBodies ? B - b0 : kBpPutBodies;
    for (int i = 0; i < count; i++) c.b[i] = host[b0 + i];
    hipLaunchKernelGGL(bp_put_kernel, dim3(1), dim3(64), 0, stream, c, count, dev + b0);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

hipError_t launch_pose_rows(const PoseRowsArgs& a, hipStream_t stream) {
  const dim3 block(kT), grid((unsigned)ts_tiles(a.n_frames), (unsigned)a.B);
  hipLaunchKernelGGL(bp_pose_kernel, grid, block, 0, stream, a);
  if (hipError_t e = hipGetLastError()) return e;
  return launch_sign_walk<BpOnPosed>(SignWalkArgs{a.n_frames, a.flag, a.quat, a.tile_i32, a.parity}, a.B, false, stream);
}

hipError_t launch_smooth_rotations(const SmoothRotationsArgs& a, hipStream_t stream) {
  const dim3 block(kT), grid((unsigned)ts_tiles(a.n_frames), (unsigned)a.B);
  if (a.degree == 1) hipLaunchKernelGGL(bp_smooth_kernel<1>, grid, block, 0, stream, a);
  else if (a.degree == 2) hipLaunchKernelGGL(bp_smooth_kernel<2>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(bp_smooth_kernel<3>, grid, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_fill_rows(const FillRowsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(bp_row_table_kernel, dim3(1), dim3(kT), 0, stream, a);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(bp_fill_kernel, dim3((unsigned)ts_tiles(a.n_frames), (unsigned)a.R), dim3(kT), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
