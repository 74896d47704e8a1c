// rb_pose.hpp -- the pose of an assignment (include/mocap_core.h, "rigid bodies": centroids, cross-covariance, Horn's 4 x 4
// matrix, cyclic Jacobi, quaternion -> R, t, rms in centred coordinates) as a function, for the body tracker (body_track.hip),
// and its middle as small functions -- rb_horn_matrix, rb_jacobi4, rb_top_quat, rb_quat_to_R -- for the kernels that pose one
// lane per frame from points of their own (body_learn.hip, body_session.hip).  They are separate functions on purpose: one
// function around matrix, sweep, eigenvector and R cost the session's pose kernel 14 registers (120 -> 134, across the 128
// boundary: 4 -> 3 waves per SIMD); called one after the other they cost none.
// One copy of this text remains, in the per-frame search's pose block (rigid_body.hip), Jacobi sweep included: behind a function
// boundary that kernel, tuned to 128 registers, spilled 632 instead of 552 B and ran 2 % longer (7.13 against 6.98 ms per
// 100 000 frames), and nobody has a cheaper measurement since.  The arithmetic is the same operation for operation, and the same
// operands in the same order give the same bits: the tracker's SEARCH poses are compared byte for byte with the search's own
// outputs (tests/test_gpu_body_track.py).  A few hundred wave-uniform operations evaluated redundantly by every lane.  FP64
// throughout, no fused operations (-ffp-contract=off is the build's rule).  Device code only.
#pragma once
#include "kernels.hpp"

namespace mocap {

// v of lane `lane` (wave-uniform) in every lane
__device__ __forceinline__ double rb_bcast(double v, int lane) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffull), lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
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

// Horn's matrix of the cross-covariance S[i][j] = sum (q - qb)_i (p - pb)_j: its top eigenvector is the rotation's quaternion
__device__ __forceinline__ void rb_horn_matrix(const double S[3][3], double A[4][4]) {
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
}

// the eigenvector of the largest eigenvalue as a unit quaternion: A, V as rb_jacobi4 leaves them (the first of equal eigenvalues)
__device__ __forceinline__ void rb_top_quat(const double A[4][4], const double V[4][4], double& qw, double& qx, double& qy, double& qz) {
  double lam = A[0][0];
  qw = V[0][0];
  qx = V[1][0];
  qy = V[2][0];
  qz = V[3][0];
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
}

__device__ __forceinline__ void rb_quat_to_R(const double qw, const double qx, const double qy, const double qz, double R[9]) {
  R[0] = ((qw * qw + qx * qx) - qy * qy) - qz * qz;
  R[1] = 2.0 * (qx * qy - qw * qz);
  R[2] = 2.0 * (qx * qz + qw * qy);
  R[3] = 2.0 * (qx * qy + qw * qz);
  R[4] = ((qw * qw - qx * qx) + qy * qy) - qz * qz;
  R[5] = 2.0 * (qy * qz - qw * qx);
  R[6] = 2.0 * (qx * qz - qw * qy);
  R[7] = 2.0 * (qy * qz + qw * qx);
  R[8] = ((qw * qw - qx * qx) - qy * qy) + qz * qz;
}

// The pose of the assignment `tuple` (one byte per marker, point index + 1, 0 = unassigned, marker 0 in the top byte; `count` of
// them assigned, >= 3) of body `mdl` among the wave's points (px, py, pz: lane = point).  mq, wp: two rows of [kRbMaxMarkers][3]
// doubles of the wave's own LDS -- the assigned model points and their world points, indexed by the marker.  -> asg (point index
// per marker, -1 = unassigned), R, t, rms and the mask of the assigned points.
__device__ __forceinline__ unsigned long long rb_pose(const RigidBodyModel* mdl, const unsigned long long tuple, int asg[kRbMaxMarkers], const int count,
                                                      const double px, const double py, const double pz, double (*mq)[3],
                                                      double (*wp)[3], double R[9], double t[3], double& rms) {
  const double inv_c = 1.0 / (double)count;
  double qb[3] = {0, 0, 0}, pb[3] = {0, 0, 0};
  unsigned long long pts = 0;
#pragma unroll
  for (int m = 0; m < kRbMaxMarkers; m++) {
    asg[m] = (int)((tuple >> (8 * (kRbMaxMarkers - 1 - m))) & 0xff) - 1;
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
  for (int m = 0; m < kRbMaxMarkers; m++)
    if (asg[m] >= 0) {
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const double r = ((R[3 * i] * mq[m][0] + R[3 * i + 1] * mq[m][1]) + R[3 * i + 2] * mq[m][2]) - wp[m][i];
        ss = ss + r * r;
      }
    }
  rms = sqrt(ss * inv_c);
  return pts;
}

}  // namespace mocap
