// jacobi6.hpp -- cyclic Jacobi on a symmetric 6 x 6 matrix, by the rules include/mocap_core.h spells out for Horn's 4 x 4 matrix
// (csrc/rb_pose.hpp, rb_jacobi4) with the index running 0 .. 5 and the 15 pairs in lexicographic order: the skip rule, the
// g = 100 |A_pq| rule from the fifth sweep, the rotation formulae, V from the identity.  Every loop over p, q, k has constant
// bounds and is unrolled, so A and V are registers; the sweep loop is not.  kJacobi6Sweeps is the contract's limit ("joints"):
// the joint fit's matrices [[I, -R], [-R^T, I]] reach off == 0 within 9 sweeps on every input of the tests (asserted there on the
// statement), and a matrix with a NaN in it runs to the limit and is SINGULAR whatever the limit is.  Device code only.
#pragma once
#include "kernels.hpp"

namespace mocap {

constexpr int kJacobi6Sweeps = 30;

__device__ __forceinline__ void jacobi6(double (&A)[6][6], double (&V)[6][6]) {
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < 6; j++) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < kJacobi6Sweeps; sweep++) {
    double off = 0.0;
    bool first = true;
#pragma unroll
    for (int p = 0; p < 5; p++)
#pragma unroll
      for (int q = p + 1; q < 6; q++) {
        off = first ? fabs(A[p][q]) : off + fabs(A[p][q]);
        first = false;
      }
    if (off == 0.0) break;
#pragma unroll
    for (int p = 0; p < 5; p++)
#pragma unroll
      for (int q = p + 1; q < 6; q++) {
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
        for (int k = 0; k < 6; k++) {
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

}  // namespace mocap
