// bb_fold.hpp -- the block cache's word of csrc/frame_bb.hip: a block's bound folded into ONE float.
// Plain C++ (no intrinsics), the same text for the kernel and for a host compiler: tests/native/bb_fold_check.cpp runs it on
// the CPU against the double expression it stands for.
//
// The search drops a block of root r when (search(): dropped())
//     s1 (2e-12 tr + y) < 1,      y = p3max2c limit_adj(r) >= 0   (the root's best error so far, with its allowances)
// s1 and tr are the block's, y is the root's at the time of the test.  With a = s1 2e-12 tr < 1 this is
//     q y < 1,                    q = s1 / (1 - a)
// and q is a property of the block alone: the seed pass stores it, the test pass multiplies it with y.  The stored word only
// ever KEEPS a block the double expression would keep:
//   * 1 - a below 2^-20 (or not positive, or NaN): +inf -- never dropped.  Above it the rounding of a (two products, 2^-52
//     relative, a < 1) moves 1 - a by less than 2^-31 of itself;
//   * q is inflated by 2^-20 -- far above that, the quotient's and the test's own product's roundings together --, rounded UP
//     to float and kept out of the float denormals (a larger word only keeps);
//   * a block whose partial group has fewer than two views carries no information (s1 = +inf): +inf.
// q y < 1 in double with the stored q >= (1 + 2^-21) s1 / (1 - a) gives s1 y < (1 - 2^-22) (1 - a) in exact arithmetic, i.e.
// s1 (2e-12 tr + y) < 1 - 2^-22 (1 - a) < 1 - 2^-42, and the double evaluation of that expression (one fma, one product) is
// within 2^-51 of it: dropped there as well.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BB_FOLD_FN __host__ __device__ inline
#else
#define BB_FOLD_FN inline
#endif

namespace mocap {

BB_FOLD_FN float bb_fold_inf() {
  const uint32_t u = 0x7f800000u;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// smallest float >= x for x > 0 finite (plain conversion + one step where it rounded down); +inf above the float range
BB_FOLD_FN float bb_fold_float_up(double x) {
  float f = (float)x;
  if ((double)f < x) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 1u;  // (f > 0: the next float up, +inf behind the largest)
    memcpy(&f, &u, 4);
  }
  return f;
}

BB_FOLD_FN float bb_fold_bound(double s1, double tr) {
  const double den = 1.0 - s1 * (2e-12 * tr);
  if (!(den > 0x1p-20) || !(s1 == s1)) return bb_fold_inf();
  const double q = (s1 / den) * (1.0 + 0x1p-20);
  if (!(q < 3e38)) return bb_fold_inf();
  if (!(q > 0x1p-126)) return s1 > 0.0 ? 0x1p-126f : (float)q;  // (s1 <= 0 never comes out of a Cholesky trace; it is dropped as before)
  return bb_fold_float_up(q);
}

// the test pass: the block is dropped
BB_FOLD_FN bool bb_fold_dropped(float q, double y) { return (double)q * y < 1.0; }

}  // namespace mocap
