// ba_lens.hip -- the kernels of the "lens calibration" section of include/mocap_core.h: the joint bundle adjustment with the full lens
// model -- per camera fx, fy, cx, cy, k1, k2, p1, p2 beside its pose -- and the inverse of that lens for observations.  The
// linearisation and the camera blocks are the kernels of csrc/ba_schur.hpp with this section's camera model (csrc/ba_lens.hpp): a
// camera's 14 x 14 block is 105 + 14 sums, more than one lane can carry, so its upper triangle is cut into four row bands.  The start
// (participation, DLT), the back-substitution and the finish (gauge) know no model: csrc/ba_joint.hip.  Written here:
//   undistort  one lane per observation: a fixed number of Newton steps on the 2 x 2 lens system
// FP64 throughout, nothing fused, no atomics: every output is a function of the inputs alone.
#include "ba_lens.hpp"

namespace mocap {

namespace {

constexpr int kT = kCalibThreads;

// --------------------------------------------------------------------------------------------------------------- undistort
__global__ __launch_bounds__(kT) void bal_undistort_kernel(int C, int64_t n_obs, const double* in, const double* K,
                                                           const double* dist, double* out) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n_obs) return;
  const int c = (int)(i % C);
  double uo, vo;
  bal_undistort(K + 9 * c, dist + 5 * c, in[2 * i], in[2 * i + 1], uo, vo);
  out[2 * i] = uo;
  out[2 * i + 1] = vo;
}

}  // namespace

hipError_t launch_bal_linearise(const SchurArgs& a, hipStream_t stream) { return schur_launch_linearise<BalModel>(a, stream); }

hipError_t launch_bal_undistort(int C, int64_t N, const double* in, const double* K, const double* dist, double* out,
                                hipStream_t stream) {
  const int64_t n_obs = N * C;
  hipLaunchKernelGGL(bal_undistort_kernel, dim3((unsigned)calib_partials(n_obs)), dim3(kT), 0, stream, C, n_obs, in, K, dist, out);
  return hipGetLastError();
}

}  // namespace mocap
