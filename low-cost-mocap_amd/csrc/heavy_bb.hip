// heavy_bb.hip -- the candidate space of ONE root when no enumeration reaches its end.
//
// The reference expands the Cartesian product of a root's gated hits over the cameras, whatever its size
// (reference computer_code/api/helpers.py:394-400), triangulates every group and keeps the first minimum of the reprojection
// error (helpers.py:408-421).  Two markers that lie behind each other as seen from the root's camera put TWO hits into
// nearly every other camera: at 64 cameras that is 2^60 groups -- the reference would not return either, and the frame
// kernels cap a root at 2^24 groups and flag the frame.  The winner of such a root can still be found exactly:
//
//   * a group's error is bounded from below by the smallest eigenvalue of its DLT matrix (EigCut, mocap_device.hpp), and the
//     matrix of a PARTIAL group -- some multi-hit cameras not yet decided -- bounds every completion (it is a sum of
//     positive semi-definite terms): the same inequality, with the same rounding allowances, csrc/frame_bb.hip drops its
//     blocks on;
//   * the search goes through the multi-hit cameras level by level (breadth first).  A node = the digits chosen so far + the
//     DLT matrix of the single-hit cameras and those digits; its children (one per hit of the next camera) are tested against
//     the error of group 0 -- the closest hit in every camera, evaluated by the frame kernel itself before this kernel runs,
//     almost always the winner -- and the survivors form the next level's frontier;
//   * the leaves that survive the last level are complete groups: they are triangulated and scored by the SAME device
//     function, in the same camera order, as every other group of the path (triangulate_and_score), and the first minimum
//     in candidate order (error bits, then the mixed-radix index compared digit by digit from the slowest camera down)
//     replaces the root's point if it beats group 0.
//
// Nothing is dropped on anything but a rigorous bound, so the result is the one the enumeration would give
// (tests/test_gpu_wide_adversarial.py runs roots both ways where the enumeration is feasible).  A frontier that outgrows the
// workspace (two markers that coincide to within the noise in most cameras: nothing separates the mixtures) flags the frame
// like the cap did.
//
// One 1 024-lane workgroup per heavy root (records exported by frame_kernel.hip's wide variant in the re-submit pass);
// plain intrinsics only -- one matrix for all cameras or one per camera (the host does not export otherwise).
#include "mocap_device.hpp"
#include "kernels.hpp"
#include "frame_common.hpp"

namespace mocap {

constexpr int kHvThreads = 1024;  // (one workgroup per CU: the frontier of a hard root is tens of thousands of nodes per level)
constexpr int kHvEnumDigits = 20;  // multi-hit cameras of a root the fall-back enumerates (product <= 2^20, two hits at least each)
constexpr int kHvGlobalEnumDigits = 24;  // ... of a root heavy_enum_kernel enumerates over the whole GPU (product <= 2^24)
constexpr int kHvEnumThreads = 256;
constexpr int kHvEnumSlice = 16 * kHvEnumThreads;  // groups per slice (roots with more hits than the table holds)
constexpr int kHvEnumTab = 256;  // hits of a root heavy_enum_kernel tabulates (contribution + pixel)
constexpr int kHvDigits = 64;  // digit slots of a node (>= multi-hit cameras of a root: < kMaxCameras)

size_t heavy_bb_ws_bytes(int ncap) { return (size_t)2 * ncap * (sizeof(double) * 10 + kHvDigits); }

// The two kernels below exist twice, as frame_bb.hip's search does: the identical-K kernels and the per-camera-K ones
// (heavy_bb_calib_kernel, heavy_enum_calib_kernel) are the same text (heavy_bb_body.inc, heavy_enum_body.inc), included once per
// __global__ with HV_PERK set.  PERK: one plain K per camera.  The reference takes the intrinsics of a view by the POSITION of
// its camera among the cameras the group sees (helpers.py:305-307, :231-237).  In a heavy root every camera with at least one
// hit is in every group, so the position of camera c is a property of the root -- the cameras below c with a hit, the root's own
// among them -- whatever digits are chosen: s_pos[], computed once per root next to s_lvl / s_dcam.  DLT contributions come from
// Pq[position][camera] = K[position] [R|t][camera], the table triangulate_and_score<UNIFORM_K=false> reads, which scores the
// leaves and the enumerated groups; rows and reprojection of a view then use the same K, the identity ra.x = z (v - v^) the
// eigenvalue bound rests on holds, and P_c[2] = (R_c[2], t_c[2]) for every plain K: the bounds keep their constants (p3max2,
// p3max2c, bb_c0) and allowances.
template <bool F32R>
__global__ __launch_bounds__(kHvThreads) void heavy_bb_kernel(HeavyArgs a) {
#define HV_PERK false
#include "heavy_bb_body.inc"
#undef HV_PERK
}
template <bool F32R>
__global__ __launch_bounds__(kHvThreads) void heavy_bb_calib_kernel(HeavyArgs a) {
#define HV_PERK true
#include "heavy_bb_body.inc"
#undef HV_PERK
}

// ---------------------------------------------------------------------------------------------------------------------
// heavy_enum_kernel: the roots the search gave up on with at most 2^24 groups, ENUMERATED -- every group of the Cartesian
// product triangulated and scored by the path's own device function (helpers.py:394-421 as written), the whole GPU on one
// root at a time.  All workgroups walk the queued roots in the same order and pull slices of the root's group range from a
// counter; a lane keeps the first minimum of its ascending run, the smallest error seen anywhere (a global word) is everybody's
// cut-off (a cut-off only ever skips work: mocap_device.hpp); per workgroup the lexicographic minimum of (error bits, group
// index) goes to a partial record, and the last workgroup to report merges the records the same way and writes the root's
// slot -- the first minimum in candidate order (np.argmin, helpers.py:418), whatever ran where.
struct HvPart {
  unsigned long long ebits;
  uint32_t g, pad;
  double X[3];
};
static_assert(sizeof(HvPart) == kHeavyEnumPartBytes, "partial record layout");

template <bool F32R>
__global__ __launch_bounds__(kHvEnumThreads) void heavy_enum_kernel(HeavyArgs a) {
#define HV_PERK false
#include "heavy_enum_body.inc"
#undef HV_PERK
}
template <bool F32R>
__global__ __launch_bounds__(kHvEnumThreads) void heavy_enum_calib_kernel(HeavyArgs a) {
#define HV_PERK true
#include "heavy_enum_body.inc"
#undef HV_PERK
}

// (the variant follows the camera tables: CamView::uniformK says which layout Pq has; the host exports heavy roots for
// per-camera K only when every matrix is plain)
hipError_t launch_heavy_enum(const HeavyArgs& a, hipStream_t stream) {
  void (*k)(HeavyArgs);
  if (a.cv.uniformK)
    k = a.cv.f32_rounding ? heavy_enum_kernel<true> : heavy_enum_kernel<false>;
  else
    k = a.cv.f32_rounding ? heavy_enum_calib_kernel<true> : heavy_enum_calib_kernel<false>;
  hipLaunchKernelGGL(k, dim3(a.enum_grid), dim3(kHvEnumThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_heavy_bb(const HeavyArgs& a, int grid, hipStream_t stream) {
  void (*k)(HeavyArgs);
  if (a.cv.uniformK)
    k = a.cv.f32_rounding ? heavy_bb_kernel<true> : heavy_bb_kernel<false>;
  else
    k = a.cv.f32_rounding ? heavy_bb_calib_kernel<true> : heavy_bb_calib_kernel<false>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(kHvThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
