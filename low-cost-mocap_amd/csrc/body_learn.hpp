// body_learn.hpp -- rigid-body learning (include/mocap_core.h, "rigid-body learning"): what body_learn.hip launches and
// body_learn_capi.hip lays out.  A header of its own: no existing translation unit includes it.
#pragma once
#include "kernels.hpp"

namespace mocap {

constexpr int kLbResult = 129;  // mirrored from include/mocap_core.h (MOCAP_LB_RESULT)
// one partial per workgroup (the grid is calib_partials(F), 256 frames each), per pass:
constexpr int kLbGatherSlab = 2 + 2 * kRbPairs;         // valid frames, lowest complete frame, c_ij [28], sum D [28]
constexpr int kLbSpreadSlab = kRbPairs;                 // sum (D - d_ij)^2 [28]
constexpr int kLbRoundSlab = 5 * kRbMaxMarkers + 2;     // per marker {sum y [3], count, sum |y - q|^2}, frames used, sum rms^2
constexpr int kLbSlabDoubles = kLbGatherSlab;           // the widest of the three

// what the launches of one call hand to each other, in device memory
struct BodyLearnState {
  double Q[kRbMaxMarkers][3];  // the template of the round to come (rows >= N zero)
  double d[kRbPairs];          // d_ij, for the second pass of the pair statistics
  int32_t no_ref;              // 1: there is no reference frame, every later launch returns at once
  int32_t flags;               // MOCAP_LB_ST_* collected over the rounds
};

struct BodyLearnArgs {
  int64_t n_frames;
  int K_max, N;
  int32_t sel[kRbMaxMarkers];
  int64_t ref_frame;  // -1 = the lowest valid frame that shows every marker
  double max_rms;
  const double* xyz;      // [F][K_max][3]
  const int32_t* n_pts;   // [F]
  const int32_t* id;      // [F][K_max]
  const int32_t* status;  // [F] or null
  int8_t* slot;           // [F][8]: the slot each marker is present at, -1 = absent (an invalid frame: all -1)
  double* slab;           // [calib_partials(F)][kLbSlabDoubles]
  BodyLearnState* state;
  double* result;         // [kLbResult]
};

// the whole call: gather, pair statistics, `iters` rounds -- 4 + 2 iters launches on `stream`, no host round trip
hipError_t launch_body_learn(const BodyLearnArgs& a, int iters, hipStream_t stream);

}  // namespace mocap
