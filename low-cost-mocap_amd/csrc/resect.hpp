// resect.hpp -- what csrc/resect.hip (kernels) and csrc/resect_capi.hip (the "camera resection" section of include/mocap_core.h) share:
// the argument block of every launch and the launchers, which own the grid formulas.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "resect_math.hpp"

namespace mocap {

constexpr int kRsTile = 256;    // rows staged through LDS at a time by the scoring kernel
constexpr int kRsSlice = 512;   // rows per point slice (grid.y) of the scoring kernel
constexpr int kRsCandTile = 256;  // candidate poses (hypothesis x solution) per workgroup of the scoring kernel
// the record the fold kernels write into pinned host memory: sums [kRsSums] | pose [12] | state [6] | finish [4]
constexpr int kRsRecPose = kRsSums, kRsRecState = kRsSums + 12, kRsRecFinish = kRsSums + 18, kRsRec = 64;
// pose slots of RsArgs::pose
constexpr int kRsSlotCur = 0, kRsSlotBase = 1, kRsSlotInc = 2, kRsSlotWinner = 3, kRsSlotPrior = 4, kRsSlots = 5;

struct RsArgs {
  int64_t N;
  int H, has_prior, min_inliers;
  uint64_t seed;
  double k4[4], thr2;   // fx, fy, cx, cy; threshold_px^2
  const double* X;      // [N][3]  device
  const double* obs;    // [N][2]
  double* rows;         // [N][5]: X, u, v of the valid rows, in input order
  int32_t* orig;        // [N]: input row of a valid row
  int32_t* hdr;         // [0] valid rows
  int32_t* blk;         // [calib_partials(N)] valid rows per workgroup of the compaction, then their offsets
  double* poses;        // [H][4][12]
  int32_t* n_sol;       // [H]
  int32_t* samp;        // [H][3] input rows of the sample (-1: the prior)
  int32_t* counts;      // [H][4]
  double* state;        // valid rows, winner's inliers, hypothesis, solution, hypotheses without a solution, status
  double* pose;         // [kRsSlots][12]: 0 the pose being linearised, 1 the base of a trial, 2 the trial's increment (G | dt),
                        // 3 the winner, 4 the prior (NaN without one)
  uint8_t* mask;        // [N] by valid row: the current inlier mask
  uint8_t* mask_out;    // [N] by input row
  double* slab;         // [calib_partials(N)][kRsSums]
  double* rec;          // [kRsRec] pinned host memory
};

hipError_t launch_resect_search(const RsArgs& a, hipStream_t stream);   // compact, hypotheses, score, winner
// slot 0 linearised -> rec.  with_base = 0: the mask becomes the classification at slot 0 first; 1: slot 0 is the trial
// slot 1 + slot 2, the mask stays and the sums carry the cost's change against slot 1
hipError_t launch_resect_normal_eq(const RsArgs& a, int with_base, hipStream_t stream);
hipError_t launch_resect_finish(const RsArgs& a, hipStream_t stream);   // the mask at pose slot 0 and the three costs -> rec

}  // namespace mocap
