// joints.hpp -- joints of a recorded session (include/mocap_core.h, "joints"): what joints.hip launches and joints_capi.hip lays
// out.  A header of its own: no existing translation unit includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "joints_host.hpp"

namespace mocap {

constexpr int kJtTile = 256;                       // frames per workgroup of the pair passes: the contract's tile
constexpr int kJtBlock = 4;                        // bodies per side of a block of pairs
constexpr int kJtPairs = kJtBlock * kJtBlock;      // pairs of a block pair: pair = 4 * (a - a0) + (b - b0)
constexpr int kJtSums = 16;                        // sums per pair: Rel (9, row-major), d (3), g (3), d.d
constexpr int kJtSlots = kJtPairs * kJtSums;       // slab slots of a block pair in the first pass: slot = 16 * pair + sum
constexpr int kJtPutJoints = 16;                   // joints per table launch: the chunk travels as a kernel argument (2 KB)

__host__ __device__ inline int64_t jt_tiles(int64_t n_frames) { return (n_frames + kJtTile - 1) / kJtTile; }
__host__ __device__ inline int jt_blocks(int B) { return (B + kJtBlock - 1) / kJtBlock; }
__host__ __device__ inline int jt_block_pairs(int B) { return jt_blocks(B) * (jt_blocks(B) + 1) / 2; }  // (bp, bq), bp <= bq

struct FindJointsArgs {
  int64_t n_frames;
  int B, min_common;
  double tol_rank, max_sep;
  const int32_t* flag;     // [B][F]
  const double *Rm, *t_pose;  // [B][F][9], [B][F][3]
  double* slab;            // workspace [round_pairs * kJtSlots][P]: the tile sums of one slot lie together
  int32_t* cslab;          // workspace [round_pairs * kJtPairs][P]: the tile counts
  double* sums;            // workspace [B][B][16]: the sixteen SUMs of a pair a < b
  int round_pairs;         // block pairs per round of launches (the slab holds that many)
  int32_t *cnt, *kind, *accepted;      // [B][B]
  double *lam, *sep, *centre, *axis;   // [B][B][3], [B][B], [B][B][3], [B][B][3]
  int32_t *parent, *n_joints;          // [B], [1]
};

struct JointSeriesArgs {
  int64_t n_frames;
  int B, J;
  const int32_t* flag;     // [B][F]
  const double *quat, *Rm, *t_pose;  // [B][F][4], [9], [3]
  const JtJoint* joints;   // workspace [J]
  int32_t* present;        // [J][F]
  double *centre, *gap, *quat_rel, *twist;  // [J][F][3], [J][F], [J][F][4], [J][F][2]
};

struct JtJointChunk {
  JtJoint j[kJtPutJoints];
};

// per round of block pairs: the sixteen sums and their fold; one lane per pair for the 6 x 6 problem; per round again: the
// residual and its fold (sep, accepted); one workgroup for the skeleton
hipError_t launch_find_joints(const FindJointsArgs& a, hipStream_t stream);
// ceil(J / 16) launches: the host's table into device memory, behind everything queued on the stream
hipError_t launch_put_joints(const JtJoint* host, int J, JtJoint* dev, hipStream_t stream);
hipError_t launch_joint_series(const JointSeriesArgs& a, hipStream_t stream);

}  // namespace mocap
