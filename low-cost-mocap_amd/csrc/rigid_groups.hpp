// rigid_groups.hpp -- rigid groups (include/mocap_core.h, "rigid groups"): what rigid_groups.hip launches and
// rigid_groups_capi.hip lays out.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mocap {

constexpr int kRgMaxRows = 256;            // mirrored from include/mocap_core.h (MOCAP_RG_MAX_ROWS)
constexpr int64_t kRgMaxFrames = 1 << 22;  // mirrored from include/mocap_core.h (MOCAP_RG_MAX_FRAMES)
constexpr int kRgTile = 256;               // frames per workgroup of the pair pass: the contract's tile
constexpr int kRgBlock = 8;                // rows per side of a block of pairs
constexpr int kRgSlots = kRgBlock * kRgBlock;  // slab slots of a block pair: slot = 8 * (p - p0) + (q - q0)

__host__ __device__ inline int64_t rg_tiles(int64_t n_frames) { return (n_frames + kRgTile - 1) / kRgTile; }
__host__ __device__ inline int rg_blocks(int R) { return (R + kRgBlock - 1) / kRgBlock; }
__host__ __device__ inline int rg_block_pairs(int R) { return rg_blocks(R) * (rg_blocks(R) + 1) / 2; }  // (bp, bq), bp <= bq

struct RigidGroupsArgs {
  int64_t n_frames;
  int R, min_common;
  double tol, max_dist, min_travel;
  const double* traj;  // [R][F][3]
  double* slab;        // workspace [round_pairs * kRgSlots][P]: the tile sums of one slot lie together
  int32_t* cslab;      // workspace, the same shape: the tile counts
  unsigned long long* bounds;  // workspace [R][6]: order-preserving keys of min x, y, z and max x, y, z
  int round_pairs;     // block pairs per round of launches (the slab holds that many)
  int32_t* cnt;        // [R][R]
  double *dist, *spread;  // [R][R]
  double* travel;         // [R]
  int32_t *group_of, *gsize, *ghead, *gconf;  // [R]
  double* gspread;                            // [R]
  int32_t* n_groups;                          // [1]
};

// the bounds (two launches), then per round of block pairs: pair sums, their fold (cnt, dist), pair squares, their fold (spread);
// then one workgroup for travel, edges, components and the per-group figures
hipError_t launch_rigid_groups(const RigidGroupsArgs& a, hipStream_t stream);

}  // namespace mocap
