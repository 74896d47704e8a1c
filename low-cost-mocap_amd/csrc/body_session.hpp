// body_session.hpp -- body trajectories (include/mocap_core.h, "body trajectories"): what body_session.hip launches and
// body_session_capi.hip lays out.  A header of its own: no existing translation unit includes it.
#pragma once
#include <vector>

#include "track_smooth.hpp"

namespace mocap {

constexpr int kBpMaxBodies = 64;  // mirrored from include/mocap_core.h (MOCAP_BP_MAX_BODIES)
constexpr int kBpMaxMarkers = 8;  // the rigid-body section's (MOCAP_RB_MAX_MARKERS)
constexpr int kBpPosed = 1, kBpFew = 2, kBpDegenerate = 4, kBpRms = 8;                       // MOCAP_BP_*
constexpr int kBpSrcNone = 0, kBpSrcMeasured = 1, kBpSrcRigid = 2, kBpSrcRigidFilled = 3;  // MOCAP_BP_SRC_*
constexpr int kBpPutBodies = 8;   // bodies per table launch: the chunk travels as a kernel argument (2.1 KB of the 4 KB there are)

struct BpBody {                       // one body of a call, as the host tabulates it
  int32_t n, pad;                     // markers
  int32_t rows[kBpMaxMarkers];        // the session row of each marker
  double q[kBpMaxMarkers][3];         // body coordinates
  unsigned long long posable[4];      // bit s: the marker subset s (bit m = marker m) is posable
};
struct BpBodyChunk {
  BpBody b[kBpPutBodies];
};

struct PoseRowsArgs {
  int64_t n_frames;
  int R, B;
  double max_rms;
  const double* traj;       // [R][F][3]
  const BpBody* bodies;     // workspace [B]
  int32_t* tile_i32;        // workspace [B][ts_tiles(F)]: the last POSED frame of a tile, then of the tiles before it; then the parities
  uint8_t* parity;          // workspace [B][F]: the flips' parity within the tile, up to and including the frame
  int32_t *n_used, *present, *flag;  // [B][F]
  double *quat, *Rm, *t_pose, *rms;  // [B][F][4], [9], [3], [1]
};

struct SmoothRotationsArgs {
  int64_t n_frames;
  int B, degree, W, n_min, max_gap;
  double span;
  const double* t;          // [F]
  const double* quat;       // [B][F][4]
  const uint8_t* good;      // workspace [F] (launch_good_times)
  double *quat_s, *omega, *res;  // [B][F][4], [3], [1]
  int32_t *n_used, *flag;        // [B][F]
};

struct FillRowsArgs {
  int64_t n_frames;
  int R, B;
  const double* traj;       // [R][F][3]
  const BpBody* bodies;     // workspace [B]
  int32_t* row_of;          // workspace [R]: 8 b + m of the row, -1 = a row of no body
  const int32_t* flag;      // [B][F] stage 1
  const double *Rm, *t_pose;
  const int32_t* flag_s;    // [B][F] or null (then quat_s and pos_s are null too)
  const double *quat_s, *pos_s;
  double* filled;           // [R][F][3]
  int32_t* src;             // [R][F]
};

// ceil(B / 8) launches: the host's table into device memory, behind everything queued on the stream
hipError_t launch_put_bodies(const BpBody* host, int B, BpBody* dev, hipStream_t stream);
// the poses and, in four more launches, the sign-continuous quaternions
hipError_t launch_pose_rows(const PoseRowsArgs& a, hipStream_t stream);
// the fit alone: the good-time bits are track_smooth.hpp's launch_good_times
hipError_t launch_smooth_rotations(const SmoothRotationsArgs& a, hipStream_t stream);
// two launches: the row table, the fill
hipError_t launch_fill_rows(const FillRowsArgs& a, hipStream_t stream);

// Host side (body_session_capi.hip), shared with "joint poses": the bodies of a call checked by the section's rules and tabulated
// with their posable masks.  `who` is the public call's name in the error text; the context's lock is the caller's.
int bodies_table(mocap_ctx* ctx, const char* who, int R, int B, const int32_t* n_markers, const int32_t* rows, const double* markers,
                 std::vector<BpBody>& table);

}  // namespace mocap
