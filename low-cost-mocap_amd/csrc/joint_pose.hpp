// joint_pose.hpp -- joint poses (include/mocap_core.h, "joint poses"): what joint_pose.hip launches and joint_pose_capi.hip lays
// out.  A header of its own: no existing translation unit includes it.
#pragma once
#include "body_session.hpp"
#include "joint_pose_host.hpp"

namespace mocap {

constexpr int kJpPutDirs = 24;  // directed joints per table launch: the chunk travels as a kernel argument (3.4 KB of the 4 KB there are)

struct JpDirChunk {
  JpDir d[kJpPutDirs];
};

struct PoseJointsArgs {
  int64_t n_frames;
  int R, B;
  double axis_len, max_rms;
  const double* traj;     // [R][F][3]
  const BpBody* bodies;    // workspace [B]
  const JpDir* dirs;       // workspace [2 J], ordered by (body, joint index)
  const int32_t* flag;     // [B][F] mocap_pose_rows'
  const double *quat, *Rm, *t_pose;
  int32_t *flag_j, *hops, *via;        // [B][F]
  double *quat_j, *Rm_j, *t_j, *rms_j;  // [B][F][4], [9], [3], [1]
  int32_t* tile_i32;       // workspace [B][ts_tiles(F)] (sign_walk.hpp)
  uint8_t* parity;         // workspace [B][F]
  int32_t first[kJpMaxBodies + 1];  // dirs[first[y] .. first[y + 1]) are the joints of body y
};

// ceil(n / 24) launches: the host's table into device memory, behind everything queued on the stream
hipError_t launch_put_dirs(const JpDir* host, int n, JpDir* dev, hipStream_t stream);
// round 0, one launch per round 1 .. max_rounds, and the sign walk's five
hipError_t launch_pose_joints(const PoseJointsArgs& a, int max_rounds, hipStream_t stream);

}  // namespace mocap
