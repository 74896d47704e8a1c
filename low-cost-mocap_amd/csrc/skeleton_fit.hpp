// skeleton_fit.hpp -- skeleton fit (include/mocap_core.h, "skeleton fit"): what skeleton_fit.hip launches and skeleton_fit_capi.hip
// lays out.  A header of its own: no existing translation unit includes it.
#pragma once
#include "body_session.hpp"
#include "skeleton_fit_host.hpp"

namespace mocap {

constexpr int kSkPutDirs = 32;  // directed joints per table launch: the chunk travels as a kernel argument (3.5 KB of the 4 KB there are)

struct SkDirChunk {
  SkDir d[kSkPutDirs];
};

// The workspace of a round: per body kSkPlanes planes of `cap` doubles, [body][plane][frame of the round], so that lanes = frames
// coalesce.  H, g: the body's block (own terms, then its children's complements) and gradient; Up: the coupling to the parent as
// SkUp's 16 numbers; W = M^-1 C; Z = M^-1 g, then the step; Trial: the trial pose; Share: the body's markers' and its joint-to-
// parent's cost at the current pose, then at the trial pose.
constexpr int kSkH = 0, kSkG = 21, kSkUp = 27, kSkW = 43, kSkZ = 79, kSkTrial = 85, kSkShare = 92, kSkPlanes = 96;
constexpr size_t kSkWsCap = (size_t)256 << 20;  // bytes of round workspace at most: the frames are taken in rounds under it

// bytes of workspace one frame of a round takes
inline size_t sk_frame_bytes(int B) { return (size_t)B * (kSkPlanes * sizeof(double) + sizeof(int32_t)) + sizeof(double) + sizeof(int32_t); }
// frames per round: whole tiles, at least one
inline int64_t sk_round_frames(int B, int64_t n_frames) {
  const int64_t fit = (int64_t)(kSkWsCap / sk_frame_bytes(B)) / kTsTile * kTsTile, all = ts_tiles(n_frames) * kTsTile;
  return all < fit ? all : fit < kTsTile ? kTsTile : fit;
}

struct SkArgs {
  int64_t n_frames, f0, cap;  // F; the round's first frame; the planes' stride (frames per round)
  int nf;                     // frames of this round
  int R, B, J;
  double axis_len, w_joint;
  const double* traj;      // [R][F][3]
  const BpBody* bodies;    // workspace [B]
  const SkDir* dirs;       // workspace [2 J], ordered by (body, joint index)
  const int32_t* flag;     // [B][F]
  const double *quat, *t_pose;
  double *quat_s, *Rm_s, *t_s, *rms_s;  // [B][F][4], [9], [3], [1]: quat_s and t_s hold the current pose while the loop runs
  double *cost0, *cost;    // [F]
  int32_t *steps, *n_act;  // [F]
  double* ws;              // workspace [B][kSkPlanes][cap]
  int32_t* act;            // workspace [B][cap]: 1 = the (body, frame) is ACTIVE
  double* lam;             // workspace [cap]
  int32_t* piv;            // workspace [cap]: every pivot of the last solve finite and > 0
  int32_t* tile_i32;       // workspace [B][ts_tiles(F)] (sign_walk.hpp)
  uint8_t* parity;         // workspace [B][F]
  SkForest fr;
};

// ceil(n / 32) launches: the host's table into device memory, behind everything queued on the stream
hipError_t launch_put_sk_dirs(const SkDir* host, int n, SkDir* dev, hipStream_t stream);
// one round's frames: the start, `iters` passes of four launches, the outputs
hipError_t launch_fit_skeleton_round(const SkArgs& a, int iters, hipStream_t stream);
// the sign walk over quat_s, all frames: five launches
hipError_t launch_fit_skeleton_signs(const SkArgs& a, hipStream_t stream);

}  // namespace mocap
