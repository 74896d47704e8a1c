// track_smooth.hpp -- trajectories (include/mocap_core.h, "trajectories"): what track_smooth.hip launches and
// track_smooth_capi.hip lays out.  A header of its own: no existing translation unit includes it.
#pragma once
#include "kernels.hpp"

namespace mocap {

constexpr int kTsMaxRows = 1024;      // mirrored from include/mocap_core.h (MOCAP_TS_MAX_ROWS)
constexpr int kTsMaxHalfWindow = 32;  // ... (MOCAP_TS_MAX_HALF_WINDOW)
constexpr int kTsMaxPoints = 64;      // K_max, the marker tracker's
constexpr int kTsTile = 256;          // frames per workgroup, of every kernel of the section

inline int64_t ts_tiles(int64_t n_frames) { return (n_frames + kTsTile - 1) / kTsTile; }

struct GatherTracksArgs {
  int64_t n_frames;
  int K_max, min_hits, n_ids, R;
  const double* xyz;       // [F][K_max][3]
  const int32_t* n_pts;    // [F]
  const int32_t* id;       // [F][K_max]
  const int32_t* hits;     // [F][K_max] or null
  const int32_t* relabel;  // [n_ids]
  double* traj;            // [R][F][3]
};

struct SmoothTracksArgs {
  int64_t n_frames;
  int R, degree, W, n_min, max_gap;
  double span;
  const double* t;     // [F]
  const double* traj;  // [R][F][3]
  double* tile_max;    // workspace [ts_tiles(F)]: per tile the largest finite t, then the largest before the tile
  uint8_t* good;       // workspace [F]: 1 = the frame has a good time
  double *pos, *vel, *acc;  // [R][F][3]
  double* res;              // [R][F]
  int32_t *n_used, *flag;   // [R][F]
};

// one launch: a lane per frame, every row of traj written
hipError_t launch_gather_tracks(const GatherTracksArgs& a, hipStream_t stream);
// three launches: the good-time bits of t (tile maxima, their prefix, the bits); reads n_frames and t, writes tile_max and good
hipError_t launch_good_times(const SmoothTracksArgs& a, hipStream_t stream);
// four launches: the good-time bits, then the fit
hipError_t launch_smooth_tracks(const SmoothTracksArgs& a, hipStream_t stream);

}  // namespace mocap
