// track_stitch.hpp -- track stitching (include/mocap_core.h, "track stitching"): what track_stitch.hip launches and
// track_stitch_capi.hip lays out.
#pragma once
#include "track_smooth.hpp"

namespace mocap {

constexpr int kStMaxFit = 64;    // mirrored from include/mocap_core.h (MOCAP_ST_MAX_FIT)
constexpr int kStModel = 7;      // doubles of an end model: pos [3], vel [3], the time of its end frame

struct StitchTracksArgs {
  int64_t n_frames;
  int R, fit_frames;
  double max_dt, gate, gate_rate;
  const double* t;     // [F]
  const double* traj;  // [R][F][3]
  double* tile_max;    // workspace [ts_tiles(F)], the good-time launches'
  uint8_t* good;       // workspace [F]: 1 = the frame has a good time
  double* model;       // workspace [R][2][kStModel]: the tail model of row r, then its head model
  double* table;       // workspace [R][R]: the cost of p -> q, +inf = not admissible
  int32_t* ext;        // [R][3]
  int32_t *next, *prev;  // [R]
  double* cost;          // [R]
  int32_t *chain, *row_of;  // [R]
  int32_t* n_chains;        // [1]
};

// eight launches: the good-time bits (three, track_smooth.hip's), extents (two), end models, pair costs, association and chains
hipError_t launch_stitch_tracks(const StitchTracksArgs& a, hipStream_t stream);

}  // namespace mocap
