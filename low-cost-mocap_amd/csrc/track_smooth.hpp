// track_smooth.hpp -- trajectories (include/mocap_core.h, "trajectories"): what track_smooth.hip launches and
// track_smooth_capi.hip lays out, and what the later session stages (stitching, body trajectories) share with them.
#pragma once
#include "kernels.hpp"

struct mocap_ctx;

namespace mocap {

constexpr int kTsMaxRows = 1024;      // mirrored from include/mocap_core.h (MOCAP_TS_MAX_ROWS)
constexpr int kTsMaxHalfWindow = 32;  // ... (MOCAP_TS_MAX_HALF_WINDOW)
constexpr int kTsMaxPoints = 64;      // K_max, the marker tracker's
constexpr int kTsTile = 256;          // frames per workgroup, of every kernel of the section
constexpr int kTsSmoothed = 1, kTsFilled = 2, kTsFew = 4, kTsSingular = 8, kTsBadTime = 16;  // MOCAP_TS_*

inline int64_t ts_tiles(int64_t n_frames) { return (n_frames + kTsTile - 1) / kTsTile; }

// the session kernels' test of a sample
__device__ __forceinline__ bool finite1(double v) { return fabs(v) < __builtin_inf(); }  // false for NaN
template <int N>
__device__ __forceinline__ bool finiteN(const double* p) {
  bool ok = finite1(p[0]);
#pragma unroll
  for (int k = 1; k < N; k++) ok = ok && finite1(p[k]);
  return ok;
}

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

struct GoodTimesArgs {
  int64_t n_frames;
  const double* t;   // [F]
  double* tile_max;  // workspace [ts_tiles(F)]: per tile the largest finite t, then the largest before the tile
  uint8_t* good;     // workspace [F]: 1 = the frame has a good time
};

struct SmoothTracksArgs {
  int64_t n_frames;
  int R, degree, W, n_min, max_gap;
  double span;
  const double* t;      // [F]
  const double* traj;   // [R][F][3]
  const uint8_t* good;  // [F] (launch_good_times)
  double *pos, *vel, *acc;  // [R][F][3]
  double* res;              // [R][F]
  int32_t *n_used, *flag;   // [R][F]
};

// one launch: a lane per frame, every row of traj written
hipError_t launch_gather_tracks(const GatherTracksArgs& a, hipStream_t stream);
// three launches: the good-time bits of t (tile maxima, their prefix, the bits)
hipError_t launch_good_times(const GoodTimesArgs& a, hipStream_t stream);
// the fit alone
hipError_t launch_smooth_tracks(const SmoothTracksArgs& a, hipStream_t stream);

// Host side (track_smooth_capi.hip), shared by the sections that take rows and a window.  `who` is the public call's name in the
// error text; the context's lock is the caller's.
int rows_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int R);
int window_check(mocap_ctx* ctx, const char* who, int degree, int W, double span, int n_min, int max_gap);
// the good-time bits of t [F] (device memory): their workspace carved out of the context's calib_ws (`ws` names it in the error
// text), the three launches queued -> good [F]
int good_times_locked(mocap_ctx* ctx, const char* ws, int64_t n_frames, const double* t, const uint8_t** good);

}  // namespace mocap
