// precision_host.hpp -- the host's part of "predicted precision" (include/mocap_core.h): the argument rules of its entry points and
// the fold of the caller's coordinates into the per-call camera table.  Plain C++, read by a host compiler alone
// (csrc/precision_capi.hip, and tests/native/precision_check.cpp under the host sanitizers).  No inverse is taken anywhere.
#pragma once
#include <stdint.h>

namespace mocap {

constexpr int kPmMaxPoints = 1 << 24;           // mirrored from include/mocap_core.h (MOCAP_PM_MAX_POINTS)
constexpr int64_t kPmMaxVoxels = 1ll << 27;     // ... MOCAP_PM_MAX_VOXELS
constexpr int kPmMaxDim = 1024;                 // ... nx, ny, nz at most
constexpr int kPmSummary = 72;                  // ... MOCAP_PM_SUMMARY
constexpr int kPmHist = 65, kPmGood = 65, kPmBox = 66;  // the summary's layout: histogram 0 .. 64, GOOD, imin imax jmin jmax kmin kmax

inline bool pm_finite(double x) { return x - x == 0.0; }

// P' = P [[A, a], [0, 1]] per camera, frame = [A | a] row-major 3 x 4; frame == null: P' = P byte for byte.
//   P'[r][j] = (P[r][0] A[0][j] + P[r][1] A[1][j]) + P[r][2] A[2][j]                 j < 3
//   P'[r][3] = ((P[r][0] a[0] + P[r][1] a[1]) + P[r][2] a[2]) + P[r][3]
inline void pm_fold(int C, const double* P, const double* frame, double* out) {
  for (int c = 0; c < C; c++)
    for (int r = 0; r < 3; r++) {
      const double* p = P + 12 * c + 4 * r;
      double* o = out + 12 * c + 4 * r;
      if (!frame) {
        for (int j = 0; j < 4; j++) o[j] = p[j];
        continue;
      }
      for (int j = 0; j < 3; j++) o[j] = (p[0] * frame[j] + p[1] * frame[4 + j]) + p[2] * frame[8 + j];
      o[3] = ((p[0] * frame[3] + p[1] * frame[7]) + p[2] * frame[11]) + p[3];
    }
}

// The rules every entry takes: sigma_px finite and > 0; frame null or twelve finite numbers.  -> null, or what is wrong.
inline const char* pm_common_check(double sigma_px, const double* frame) {
  if (!(pm_finite(sigma_px) && sigma_px > 0.0)) return "sigma_px must be finite and > 0";
  if (frame)
    for (int i = 0; i < 12; i++)
      if (!pm_finite(frame[i])) return "frame must be finite";
  return nullptr;
}

// by visibility: width, height >= 1; near >= 0 (so not NaN); far > near, +inf allowed
inline const char* pm_vis_check(int width, int height, double near, double far) {
  if (width < 1 || height < 1) return "width and height must be >= 1";
  if (!(near >= 0.0) || !pm_finite(near)) return "near must be finite and >= 0";
  if (!(far > near)) return "far must be > near";
  return nullptr;
}

inline const char* pm_points_check(int64_t N) { return N < 1 || N > kPmMaxPoints ? "N outside 1 .. MOCAP_PM_MAX_POINTS" : nullptr; }

inline const char* pm_frames_check(int64_t n_frames, int K_max) {
  if (n_frames < 0 || K_max < 1) return "bad size argument";
  if (n_frames > kPmMaxPoints / (int64_t)K_max) return "n_frames x K_max above MOCAP_PM_MAX_POINTS";
  return nullptr;
}

inline const char* pm_map_check(int nx, int ny, int nz, int min_views, double max_sigma) {
  if (nx < 1 || ny < 1 || nz < 1 || nx > kPmMaxDim || ny > kPmMaxDim || nz > kPmMaxDim) return "nx, ny, nz outside 1 .. 1024";
  if ((int64_t)nx * ny * nz > kPmMaxVoxels) return "nx ny nz above MOCAP_PM_MAX_VOXELS";
  if (min_views < 0) return "min_views must be >= 0";
  if (max_sigma != max_sigma) return "max_sigma must not be NaN";
  return nullptr;
}

// The summary before any voxel: histogram and GOOD 0, every min the dimension, every max -1.
inline void pm_summary_init(int nx, int ny, int nz, int64_t* s) {
  for (int i = 0; i <= kPmGood; i++) s[i] = 0;
  const int dim[3] = {nx, ny, nz};
  for (int d = 0; d < 3; d++) {
    s[kPmBox + 2 * d] = dim[d];
    s[kPmBox + 2 * d + 1] = -1;
  }
}

}  // namespace mocap
