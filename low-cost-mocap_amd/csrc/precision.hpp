// precision.hpp -- predicted precision (include/mocap_core.h, "predicted precision"): what precision.hip launches and
// precision_capi.hip lays out.  A header of its own: no existing translation unit includes it.
#pragma once
#include <hip/hip_runtime.h>

#include "precision_host.hpp"
#include "precision_math.hpp"

namespace mocap {

constexpr int kPmThreads = 256;   // the map and the point forms: lanes per workgroup
constexpr int kPmPutCams = 32;    // cameras per table launch: the chunk travels as a kernel argument (3 KB of the 4 KB there are)

struct PmTabChunk {
  double p[kPmPutCams * 12];
};

// what every form shares
struct PmArgs {
  int C;
  const double* tab;   // workspace [C][12]: P', the per-call camera table in the caller's coordinates
  double sigma_px;
  PmVis vis;           // by visibility only
  // outputs of the point and frame forms, [n][..]
  double *cov, *sig, *axis;  // [n][6] or null, [n][3], [n][3] or null
  int32_t *n_views, *info;   // [n]
};

struct PmPointArgs {
  PmArgs s;
  int64_t N;
  const double* xyz;     // [N][3]
  const uint64_t* seen;  // [N] or null = by visibility
};

struct PmFrameArgs {
  PmArgs s;
  int64_t n_frames;
  int K_max;
  const double* xyz;      // [F][K_max][3]
  const int16_t* corr;    // [F][K_max][C]
  const int32_t* n_pts;   // [F]
  const int32_t* status;  // [F] or null (= 0)
};

struct PmMapArgs {
  PmArgs s;  // (cov, sig, axis, n_views, info unused)
  int nx, ny, nz;
  double origin[3], e0[3], e1[3], e2[3];
  int min_views;
  double max_sigma;
  uint8_t* n_views;             // [nz][ny][nx]
  float* sig_max;               // [nz][ny][nx]
  uint64_t* seen;               // [nz][ny][nx] or null
  unsigned long long* summary;  // [kPmSummary] as int64
};

// ceil(C / 32) launches: the host's table into device memory, behind everything queued on the stream
hipError_t launch_pm_put_table(const double* host, int C, double* dev, hipStream_t stream);
hipError_t launch_pm_points(const PmPointArgs& a, hipStream_t stream);
hipError_t launch_pm_frames(const PmFrameArgs& a, hipStream_t stream);
// two launches: the summary's start, then the voxels
hipError_t launch_pm_map(const PmMapArgs& a, hipStream_t stream);

}  // namespace mocap
