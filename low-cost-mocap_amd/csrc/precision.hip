// precision.hip -- the "predicted precision" section of include/mocap_core.h: sigma_px^2 H^-1 at given points, at the points of a
// frame batch, or over a voxel grid.  The core's own contract (the reference has no counterpart).
//
// One lane per point, slot or voxel (i fastest: a wave's stores of the map are consecutive), walking csrc/precision_math.hpp.  The
// loop over the cameras is wave-uniform and the per-call table P' [C][12] is addressed through the constant address space: one
// scalar-cache read per wave and camera.  H (6) and the Jacobi state (9 + 9 doubles) are registers.  No LDS but for the map's
// summary: a workgroup's histogram, GOOD count and bounding box are integers reduced in LDS, then one integer atomic per non-empty
// entry and workgroup -- the result does not depend on the order.  No floating-point atomics.
#include "precision.hpp"

#include "kernels.hpp"
#include "mocap_device.hpp"

namespace mocap {

namespace {

__global__ __launch_bounds__(64) void pm_put_kernel(PmTabChunk c, int count, double* dev) {
  for (int i = threadIdx.x; i < count * 12; i += 64) dev[i] = c.p[i];
}

__device__ __forceinline__ void pm_store(const PmArgs& s, size_t i, const PmPoint& o) {
  if (s.cov)
    for (int e = 0; e < 6; e++) s.cov[i * 6 + e] = o.cov[e];
  for (int e = 0; e < 3; e++) s.sig[i * 3 + e] = o.sig[e];
  if (s.axis)
    for (int e = 0; e < 3; e++) s.axis[i * 3 + e] = o.axis[e];
  s.n_views[i] = o.n_views;
  s.info[i] = o.info;
}

__global__ __launch_bounds__(kPmThreads) void pm_points_kernel(PmPointArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kPmThreads + threadIdx.x;
  if (i >= a.N) return;
  const uint64_t bits = a.seen ? a.seen[i] : 0;
  auto named = [&](int c) -> bool { return (bits >> c) & 1; };
  PmPoint o;
  pm_point(a.s.C, as_ctab(a.s.tab), a.seen == nullptr, named, a.s.vis, a.s.sigma_px, a.xyz[i * 3], a.xyz[i * 3 + 1], a.xyz[i * 3 + 2], o);
  pm_store(a.s, (size_t)i, o);
}

__global__ __launch_bounds__(kPmThreads) void pm_frames_kernel(PmFrameArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kPmThreads + threadIdx.x;
  if (i >= a.n_frames * a.K_max) return;
  const int64_t f = i / a.K_max;
  const int k = (int)(i - f * a.K_max);
  const int n = a.n_pts[f];
  const int st = a.status ? a.status[f] : 0;
  PmPoint o;
  if ((st & kPcStatusSkip) || n < 0 || n > a.K_max || k >= n) {  // the refinement's rule: the frame is not processed, or the slot holds no point
    const double qnan = pm_nan();
    o.info = 0;
    o.n_views = 0;
    for (int e = 0; e < 3; e++) o.sig[e] = o.axis[e] = qnan;
    for (int e = 0; e < 6; e++) o.cov[e] = qnan;
  } else {
    const int16_t* row = a.corr + (size_t)i * a.s.C;
    auto named = [&](int c) -> bool { return row[c] >= 0; };  // (the index itself is not read)
    pm_point(a.s.C, as_ctab(a.s.tab), false, named, a.s.vis, a.s.sigma_px, a.xyz[i * 3], a.xyz[i * 3 + 1], a.xyz[i * 3 + 2], o);
  }
  pm_store(a.s, (size_t)i, o);
}

__global__ __launch_bounds__(64) void pm_summary_init_kernel(int nx, int ny, int nz, long long* s) {
  const int t = threadIdx.x;
  for (int e = t; e < kPmSummary; e += 64) {
    long long v = 0;
    if (e >= kPmBox) {
      const int d = (e - kPmBox) >> 1;
      v = ((e - kPmBox) & 1) ? -1 : (d == 0 ? nx : d == 1 ? ny : nz);
    }
    s[e] = v;
  }
}

__global__ __launch_bounds__(kPmThreads) void pm_map_kernel(PmMapArgs a) {
  __shared__ int s_sum[kPmSummary];  // the workgroup's histogram, GOOD count and box
  const int t = threadIdx.x;
  if (t < kPmSummary) s_sum[t] = t < kPmBox ? 0 : ((t - kPmBox) & 1) ? -1 : 0x7fffffff;
  __syncthreads();
  const int total = a.nx * a.ny * a.nz;  // <= 2^27
  const int lin = (int)blockIdx.x * kPmThreads + t;
  if (lin < total) {
    const int i = lin % a.nx, jk = lin / a.nx, j = jk % a.ny, k = jk / a.ny;
    double x[3];
    for (int d = 0; d < 3; d++) x[d] = ((a.origin[d] + (double)i * a.e0[d]) + (double)j * a.e1[d]) + (double)k * a.e2[d];
    auto named = [](int) -> bool { return false; };
    PmPoint o;
    pm_point(a.s.C, as_ctab(a.s.tab), true, named, a.s.vis, a.s.sigma_px, x[0], x[1], x[2], o);
    a.n_views[lin] = (uint8_t)o.n_views;
    a.sig_max[lin] = (float)o.sig_max;
    if (a.seen) a.seen[lin] = o.seen;
    atomicAdd(&s_sum[o.n_views], 1);
    if (o.info == kPmOk && o.n_views >= a.min_views && o.sig_max <= a.max_sigma) {
      atomicAdd(&s_sum[kPmGood], 1);
      atomicMin(&s_sum[kPmBox + 0], i);
      atomicMax(&s_sum[kPmBox + 1], i);
      atomicMin(&s_sum[kPmBox + 2], j);
      atomicMax(&s_sum[kPmBox + 3], j);
      atomicMin(&s_sum[kPmBox + 4], k);
      atomicMax(&s_sum[kPmBox + 5], k);
    }
  }
  __syncthreads();
  if (t < kPmBox) {
    if (s_sum[t]) atomicAdd(&a.summary[t], (unsigned long long)s_sum[t]);
  } else if (t < kPmSummary && s_sum[kPmGood]) {
    long long* box = (long long*)a.summary;
    if ((t - kPmBox) & 1)
      atomicMax(&box[t], (long long)s_sum[t]);
    else
      atomicMin(&box[t], (long long)s_sum[t]);
  }
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + kPmThreads - 1) / kPmThreads); }

}  // namespace

hipError_t launch_pm_put_table(const double* host, int C, double* dev, hipStream_t stream) {
  for (int c0 = 0; c0 < C; c0 += kPmPutCams) {
    PmTabChunk c{};
    const int count = C - c0 < kPmPutCams ? C - c0 : kPmPutCams;
    for (int i = 0; i < count * 12; i++) c.p[i] = host[12 * c0 + i];
    hipLaunchKernelGGL(pm_put_kernel, dim3(1), dim3(64), 0, stream, c, count, dev + 12 * c0);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

hipError_t launch_pm_points(const PmPointArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(pm_points_kernel, dim3(blocks_of(a.N)), dim3(kPmThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_pm_frames(const PmFrameArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(pm_frames_kernel, dim3(blocks_of(a.n_frames * a.K_max)), dim3(kPmThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_pm_map(const PmMapArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(pm_summary_init_kernel, dim3(1), dim3(64), 0, stream, a.nx, a.ny, a.nz, (long long*)a.summary);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(pm_map_kernel, dim3(blocks_of((int64_t)a.nx * a.ny * a.nz)), dim3(kPmThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
