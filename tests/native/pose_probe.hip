// pose_probe.hip -- TEST-ONLY (tests/native/Makefile -> tests/native/libmocap_poseprobe.so, loaded with ctypes by
// tests/test_gpu_pose_kernels.py): per-sample and per-model access to the device routines of the initial pose
// estimation.  It includes the product's own header (csrc/pose_kernels.hpp) and goes through the product's own
// launchers, so what it runs is what lib/libmocap_core.so runs between the host steps of its RANSAC replay; the
// product ABI (include/mocap_core.h) does not grow for tests.
//
// Every entry point works on host buffers: allocate, copy in, launch, copy back, free.  OUTPUT buffers make the round
// trip too (uploaded before the launch, downloaded after it), so a caller that fills them with a sentinel sees which
// elements the kernel wrote.  Return value: 0, or minus the HIP error code, or -100000 for a bad argument.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../low-cost-mocap_amd/csrc/pose_kernels.hpp"

namespace {

constexpr int kBadArg = -100000;
constexpr int kMaskGuard = 16;  // bytes after the mask's N that make the round trip with it

struct DevMem {  // frees on every return path
  void* p = nullptr;
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
  hipError_t up(const void* host, size_t bytes) {
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e == hipSuccess && bytes) e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
    return e;
  }
  hipError_t down(void* host, size_t bytes) const { return bytes ? hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

#define PROBE_TRY(expr)                      \
  do {                                       \
    hipError_t e__ = (expr);                 \
    if (e__ != hipSuccess) return -(int)e__; \
  } while (0)

__global__ __launch_bounds__(64) void cubic_probe_kernel(int n, const double* c, double* x, int32_t* nx) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double cf[4], r[3];
  for (int k = 0; k < 4; k++) cf[k] = c[(size_t)i * 4 + k];
  const int m = mocap::real_cubic_roots(cf, r);
  for (int k = 0; k < m; k++) x[(size_t)i * 3 + k] = r[k];
  nx[i] = m;
}

}  // namespace

extern "C" int poseprobe_mask_guard(void) { return kMaskGuard; }

// idx [n_samples][7] into the n_pts correspondences; F_out [n_slots][3][9] and nF_out [n_slots] with n_slots >= n_samples:
// the buffers' capacity, all of which is uploaded and downloaded (slots >= n_samples must come back as they went in)
extern "C" int poseprobe_seven_point(int device, int n_pts, const float* p1, const float* p2, int n_samples, const int32_t* idx,
                                     int n_slots, double* F_out, int32_t* nF_out) {
  if (n_pts < 1 || n_samples < 0 || n_slots < n_samples || n_slots < 1 || !p1 || !p2 || !idx || !F_out || !nF_out) return kBadArg;
  for (size_t i = 0; i < (size_t)n_samples * 7; i++)
    if (idx[i] < 0 || idx[i] >= n_pts) return kBadArg;
  PROBE_TRY(hipSetDevice(device));
  DevMem d1, d2, di, dF, dn;
  PROBE_TRY(d1.up(p1, sizeof(float) * 2 * (size_t)n_pts));
  PROBE_TRY(d2.up(p2, sizeof(float) * 2 * (size_t)n_pts));
  PROBE_TRY(di.up(idx, sizeof(int32_t) * 7 * (size_t)n_samples));
  PROBE_TRY(dF.up(F_out, sizeof(double) * 27 * (size_t)n_slots));
  PROBE_TRY(dn.up(nF_out, sizeof(int32_t) * (size_t)n_slots));
  if (n_samples > 0) {
    mocap::SevenArgs a{n_samples, di.as<int32_t>(), d1.as<float>(), d2.as<float>(), dF.as<double>(), dn.as<int32_t>()};
    mocap::launch_seven_point(a, nullptr);
    PROBE_TRY(hipGetLastError());
  }
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(dF.down(F_out, sizeof(double) * 27 * (size_t)n_slots));
  PROBE_TRY(dn.down(nF_out, sizeof(int32_t) * (size_t)n_slots));
  return 0;
}

// F [n_models][9]; nF [(n_models + 2) / 3] or null; t = (float)(thr * thr); count_out [n_models];
// mask [n_pts + poseprobe_mask_guard()] or null
extern "C" int poseprobe_score(int device, int n_pts, const float* p1, const float* p2, int n_models, const double* F,
                               const int32_t* nF_or_null, float t, int32_t* count_out, uint8_t* mask_or_null) {
  if (n_pts < 1 || n_models < 1 || !p1 || !p2 || !F || !count_out) return kBadArg;
  PROBE_TRY(hipSetDevice(device));
  DevMem d1, d2, dF, dn, dc, dm;
  PROBE_TRY(d1.up(p1, sizeof(float) * 2 * (size_t)n_pts));
  PROBE_TRY(d2.up(p2, sizeof(float) * 2 * (size_t)n_pts));
  PROBE_TRY(dF.up(F, sizeof(double) * 9 * (size_t)n_models));
  if (nF_or_null) PROBE_TRY(dn.up(nF_or_null, sizeof(int32_t) * (((size_t)n_models + 2) / 3)));
  PROBE_TRY(dc.up(count_out, sizeof(int32_t) * (size_t)n_models));
  if (mask_or_null) PROBE_TRY(dm.up(mask_or_null, (size_t)n_pts + kMaskGuard));
  mocap::ScoreArgs a{n_pts, d1.as<float>(), d2.as<float>(), dF.as<double>(), nF_or_null ? dn.as<int32_t>() : nullptr, t,
                     dc.as<int32_t>(), mask_or_null ? dm.as<uint8_t>() : nullptr};
  mocap::launch_score(a, n_models, nullptr);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(dc.down(count_out, sizeof(int32_t) * (size_t)n_models));
  if (mask_or_null) PROBE_TRY(dm.down(mask_or_null, (size_t)n_pts + kMaskGuard));
  return 0;
}

// coeffs [n][4] (c0 x^3 + c1 x^2 + c2 x + c3) -> roots_out [n][3] (the first nroots_out[i] are written), nroots_out [n]
extern "C" int poseprobe_cubic(int device, int n, const double* coeffs, double* roots_out, int32_t* nroots_out) {
  if (n < 1 || !coeffs || !roots_out || !nroots_out) return kBadArg;
  PROBE_TRY(hipSetDevice(device));
  DevMem dc, dx, dn;
  PROBE_TRY(dc.up(coeffs, sizeof(double) * 4 * (size_t)n));
  PROBE_TRY(dx.up(roots_out, sizeof(double) * 3 * (size_t)n));
  PROBE_TRY(dn.up(nroots_out, sizeof(int32_t) * (size_t)n));
  hipLaunchKernelGGL(cubic_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, dc.as<double>(), dx.as<double>(), dn.as<int32_t>());
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(dx.down(roots_out, sizeof(double) * 3 * (size_t)n));
  PROBE_TRY(dn.down(nroots_out, sizeof(int32_t) * (size_t)n));
  return 0;
}
