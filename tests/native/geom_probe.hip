// geom_probe.hip -- TEST-ONLY (tests/native/Makefile -> tests/native/libmocap_geomprobe.so, loaded with ctypes by
// tests/test_gpu_geom_kernels.py): per-sample access to the FP64 geometry core that every kernel of the hot path inlines
// (csrc/mocap_device.hpp: rsqrt_pos, recip_refined, div_by, smallest_eigvec4, eigcut_s1, eigcut_s1_shifted, solve_point).
// It includes the product's own header with the product's flags, so the arithmetic it runs is the arithmetic the frame
// kernels run; the product ABI (include/mocap_core.h) does not grow for tests.
//
// One lane per sample, blocks of 64 lanes.  Every entry point works on host buffers: allocate, copy in, launch, copy back,
// free.  OUTPUT buffers make the round trip too (uploaded before the launch, downloaded after it), so a caller that fills
// them with a sentinel sees which elements the kernel wrote.  Return value: 0, or minus the HIP error code, or -100000
// for a bad argument.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../low-cost-mocap_amd/csrc/mocap_device.hpp"

namespace {

constexpr int kBadArg = -100000;

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

// op: 0 = rsqrt_pos(b), 1 = recip_refined(b), 2 = div_by(a, b, recip_refined(b))
__global__ __launch_bounds__(64) void scalar_probe_kernel(int n, int op, const double* a, const double* b, double* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double y = b[i];
  out[i] = op == 0 ? mocap::rsqrt_pos(y) : op == 1 ? mocap::recip_refined(y) : mocap::div_by(a[i], y, mocap::recip_refined(y));
}

__global__ __launch_bounds__(64) void eigvec4_probe_kernel(int n, const double* a, const double* lamcut, double* vec, double* lam_lb,
                                                           int32_t* ok) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double B[10], v[4], lb;
  for (int k = 0; k < 10; k++) B[k] = a[(size_t)i * 10 + k];
  const bool r = mocap::smallest_eigvec4(B, v, lamcut[i], lb);
  ok[i] = r ? 1 : 0;
  if (r) {
    for (int k = 0; k < 4; k++) vec[(size_t)i * 4 + k] = v[k];
    lam_lb[i] = lb;
  }
}

__global__ __launch_bounds__(64) void eigcut_probe_kernel(int n, const double* a, const double* c, double* s1, double* tr) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double B[10], t;
  for (int k = 0; k < 10; k++) B[k] = a[(size_t)i * 10 + k];
  if (c) {
    const double cc[3] = {c[(size_t)i * 3], c[(size_t)i * 3 + 1], c[(size_t)i * 3 + 2]};
    s1[i] = mocap::eigcut_s1_shifted(B, cc, t);
  } else {
    s1[i] = mocap::eigcut_s1(B, t);
  }
  tr[i] = t;
}

__global__ __launch_bounds__(64) void solve_point_probe_kernel(int n, const double* a, double* X) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double B[10], x[3];
  for (int k = 0; k < 10; k++) B[k] = a[(size_t)i * 10 + k];
  mocap::solve_point(B, x);
  for (int k = 0; k < 3; k++) X[(size_t)i * 3 + k] = x[k];
}

int scalar_probe(int n, int op, const double* a, const double* b, double* out) {
  if (n < 1 || !b || !out || (op == 2 && !a)) return kBadArg;
  const size_t bytes = sizeof(double) * (size_t)n;
  DevMem da, db, dout;
  if (a) PROBE_TRY(da.up(a, bytes));
  PROBE_TRY(db.up(b, bytes));
  PROBE_TRY(dout.up(out, bytes));
  hipLaunchKernelGGL(scalar_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, op, da.as<double>(), db.as<double>(),
                     dout.as<double>());
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(dout.down(out, bytes));
  return 0;
}

}  // namespace

extern "C" int geomprobe_rsqrt(int n, const double* d, double* out) { return scalar_probe(n, 0, nullptr, d, out); }
extern "C" int geomprobe_recip(int n, const double* b, double* out) { return scalar_probe(n, 1, nullptr, b, out); }
extern "C" int geomprobe_div(int n, const double* a, const double* b, double* out) { return scalar_probe(n, 2, a, b, out); }

// a [n][10] packed like mocap::sidx, lamcut [n] -> vec [n][4], lam_lb [n] (both untouched where the call returns false), ok [n]
extern "C" int geomprobe_eigvec4(int n, const double* a, const double* lamcut, double* vec, double* lam_lb, int32_t* ok) {
  if (n < 1 || !a || !lamcut || !vec || !lam_lb || !ok) return kBadArg;
  DevMem da, dc, dv, dl, dk;
  PROBE_TRY(da.up(a, sizeof(double) * 10 * (size_t)n));
  PROBE_TRY(dc.up(lamcut, sizeof(double) * (size_t)n));
  PROBE_TRY(dv.up(vec, sizeof(double) * 4 * (size_t)n));
  PROBE_TRY(dl.up(lam_lb, sizeof(double) * (size_t)n));
  PROBE_TRY(dk.up(ok, sizeof(int32_t) * (size_t)n));
  hipLaunchKernelGGL(eigvec4_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, da.as<double>(), dc.as<double>(),
                     dv.as<double>(), dl.as<double>(), dk.as<int32_t>());
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(dv.down(vec, sizeof(double) * 4 * (size_t)n));
  PROBE_TRY(dl.down(lam_lb, sizeof(double) * (size_t)n));
  PROBE_TRY(dk.down(ok, sizeof(int32_t) * (size_t)n));
  return 0;
}

// a [n][10], c [n][3] or null (null: eigcut_s1, else eigcut_s1_shifted) -> s1 [n], tr [n]
extern "C" int geomprobe_eigcut(int n, const double* a, const double* c_or_null, double* s1, double* tr) {
  if (n < 1 || !a || !s1 || !tr) return kBadArg;
  DevMem da, dc, ds, dt;
  PROBE_TRY(da.up(a, sizeof(double) * 10 * (size_t)n));
  if (c_or_null) PROBE_TRY(dc.up(c_or_null, sizeof(double) * 3 * (size_t)n));
  PROBE_TRY(ds.up(s1, sizeof(double) * (size_t)n));
  PROBE_TRY(dt.up(tr, sizeof(double) * (size_t)n));
  hipLaunchKernelGGL(eigcut_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, da.as<double>(),
                     c_or_null ? dc.as<double>() : (const double*)nullptr, ds.as<double>(), dt.as<double>());
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(ds.down(s1, sizeof(double) * (size_t)n));
  PROBE_TRY(dt.down(tr, sizeof(double) * (size_t)n));
  return 0;
}

// a [n][10] -> X [n][3]
extern "C" int geomprobe_solve_point(int n, const double* a, double* X) {
  if (n < 1 || !a || !X) return kBadArg;
  DevMem da, dx;
  PROBE_TRY(da.up(a, sizeof(double) * 10 * (size_t)n));
  PROBE_TRY(dx.up(X, sizeof(double) * 3 * (size_t)n));
  hipLaunchKernelGGL(solve_point_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, n, da.as<double>(), dx.as<double>());
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(dx.down(X, sizeof(double) * 3 * (size_t)n));
  return 0;
}
