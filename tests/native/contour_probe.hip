// contour_probe.hip -- TEST-ONLY (tests/native/Makefile -> tests/native/libmocap_contourprobe.so, loaded with ctypes by
// tests/test_gpu_contour_kernel.py): the product's own launch_blob_contours on caller-supplied 1-bit masks, so that the
// contour kernel can be pinned on crafted masks instead of on what a blurred camera frame leaves of them.  The product's
// csrc/blob_kernels.hip is compiled into this library as it stands (no copy of the kernel text) with the product's flags;
// the product ABI (include/mocap_core.h) does not grow for tests.  No torch, no mocap context.
//
// contourprobe_run works on host buffers.  blobs, counts, status, n_contours and bbox are IN/OUT: uploaded before the launch
// and downloaded after it, so a caller that fills them with a sentinel sees what the kernel wrote, and a second call with
// only_overflowed = 1 plays the product's "run again what overflowed" pass on the first call's status.
// Return value: 0, or minus the HIP error code, or -100000 for an argument the probe or the product's launcher refuses.
#include <string.h>

#include "../../low-cost-mocap_amd/csrc/blob_kernels.hip"

namespace {

constexpr int kBadArg = -100000;
constexpr size_t kLdsCap = 160 * 1024;  // what csrc/blob_capi.hip sizes the tables for

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
};

#define PROBE_TRY(expr)                      \
  do {                                       \
    hipError_t e__ = (expr);                 \
    if (e__ != hipSuccess) return -(int)e__; \
  } while (0)

}  // namespace

extern "C" {

size_t contourprobe_lds_bytes(int S, int P_cap, int N_cap) { return mocap::blob_contour_lds_bytes(S, P_cap, N_cap); }

// masks   u64 [n_images][S][ceil(S / 64)]: bit x of word x / 64, bits at x >= S zero (refused otherwise: the kernel relies on it)
// blobs   f32 [n_images][M_max][2], counts / status / n_contours i32 [n_images], bbox i16 [n_images][M_max][4] (read only
//         with want_bbox; may be null without)
int contourprobe_run(int S, int64_t n_images, const uint64_t* masks, int M_max, int P_cap, int N_cap, int only_overflowed,
                     int want_bbox, float* blobs, int32_t* counts, int32_t* status, int32_t* n_contours, int16_t* bbox) {
  if (S < 1 || S > mocap::kBlobMaxEdge || n_images < 1 || n_images > (1 << 20) || M_max < 1 || M_max > 32767) return kBadArg;
  if (P_cap < 1 || P_cap > 65535 || N_cap < 1 || N_cap > P_cap) return kBadArg;  // 16-bit links
  if (!masks || !blobs || !counts || !status || !n_contours || (want_bbox && !bbox)) return kBadArg;
  if (want_bbox && 4 * N_cap > P_cap) return kBadArg;  // the launcher's own refusal
  if (mocap::blob_contour_lds_bytes(S, P_cap, N_cap) > kLdsCap) return kBadArg;
  const int words = (S + 63) / 64;
  if (S % 64) {
    const uint64_t beyond = ~0ull << (S % 64);
    for (int64_t r = 0; r < n_images * S; r++)
      if (masks[(size_t)r * words + words - 1] & beyond) return kBadArg;
  }
  const size_t n = (size_t)n_images;
  DevMem d_mask, d_blobs, d_counts, d_status, d_nc, d_bbox;
  PROBE_TRY(d_mask.up(masks, n * S * words * sizeof(uint64_t)));
  PROBE_TRY(d_blobs.up(blobs, n * M_max * 2 * sizeof(float)));
  PROBE_TRY(d_counts.up(counts, n * sizeof(int32_t)));
  PROBE_TRY(d_status.up(status, n * sizeof(int32_t)));
  PROBE_TRY(d_nc.up(n_contours, n * sizeof(int32_t)));
  if (want_bbox) PROBE_TRY(d_bbox.up(bbox, n * M_max * 4 * sizeof(int16_t)));
  mocap::BlobArgs a;
  memset(&a, 0, sizeof a);
  a.n_images = n_images;
  a.C = 1;
  a.S = S;
  a.M_max = M_max;
  a.mask = (unsigned long long*)d_mask.p;
  a.blobs = (float*)d_blobs.p;
  a.counts = (int32_t*)d_counts.p;
  a.status = (int32_t*)d_status.p;
  a.n_contours = (int32_t*)d_nc.p;
  a.bbox = want_bbox ? (int16_t*)d_bbox.p : nullptr;
  PROBE_TRY(mocap::launch_blob_contours(a, P_cap, N_cap, only_overflowed ? 1 : 0, nullptr));
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(d_blobs.down(blobs, n * M_max * 2 * sizeof(float)));
  PROBE_TRY(d_counts.down(counts, n * sizeof(int32_t)));
  PROBE_TRY(d_status.down(status, n * sizeof(int32_t)));
  PROBE_TRY(d_nc.down(n_contours, n * sizeof(int32_t)));
  if (want_bbox) PROBE_TRY(d_bbox.down(bbox, n * M_max * 4 * sizeof(int16_t)));
  return 0;
}

}  // extern "C"
