// blob_centroid.hip -- sub-pixel blob centroids (MOCAP_CENTROID_WEIGHTED; contract: include/mocap_core.h).
// The reference's centroid is int(m10 / m00) of the contour polygon (helpers.py:152-155): most of a pixel is gone before the
// FP64 geometry sees the point.  Behind the contour pass, every kept slot is overwritten with the grey-weighted centroid of
// the mask pixels inside its contour's bounding box:
//     w = grey - 51 (1 .. 204) for the pixels whose mask bit is on;  x = (double)sum(w x) / (double)sum(w), rounded once to float
// The three sums are exact integers, so the value does not depend on how the lanes split the window: it is bit-reproducible
// and equals the NumPy statement of tests/subpixel_reference.py.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace mocap {

namespace {
constexpr int kCentroidThreads = 256;
}  // namespace

// One workgroup per image, one wave per kept slot (waves stride over the slots).  The lanes stride over the window's
// (row, 64-bit mask word) items; a word's set bits inside [x0, x1] are iterated and their grey bytes read.  Per word the sums
// fit 32 bits (64 x 204 x 831 < 2^24); across words they are kept in 64 bits (one saturated 320 x 320 picture:
// sum(w x) = 3.3e9).  No atomics, no floating-point accumulation: a shuffle tree over the wave, lane 0 divides and stores.
// Grey bytes are read only where the mask bit is on -- tiles the dark-tile early-out skipped were never written.
__global__ __launch_bounds__(kCentroidThreads) void blob_weighted_centroid_kernel(BlobArgs a) {
  const int64_t img = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = a.S, words = (S + 63) / 64;
  int n = a.counts[img];  // 0 for a picture with BLOB_ST_CAP_OVERFLOW_
  n = n < 0 ? 0 : (n > a.M_max ? a.M_max : n);
  const unsigned long long* mask = a.mask + (size_t)img * S * words;
  const uint8_t* grey = a.grey + (size_t)img * S * S;
  for (int slot = wave; slot < n; slot += kCentroidThreads / 64) {
    const int16_t* b = a.bbox + ((size_t)img * a.M_max + slot) * 4;
    // (the clamps hold for every box the contour pass writes; they keep a stale box from reading outside the planes)
    const int x0 = max((int)b[0], 0), y0 = max((int)b[1], 0), x1 = min((int)b[2], S - 1), y1 = min((int)b[3], S - 1);
    const int w0 = x0 >> 6, nw = (x1 >> 6) - w0 + 1;
    unsigned long long sw = 0, swx = 0, swy = 0;
    const int items = (y1 >= y0 && nw > 0) ? (y1 - y0 + 1) * nw : 0;
    for (int i = lane; i < items; i += 64) {
      const int y = y0 + i / nw, w = w0 + i % nw;
      unsigned long long bits = mask[(size_t)y * words + w];
      if (w == w0) bits &= ~0ull << (x0 & 63);
      if (w == x1 >> 6) bits &= ~0ull >> (63 - (x1 & 63));
      const uint8_t* row = grey + (size_t)y * S + w * 64;
      uint32_t s = 0, sx = 0;
      while (bits) {
        const int k = __builtin_ctzll(bits);
        bits &= bits - 1;
        const uint32_t wt = (uint32_t)row[k] - (uint32_t)kGreyThreshold;
        s += wt;
        sx += wt * (uint32_t)(w * 64 + k);
      }
      sw += s;
      swx += sx;
      swy += (unsigned long long)s * (uint32_t)y;
    }
    for (int o = 32; o > 0; o >>= 1) {
      sw += __shfl_down(sw, o);
      swx += __shfl_down(swx, o);
      swy += __shfl_down(swy, o);
    }
    if (lane == 0 && sw) {  // (sum(w) > 0: the contour's own pixels are on)
      float* out = a.blobs + ((size_t)img * a.M_max + slot) * 2;
      out[0] = (float)((double)swx / (double)sw);
      out[1] = (float)((double)swy / (double)sw);
    }
  }
}

hipError_t launch_blob_weighted_centroids(const BlobArgs& a, hipStream_t stream) {
  if (a.n_images <= 0) return hipSuccess;
  if (a.n_images > 0x7fffffffll || !a.grey || !a.bbox) return hipErrorInvalidValue;
  hipLaunchKernelGGL(blob_weighted_centroid_kernel, dim3((unsigned)a.n_images), dim3(kCentroidThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
