// overlay_kernels.hip -- the drawings of the reference's preview, painted into the blob stage's `processed` frames where
// they lie ([n][S][S][3] uint8 BGR): every contour pixel green (cv.drawContours, helpers.py:148), a filled radius-1 circle on
// every centroid (cv.circle, helpers.py:157) and one epipolar line per point and later camera (drawlines, helpers.py:365).
// Sparse byte stores over data the stages before have left on the device: the 1-bit mask, the centroids, the frame path's
// correspondences and the F table.  Contracts: DESIGN.md 3.7e.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace mocap {

namespace {

constexpr int kOverlayThreads = 256;
constexpr int kOverlayRows = 32;  // rows of one picture per workgroup of the contour / mark kernel

__device__ __forceinline__ void paint(uint8_t* pic, int S, int y, int x, uint32_t bgr) {
  uint8_t* p = pic + ((size_t)y * S + x) * 3;
  p[0] = (uint8_t)bgr;
  p[1] = (uint8_t)(bgr >> 8);
  p[2] = (uint8_t)(bgr >> 16);
}

// B | G << 8 | R << 16
constexpr uint32_t kContourColour = 0x00ff00u;  // (0, 255, 0)
constexpr uint32_t kMarkColour = 0x64ff64u;     // (100, 255, 100)
__constant__ uint32_t kLinePalette[6] = {0x0000ffu, 0xff0000u, 0x00ffffu, 0xff00ffu, 0xffff00u, 0x0080ffu};

}  // namespace

// One workgroup per (picture, band of kOverlayRows rows).  Contours: a pixel some border trace of findContours visits is a
// mask pixel with one of its four edge neighbours off (the outside of the picture counts as off); one pass over the band's
// mask words with the neighbours shifted in, set bits iterated.  Marks: the pixel and its four edge neighbours of every
// stored centroid, clipped to the picture; each band paints the mark pixels that fall into it, after its contours.
__global__ __launch_bounds__(kOverlayThreads) void overlay_blobs_kernel(OverlayArgs a) {
  const int tid = threadIdx.x;
  const int S = a.S, words = (S + 63) / 64;
  const int bands = (S + kOverlayRows - 1) / kOverlayRows;
  const int64_t img = blockIdx.x / bands;
  const int band = (int)(blockIdx.x - img * bands);
  if (a.status[img] & BLOB_ST_CAP_OVERFLOW_) return;  // no contours were produced for this picture: left undrawn
  const int y0 = band * kOverlayRows, y1 = min(S, y0 + kOverlayRows);
  uint8_t* pic = a.bgr + (size_t)img * S * S * 3;
  if (a.flags & kOverlayContours) {
    const unsigned long long* m = a.mask + (size_t)img * S * words;
    for (int i = tid; i < (y1 - y0) * words; i += kOverlayThreads) {
      const int y = y0 + i / words, w = i % words;
      const unsigned long long* row = m + (size_t)y * words;
      const unsigned long long c = row[w];
      if (!c) continue;
      const unsigned long long up = y > 0 ? row[w - words] : 0ull, dn = y + 1 < S ? row[w + words] : 0ull;
      const unsigned long long left = (c << 1) | (w > 0 ? row[w - 1] >> 63 : 0ull);
      const unsigned long long right = (c >> 1) | (w + 1 < words ? row[w + 1] << 63 : 0ull);  // bits beyond column S - 1 are zero
      unsigned long long e = c & ~(up & dn & left & right);
      while (e) {
        const int x = w * 64 + __builtin_ctzll(e);
        e &= e - 1;
        if (x < S) paint(pic, S, y, x, kContourColour);
      }
    }
  }
  if (a.flags & kOverlayCentres) {
    __syncthreads();  // marks go over the band's contours
    int n = a.counts[img];
    n = n < 0 ? 0 : (n > a.M_max ? a.M_max : n);
    const float* pts = a.blobs + (size_t)img * a.M_max * 2;
    for (int i = tid; i < n * 5; i += kOverlayThreads) {
      const int p = i / 5, j = i - p * 5;
      const int x = (int)pts[2 * p] + (j == 1 ? -1 : (j == 2 ? 1 : 0));
      const int y = (int)pts[2 * p + 1] + (j == 3 ? -1 : (j == 4 ? 1 : 0));
      if (x >= 0 && x < S && y >= y0 && y < y1) paint(pic, S, y, x, kMarkColour);
    }
  }
}

hipError_t launch_overlay_blobs(const OverlayArgs& a, hipStream_t stream) {
  if (a.n_images <= 0 || !(a.flags & (kOverlayContours | kOverlayCentres))) return hipSuccess;
  const int64_t grid = a.n_images * ((a.S + kOverlayRows - 1) / kOverlayRows);
  if (grid > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(overlay_blobs_kernel, dim3((unsigned)grid), dim3(kOverlayThreads), 0, stream, a);
  return hipGetLastError();
}

// One workgroup per picture (frame f, camera i).  For every output point k of the frame, in ascending k: the point's root
// camera r is the lowest one with a correspondence; for i > r the line is computeCorrespondEpilines of the root's blob under
// F[r][i], as the frame kernels form it (epiline_wide, csrc/frame_kernel.hip).  A lane owns a column (|b| >= |a|) or a row
// of the picture; the barrier after each line keeps the order of the lines -- a pixel ends with the colour of the largest
// k covering it -- although consecutive lines may be walked along different axes.  Every branch around the barrier depends
// on (f, i, k) alone.
__global__ __launch_bounds__(kOverlayThreads) void overlay_epilines_kernel(EpilineArgs a) {
  const int tid = threadIdx.x;
  const int C = a.C, S = a.S;
  const int64_t f = blockIdx.x / C;
  const int i = (int)(blockIdx.x - f * C);
  if (a.status[f] != 0) return;
  int n = a.n_pts[f];
  n = n < 0 ? 0 : (n > a.K_max ? a.K_max : n);
  uint8_t* pic = a.bgr + ((size_t)f * C + i) * S * S * 3;
  for (int k = 0; k < n; k++) {
    const int16_t* ck = a.corr + ((size_t)f * a.K_max + k) * C;
    int r = 0;
    while (r < i && ck[r] < 0) r++;
    if (r >= i) continue;  // the root's camera is this one or a later one
    const int rb = ck[r];
    int cnt = a.counts[(size_t)f * C + r];
    cnt = cnt > a.M_max ? a.M_max : cnt;
    if (rb >= cnt) continue;
    const float* rp = a.blobs + (((size_t)f * C + r) * a.M_max + rb) * 2;
    const double* Fm = a.F + 9 * ((size_t)r * C + i);
    const double px = (double)rp[0], py = (double)rp[1];
    double la = Fm[0] * px + Fm[1] * py + Fm[2];
    double lb = Fm[3] * px + Fm[4] * py + Fm[5];
    double lc = Fm[6] * px + Fm[7] * py + Fm[8];
    double nu = la * la + lb * lb;
    nu = nu != 0.0 ? 1.0 / sqrt(nu) : 1.0;
    la *= nu;
    lb *= nu;
    lc *= nu;
    if (a.f32_rounding) {
      la = (double)(float)la;
      lb = (double)(float)lb;
      lc = (double)(float)lc;
    }
    const uint32_t colour = kLinePalette[k % 6];
    const double edge = (double)S;
    if (fabs(lb) >= fabs(la) && lb != 0.0) {
      for (int x = tid; x < S; x += kOverlayThreads) {
        const double y = rint(-(la * (double)x + lc) / lb);
        if (y >= 0.0 && y < edge) paint(pic, S, (int)y, x, colour);
      }
    } else if (la != 0.0) {
      for (int y = tid; y < S; y += kOverlayThreads) {
        const double x = rint(-(lb * (double)y + lc) / la);
        if (x >= 0.0 && x < edge) paint(pic, S, y, (int)x, colour);
      }
    } else {
      continue;
    }
    __syncthreads();
  }
}

hipError_t launch_overlay_epilines(const EpilineArgs& a, hipStream_t stream) {
  if (a.n_frames <= 0) return hipSuccess;
  const int64_t grid = a.n_frames * a.C;
  if (grid > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(overlay_epilines_kernel, dim3((unsigned)grid), dim3(kOverlayThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
