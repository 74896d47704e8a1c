// jpeg_kernels.hip -- baseline JPEG encoder for the preview stream (reference index.py:55-56: np.hstack of the processed
// frames, then cv.imencode('.jpg')).  The bytes are libjpeg's with its defaults, integer arithmetic throughout (jccolor.c,
// jcsample.c h2v2_downsample, jfdctint.c, jcdctmgr.c, jchuff.c); tests/jpeg_reference.py restates them and is pinned to a
// libjpeg build byte for byte.  Without restart markers an image's scan is one bit string, so the work is cut in four:
//   transform  one wave per 16 x 16 MCU: BGR -> YCbCr, chroma 2 x 2 mean, both DCT passes, quantisation; the six blocks'
//              zigzag coefficients go to HBM, with the coded size of each block's AC part (a lane per coefficient: the run
//              in front of a coefficient is the distance to the next lower set bit of the wave's non-zero ballot)
//   size       one workgroup per image: DC size from the predecessor block's DC (known now, no serial pass), exclusive scan
//              of the blocks' bits, and the words the next pass ORs into are zeroed (only as many as the image needs)
//   emit       one wave per MCU again: every lane writes its codes at its bit offset with atomicOr on 32-bit words --
//              order-independent, so the scan is bit-reproducible
//   stuff      one workgroup per image: 1-padding of the last byte, count of 0xFF bytes per 16-byte piece, scan, copy behind
//              the header with the 0x00s inserted, EOI, size and status; nothing is written at or beyond `capacity`
#include <hip/hip_runtime.h>

#include "../../include/mocap_core.h"
#include "jpeg_tables.hpp"
#include "kernels.hpp"

namespace mocap {

namespace {

constexpr int kMcuWaves = 4;        // MCUs per 256-lane workgroup (transform, emit)
constexpr int kImageThreads = 1024; // size, stuff: one workgroup per image
// a block's 8 x 8 ints are kept with rows of 9: the row pass (lane = block * 8 + row) and the column pass
// (lane = block * 8 + column) then both touch 48 different LDS banks
constexpr int kRowPitch = 9, kBlockPitch = 72;

static __device__ const jpeg::HuffCodes d_huff = jpeg::derive_codes();
static __device__ const jpeg::InvZigzag d_izz = jpeg::derive_inv_zigzag();

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jfdctint.c over d[0..7]: ROWS = pass 1 (results scaled up by 4), else pass 2
template <bool ROWS>
__device__ __forceinline__ void dct_pass(int* d) {
  constexpr int s = ROWS ? 11 : 15;
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  if (ROWS) {
    d[0] = (tmp10 + tmp11) << 2;
    d[4] = (tmp10 - tmp11) << 2;
  } else {
    d[0] = descale(tmp10 + tmp11, 2);
    d[4] = descale(tmp10 - tmp11, 2);
  }
  int z1 = (tmp12 + tmp13) * 4433;
  d[2] = descale(z1 + tmp13 * 6270, s);
  d[6] = descale(z1 - tmp12 * 15137, s);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = descale(t4 + z1 + z3, s);
  d[5] = descale(t5 + z2 + z4, s);
  d[3] = descale(t6 + z2 + z3, s);
  d[1] = descale(t7 + z1 + z4, s);
}

__device__ __forceinline__ int bit_length(int a) { return a ? 32 - __clz(a) : 0; }

// jchuff.c encode_one_block, the part of zigzag position k >= 1 (v = its coefficient, nz = the block's non-zero positions
// without the DC): the ZRLs and the symbol of the run in front of it and its value bits, or the EOB when the block ends in
// zeros (position 63).  bits: the code bits, first bit highest; n <= 59.
__device__ __forceinline__ void ac_code(int v, int k, unsigned long long nz, int tbl, unsigned long long& bits, int& n) {
  bits = 0;
  n = 0;
  if (k == 0) return;
  if (v != 0) {
    const unsigned long long below = nz & ((1ull << k) - 1ull);
    const int prev = below ? 63 - __clzll((long long)below) : 0;
    const int run = k - prev - 1;
    const int size = bit_length(v < 0 ? -v : v);
    const unsigned zrl = d_huff.ac[tbl][0xF0];
    for (int i = 0; i < (run >> 4); i++) {
      bits = bits << (zrl & 255u) | (zrl >> 8);
      n += (int)(zrl & 255u);
    }
    const unsigned c = d_huff.ac[tbl][((run & 15) << 4 | size) & 255];
    bits = bits << (c & 255u) | (c >> 8);
    bits = bits << size | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u));
    n += (int)(c & 255u) + size;
  } else if (k == 63) {
    const unsigned c = d_huff.ac[tbl][0];
    bits = c >> 8;
    n = (int)(c & 255u);
  }
}

__device__ __forceinline__ void dc_code(int diff, int tbl, unsigned long long& bits, int& n) {
  int size = bit_length(diff < 0 ? -diff : diff);
  size = size > 11 ? 11 : size;
  const unsigned c = d_huff.dc[tbl][size];
  bits = (unsigned long long)(c >> 8) << size | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1u));
  n = (int)(c & 255u) + size;
}

// DC of the previous block of the same component (0 at the start of the image): blocks are Y00 Y01 Y10 Y11 Cb Cr per MCU
__device__ __forceinline__ int dc_pred(const int16_t* coef_img, int64_t mcu, int b) {
  if (b >= 1 && b <= 3) return coef_img[(mcu * 6 + b - 1) * 64];
  if (mcu == 0) return 0;
  return coef_img[((mcu - 1) * 6 + (b == 0 ? 3 : b)) * 64];
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ unsigned wave_inclusive_scan(unsigned v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

__global__ __launch_bounds__(kMcuWaves * 64) void jpeg_transform_kernel(JpegArgs a, JpegParams p) {
  __shared__ uint32_t s_raw[kMcuWaves][192];                  // 16 rows x 48 bytes
  __shared__ int s_blk[kMcuWaves][6 * kBlockPitch];
  __shared__ __attribute__((aligned(4))) int16_t s_zz[kMcuWaves][6 * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t n_mcu = (int64_t)a.mcu_x * a.mcu_y;
  const int64_t g = (int64_t)blockIdx.x * kMcuWaves + wv;
  const bool active = g < a.n_images * n_mcu;
  const int64_t f = active ? g / n_mcu : 0, mcu = active ? g - f * n_mcu : 0;
  const int my = (int)(mcu / a.mcu_x), mx = (int)(mcu - (int64_t)my * a.mcu_x);
  const int per_tile = a.W / 16, t = mx / per_tile, tx = mx - t * per_tile;
  const size_t row_bytes = (size_t)a.W * 3;
  const uint8_t* src = a.bgr + (((size_t)f * a.T + t) * a.H + (size_t)my * 16) * row_bytes + (size_t)tx * 48;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const int idx = lane + 64 * j, row = idx / 12, c = idx - row * 12;
    s_raw[wv][idx] = active ? *(const uint32_t*)(src + row * row_bytes + c * 4) : 0u;
  }
  __syncthreads();
  {  // a lane per 2 x 2 quad: four luminance samples and one sample of each chrominance plane
    const uint8_t* rb = (const uint8_t*)s_raw[wv];
    const int qy = lane >> 3, qx = lane & 7;
    int cb = 0, cr = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int y = 2 * qy + (k >> 1), x = 2 * qx + (k & 1);
      const uint8_t* px = rb + y * 48 + x * 3;
      const int B = px[0], G = px[1], R = px[2];
      const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
      cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
      cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
      s_blk[wv][((y >> 3) * 2 + (x >> 3)) * kBlockPitch + (y & 7) * kRowPitch + (x & 7)] = Y - 128;
    }
    const int bias = 1 + (qx & 1);  // 1, 2, 1, 2 along an output row; an MCU starts at an even chroma column
    s_blk[wv][4 * kBlockPitch + qy * kRowPitch + qx] = ((cb + bias) >> 2) - 128;
    s_blk[wv][5 * kBlockPitch + qy * kRowPitch + qx] = ((cr + bias) >> 2) - 128;
  }
  __syncthreads();
  int d[8];
  if (lane < 48) {
    int* row = &s_blk[wv][(lane >> 3) * kBlockPitch + (lane & 7) * kRowPitch];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = row[k];
    dct_pass<true>(d);
#pragma unroll
    for (int k = 0; k < 8; k++) row[k] = d[k];
  }
  __syncthreads();
  if (lane < 48) {
    const int b = lane >> 3, c = lane & 7;
    const int* col = &s_blk[wv][b * kBlockPitch + c];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = col[k * kRowPitch];
    dct_pass<false>(d);
    const uint16_t* q = p.quant[b < 4 ? 0 : 1];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int nat = k * 8 + c, Q = q[nat];
      const int av = d[k] < 0 ? -d[k] : d[k];
      const int qv = (av + 4 * Q) / (8 * Q);
      s_zz[wv][b * 64 + d_izz.at[nat]] = (int16_t)(d[k] < 0 ? -qv : qv);
    }
  }
  __syncthreads();
  if (!active) return;  // no barrier below
  const int64_t blk0 = mcu * 6;
  int16_t* coef_img = a.coef + (size_t)f * n_mcu * 6 * 64;
  uint32_t* dst = (uint32_t*)(coef_img + blk0 * 64);
  const uint32_t* zz32 = (const uint32_t*)s_zz[wv];
#pragma unroll
  for (int j = 0; j < 3; j++) dst[lane + 64 * j] = zz32[lane + 64 * j];
  for (int b = 0; b < 6; b++) {
    const int v = s_zz[wv][b * 64 + lane];
    const unsigned long long nz = __ballot(v != 0) & ~1ull;
    unsigned long long bits;
    int n;
    ac_code(v, lane, nz, b < 4 ? 0 : 1, bits, n);
    n = wave_sum(n);
    if (lane == 0) a.acbits[(size_t)f * n_mcu * 6 + blk0 + b] = n;
  }
}

__global__ __launch_bounds__(kImageThreads) void jpeg_size_kernel(JpegArgs a) {
  __shared__ unsigned s_wave[kImageThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t f = blockIdx.x, n_blk = (int64_t)a.mcu_x * a.mcu_y * 6;
  const int16_t* coef_img = a.coef + (size_t)f * n_blk * 64;
  const int32_t* acb = a.acbits + (size_t)f * n_blk;
  uint32_t* off = a.bitoff + (size_t)f * n_blk;
  unsigned carry = 0;
  for (int64_t base = 0; base < n_blk; base += kImageThreads) {
    const int64_t i = base + tid;
    unsigned n = 0;
    if (i < n_blk) {
      const int64_t mcu = i / 6;
      const int b = (int)(i - mcu * 6);
      unsigned long long bits;
      int nd;
      dc_code(coef_img[i * 64] - dc_pred(coef_img, mcu, b), b < 4 ? 0 : 1, bits, nd);
      n = (unsigned)(acb[i] + nd);
    }
    const unsigned inc = wave_inclusive_scan(n, lane);
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int w = 0; w < kImageThreads / 64; w++) {
      before += w < wv ? s_wave[w] : 0u;
      all += s_wave[w];
    }
    if (i < n_blk) off[i] = carry + before + inc - n;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) a.total_bits[f] = carry;
  // the words the emit pass ORs into, and the whole 16-byte piece the stuff pass reads last
  int64_t n4 = ((int64_t)carry + 31) / 32 / 4 + 1;
  n4 = n4 < a.scan_words / 4 ? n4 : a.scan_words / 4;
  uint4* z = (uint4*)(a.scan + (size_t)f * a.scan_words);
  for (int64_t i = tid; i < n4; i += kImageThreads) z[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(kMcuWaves * 64) void jpeg_emit_kernel(JpegArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t n_mcu = (int64_t)a.mcu_x * a.mcu_y;
  const int64_t g = (int64_t)blockIdx.x * kMcuWaves + wv;
  if (g >= a.n_images * n_mcu) return;  // whole waves leave; no barrier in this kernel
  const int64_t f = g / n_mcu, mcu = g - f * n_mcu;
  const int16_t* coef_img = a.coef + (size_t)f * n_mcu * 6 * 64;
  const uint32_t* off = a.bitoff + (size_t)f * n_mcu * 6;
  uint32_t* words = a.scan + (size_t)f * a.scan_words;
  for (int b = 0; b < 6; b++) {
    const int64_t blk = mcu * 6 + b;
    const int v = coef_img[blk * 64 + lane];
    const int tbl = b < 4 ? 0 : 1;
    const unsigned long long nz = __ballot(v != 0) & ~1ull;
    unsigned long long bits;
    int n;
    if (lane == 0) dc_code(v - dc_pred(coef_img, mcu, b), tbl, bits, n);
    else ac_code(v, lane, nz, tbl, bits, n);
    const unsigned inc = wave_inclusive_scan((unsigned)n, lane);
    if (n == 0) continue;
    const unsigned pos = off[blk] + inc - (unsigned)n;
    const int64_t w = pos >> 5;
    const int s = (int)(pos & 31u);
    const unsigned long long x = bits << (64 - n);   // left-aligned; n is 1..59
    const unsigned long long hi = x >> s;
    const unsigned w0 = (unsigned)(hi >> 32), w1 = (unsigned)hi, w2 = s ? (unsigned)((x << (64 - s)) >> 32) : 0u;
    if (w0 && w < a.scan_words) atomicOr(&words[w], w0);
    if (w1 && w + 1 < a.scan_words) atomicOr(&words[w + 1], w1);
    if (w2 && w + 2 < a.scan_words) atomicOr(&words[w + 2], w2);
  }
}

__global__ __launch_bounds__(kImageThreads) void jpeg_stuff_kernel(JpegArgs a, JpegParams p) {
  __shared__ unsigned s_wave[kImageThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t f = blockIdx.x, cap = a.capacity;
  uint8_t* out = a.out + (size_t)f * a.out_stride;
  const unsigned total = a.total_bits[f];
  const int64_t nb = ((int64_t)total + 7) / 8;  // <= 4 * scan_words
  const unsigned pad = (total & 7u) ? (1u << (8 - (total & 7u))) - 1u : 0u;
  for (int i = tid; i < jpeg::kHeaderBytes; i += kImageThreads)
    if (i < cap) out[i] = p.header[i];
  const uint4* src = (const uint4*)(a.scan + (size_t)f * a.scan_words);
  int64_t stuffed = 0;  // 0x00s inserted so far
  for (int64_t base = 0; base < nb; base += (int64_t)kImageThreads * 16) {
    const int64_t i0 = base + (int64_t)tid * 16;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (i0 < nb) {
      const uint4 q = src[i0 >> 4];
      w[0] = q.x;
      w[1] = q.y;
      w[2] = q.z;
      w[3] = q.w;
    }
    if (i0 <= nb - 1 && nb - 1 < i0 + 16) {
      const int j = (int)(nb - 1 - i0);
      w[j >> 2] |= pad << (24 - 8 * (j & 3));
    }
    unsigned cnt = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) cnt += (i0 + j < nb && ((w[j >> 2] >> (24 - 8 * (j & 3))) & 255u) == 255u) ? 1u : 0u;
    const unsigned inc = wave_inclusive_scan(cnt, lane);
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int k = 0; k < kImageThreads / 64; k++) {
      before += k < wv ? s_wave[k] : 0u;
      all += s_wave[k];
    }
    int64_t pos = jpeg::kHeaderBytes + i0 + stuffed + before + inc - cnt;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const unsigned byte = (w[j >> 2] >> (24 - 8 * (j & 3))) & 255u;
      if (i0 + j < nb) {
        if (pos < cap) out[pos] = (uint8_t)byte;
        pos++;
        if (byte == 255u) {
          if (pos < cap) out[pos] = 0;
          pos++;
        }
      }
    }
    stuffed += all;
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t size = jpeg::kHeaderBytes + nb + stuffed + 2;
    if (size - 2 < cap) out[size - 2] = 0xff;
    if (size - 1 < cap) out[size - 1] = 0xd9;
    a.sizes[f] = size;
    a.status[f] = size > cap ? MOCAP_JPEG_ST_OVERFLOW : 0;
  }
}

__global__ __launch_bounds__(256) void jpeg_export_kernel(const uint8_t* src, int64_t src_stride, const int64_t* sizes,
                                                          int64_t capacity, uint8_t* dst, int64_t dst_stride, int64_t* dst_sizes) {
  const int64_t f = blockIdx.y;
  const int64_t size = sizes[f], n = size < capacity ? size : capacity;
  if (blockIdx.x == 0 && threadIdx.x == 0) dst_sizes[f] = size;
  const uint4* s = (const uint4*)(src + (size_t)f * src_stride);
  uint4* d = (uint4*)(dst + (size_t)f * dst_stride);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i * 16 < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = s[i];
}

}  // namespace

hipError_t launch_jpeg_encode(const JpegArgs& a, const JpegParams& p, hipStream_t stream) {
  if (a.n_images <= 0) return hipSuccess;
  const int64_t mcus = a.n_images * a.mcu_x * a.mcu_y, groups = (mcus + kMcuWaves - 1) / kMcuWaves;
  if (groups > 0x7fffffff || a.n_images > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)groups), dim3(kMcuWaves * 64), 0, stream, a, p);
  hipLaunchKernelGGL(jpeg_size_kernel, dim3((unsigned)a.n_images), dim3(kImageThreads), 0, stream, a);
  hipLaunchKernelGGL(jpeg_emit_kernel, dim3((unsigned)groups), dim3(kMcuWaves * 64), 0, stream, a);
  hipLaunchKernelGGL(jpeg_stuff_kernel, dim3((unsigned)a.n_images), dim3(kImageThreads), 0, stream, a, p);
  return hipGetLastError();
}

hipError_t launch_jpeg_export(int64_t n_images, const uint8_t* src, int64_t src_stride, const int64_t* sizes, int64_t capacity,
                              uint8_t* dst, int64_t dst_stride, int64_t* dst_sizes, hipStream_t stream) {
  if (n_images <= 0) return hipSuccess;
  if (n_images > 65535) return hipErrorInvalidValue;
  const int64_t pieces = (capacity + 15) / 16, want = (pieces + 255) / 256;
  hipLaunchKernelGGL(jpeg_export_kernel, dim3((unsigned)(want < 64 ? (want < 1 ? 1 : want) : 64), (unsigned)n_images), dim3(256), 0,
                     stream, src, src_stride, sizes, capacity, dst, dst_stride, dst_sizes);
  return hipGetLastError();
}

}  // namespace mocap
