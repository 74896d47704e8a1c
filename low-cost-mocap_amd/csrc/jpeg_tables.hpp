// jpeg_tables.hpp -- what the baseline JPEG encoder (jpeg_kernels.hip, jpeg_capi.hip) shares between host and device: the
// Annex-K tables, the Huffman codes derived from them at compile time, and the host-only parts of the C ABI (quantisation
// tables of a quality, the 623 header bytes, the size bound, the argument checks).  Plain C++17 with no HIP in it, so that the
// host parts can be built into a stand-alone program and run under a sanitizer (tests/native/jpeg_host_check.cpp).
// The stream is the one libjpeg writes with its defaults (cv.imencode('.jpg'), reference index.py:56): baseline sequential,
// YCbCr 4:2:0, JDCT_ISLOW, standard Huffman tables, no restart markers, JFIF 1.01 APP0 with density 1:1.
#pragma once
#include <cstdint>
#include <cstring>
#include <initializer_list>

namespace mocap {
namespace jpeg {

constexpr int kHeaderBytes = 623;  // SOI 2 | APP0 18 | DQT 69 + 69 | SOF0 19 | DHT 33 + 183 + 33 + 183 | SOS 14
constexpr int kBlocksPerMcu = 6;   // Y00 Y01 Y10 Y11 Cb Cr
// Bits one coded block can take: DC = code (<= 11 bits, chrominance category 11) + 11 value bits; each of the 63 AC
// coefficients = code (<= 16 bits) + 10 value bits.  A zero run only shortens this (a ZRL symbol is 11 bits for 16 zeros,
// an EOB replaces at least one coefficient).
constexpr int kMaxBlockBits = 22 + 63 * 26;  // 1660

// natural order of zigzag position k (Figure A.6)
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Tables K.1 and K.2, natural order
constexpr uint8_t kStdQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Tables K.3 - K.6: codes per length 1..16, then the symbols in code order
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// code << 8 | length per symbol, [0] luminance / [1] chrominance (jchuff.c jpeg_make_c_derived_tbl); 0 = symbol not in the table
struct HuffCodes {
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};
constexpr HuffCodes derive_codes() {
  HuffCodes h{};
  for (int t = 0; t < 2; t++) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
      for (int i = 0; i < kDcBits[t][len - 1]; i++) h.dc[t][kDcVals[k++]] = code++ << 8 | (uint32_t)len;
      code <<= 1;
    }
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; len++) {
      for (int i = 0; i < kAcBits[t][len - 1]; i++) h.ac[t][kAcVals[t][k++]] = code++ << 8 | (uint32_t)len;
      code <<= 1;
    }
  }
  return h;
}

// zigzag position of natural index i
struct InvZigzag {
  uint8_t at[64];
};
constexpr InvZigzag derive_inv_zigzag() {
  InvZigzag z{};
  for (int k = 0; k < 64; k++) z.at[kZigzag[k]] = (uint8_t)k;
  return z;
}

// ---------------------------------------------------------------- host-only parts of the C ABI
// divisors of a quality in natural order (jcparam.c jpeg_quality_scaling / jpeg_add_quant_table with force_baseline)
inline void quant_tables(int quality, uint16_t q[2][64]) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; t++)
    for (int i = 0; i < 64; i++) {
      long v = ((long)kStdQuant[t][i] * scale + 50) / 100;
      q[t][i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

// the bytes in front of the scan; depend on the image size and the quality only.  out: kHeaderBytes bytes
inline void build_header(int H, int W_total, int quality, uint8_t* out) {
  uint16_t q[2][64];
  quant_tables(quality, q);
  uint8_t* p = out;
  auto put = [&p](std::initializer_list<int> bytes) {
    for (int b : bytes) *p++ = (uint8_t)b;
  };
  put({0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < 2; t++) {
    put({0xff, 0xdb, 0, 67, t});
    for (int k = 0; k < 64; k++) *p++ = (uint8_t)q[t][kZigzag[k]];
  }
  put({0xff, 0xc0, 0, 17, 8, H >> 8, H & 255, W_total >> 8, W_total & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
  for (int t = 0; t < 2; t++) {
    put({0xff, 0xc4, 0, 31, t});
    memcpy(p, kDcBits[t], 16);
    memcpy(p + 16, kDcVals, 12);
    p += 28;
    put({0xff, 0xc4, 0, 181, 0x10 | t});
    memcpy(p, kAcBits[t], 16);
    memcpy(p + 16, kAcVals[t], 162);
    p += 178;
  }
  put({0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
}

inline int64_t blocks_of(int H, int W_total) { return (int64_t)(H / 16) * (W_total / 16) * kBlocksPerMcu; }
// bytes the unstuffed scan of one image can take (workspace), a multiple of 16
inline int64_t scan_bytes_bound(int H, int W_total) { return ((blocks_of(H, W_total) * kMaxBlockBits + 7) / 8 + 15) / 16 * 16; }

// header + worst-case scan, every byte of it 0xFF and followed by a stuffed 0x00, + EOI; -1 = not a size the encoder takes
inline int64_t bound(int H, int W_total) {
  if (H < 16 || W_total < 16 || H % 16 || W_total % 16 || H > 65520 || W_total > 65520) return -1;
  return kHeaderBytes + 2 * ((blocks_of(H, W_total) * kMaxBlockBits + 7) / 8) + 2;
}

// argument check of mocap_encode_jpeg*: null = fine, else what is wrong.  Bit offsets inside one image are 32-bit.
inline const char* check_args(int64_t n_images, int T, int H, int W, int quality, int64_t capacity) {
  if (n_images < 0) return "n_images is negative";
  if (T < 1) return "T must be at least 1";
  if (H < 16 || W < 16 || H % 16 || W % 16) return "H and W must be multiples of 16";
  if (quality < 1 || quality > 100) return "quality must be 1..100 (libjpeg clamps; this encoder refuses)";
  if (capacity < 1) return "capacity must be positive";
  if ((int64_t)T * W > 65520 || H > 65520) return "image larger than 65520 pixels on a side";
  if (blocks_of(H, T * W) * kMaxBlockBits >= ((int64_t)1 << 31)) return "image too large: its worst-case scan exceeds 2^31 bits";
  return nullptr;
}

}  // namespace jpeg
}  // namespace mocap
