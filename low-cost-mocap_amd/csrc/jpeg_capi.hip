// jpeg_capi.hip -- C ABI of the preview-stream JPEG encoder (include/mocap_core.h, "preview stream"): argument checks,
// the per-(shape, quality) header and divisors, the workspace, and the kernels of jpeg_kernels.hip on the context's stream.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "../../include/mocap_core.h"
#include "ctx.hpp"
#include "jpeg_tables.hpp"

using namespace mocap;

extern "C" int64_t mocap_jpeg_bound(int H, int W_total) { return jpeg::bound(H, W_total); }

int jpeg_dev_locked(mocap_ctx* ctx, const char* who, int64_t n_images, int T, int H, int W, const uint8_t* d_bgr, int quality,
                    uint8_t* d_jpeg, int64_t capacity, int64_t* d_sizes, int32_t* d_status, int64_t out_stride) {
  const char* bad = jpeg::check_args(n_images, T, H, W, quality, capacity);
  if (bad) return ctx->fail(MOCAP_E_ARG, "%s: %s", who, bad);
  if (n_images == 0) return MOCAP_OK;
  if (!d_bgr || !d_jpeg || !d_sizes || !d_status) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  if ((uintptr_t)d_bgr % 4) return ctx->fail(MOCAP_E_ARG, "%s: the frames must be 4-byte aligned", who);
  const int Wt = T * W;
  if (ctx->jpeg_key[0] != H || ctx->jpeg_key[1] != Wt || ctx->jpeg_key[2] != quality) {
    memset(&ctx->jpeg_params, 0, sizeof ctx->jpeg_params);
    jpeg::build_header(H, Wt, quality, ctx->jpeg_params.header);
    jpeg::quant_tables(quality, ctx->jpeg_params.quant);
    ctx->jpeg_key[0] = H;
    ctx->jpeg_key[1] = Wt;
    ctx->jpeg_key[2] = quality;
  }
  // the workspace holds a chunk of images (at most ~256 MB, one image at least); chunks follow each other on the stream
  const size_t n_blk = (size_t)jpeg::blocks_of(H, Wt), scan_words = (size_t)jpeg::scan_bytes_bound(H, Wt) / 4;
  const size_t per_image = n_blk * (64 * sizeof(int16_t) + 8) + scan_words * 4 + 4;
  int64_t chunk = (int64_t)(((size_t)256 << 20) / per_image);
  chunk = chunk < 1 ? 1 : (chunk > n_images ? n_images : chunk);
  JpegArgs a;
  memset(&a, 0, sizeof a);
  auto lay = [&](void* base) {
    Carver c(base);
    a.coef = c.take<int16_t>(chunk * n_blk * 64);
    a.acbits = c.take<int32_t>(chunk * n_blk);
    a.bitoff = c.take<uint32_t>(chunk * n_blk);
    a.total_bits = c.take<uint32_t>(chunk);
    a.scan = c.take<uint32_t>(chunk * scan_words);
    return c.off;
  };
  const size_t total = lay(nullptr);
  if (ctx->jpeg_ws.reserve(total)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%zu) failed (JPEG workspace)", total);
  lay(ctx->jpeg_ws.ptr);
  a.T = T;
  a.H = H;
  a.W = W;
  a.mcu_x = Wt / 16;
  a.mcu_y = H / 16;
  a.scan_words = (int64_t)scan_words;
  a.capacity = capacity;
  a.out_stride = out_stride > capacity ? out_stride : capacity;
  for (int64_t f0 = 0; f0 < n_images; f0 += chunk) {
    a.n_images = n_images - f0 < chunk ? n_images - f0 : chunk;
    a.bgr = d_bgr + (size_t)f0 * T * H * W * 3;
    a.out = d_jpeg + (size_t)f0 * a.out_stride;
    a.sizes = d_sizes + f0;
    a.status = d_status + f0;
    HIP_TRY(ctx, launch_jpeg_encode(a, ctx->jpeg_params, ctx->stream));
  }
  return MOCAP_OK;
}

extern "C" int mocap_encode_jpeg_dev(mocap_ctx* ctx, int64_t n_images, int T, int H, int W, const uint8_t* d_bgr, int quality,
                                     uint8_t* d_jpeg, int64_t capacity, int64_t* d_sizes, int32_t* d_status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = jpeg_dev_locked(ctx, "mocap_encode_jpeg_dev", n_images, T, H, W, d_bgr, quality, d_jpeg, capacity, d_sizes, d_status);
  return rc ? rc : ctx->mark_enqueued();
}

namespace {

// sizes and status to the host, then of every stream the bytes that exist: min(size, capacity)
int fetch_streams(mocap_ctx* ctx, int64_t n, const uint8_t* d_out, int64_t capacity, const int64_t* d_sizes, const int32_t* d_status,
                  uint8_t* jpeg, int64_t* sizes, int32_t* status) {
  HIP_TRY(ctx, hipMemcpyAsync(sizes, d_sizes, sizeof(int64_t) * n, hipMemcpyDeviceToHost, ctx->stream));
  if (status) HIP_TRY(ctx, hipMemcpyAsync(status, d_status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int64_t f = 0; f < n; f++) {
    const int64_t k = sizes[f] < capacity ? sizes[f] : capacity;
    HIP_TRY(ctx, hipMemcpyAsync(jpeg + (size_t)f * capacity, d_out + (size_t)f * capacity, (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

}  // namespace

extern "C" int mocap_encode_jpeg(mocap_ctx* ctx, int64_t n_images, int T, int H, int W, const uint8_t* bgr, int quality,
                                 uint8_t* jpeg, int64_t capacity, int64_t* sizes, int32_t* status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const char* bad = jpeg::check_args(n_images, T, H, W, quality, capacity);
  if (bad) return ctx->fail(MOCAP_E_ARG, "mocap_encode_jpeg: %s", bad);
  if (n_images == 0) return MOCAP_OK;
  if (!bgr || !jpeg || !sizes || !status) return ctx->fail(MOCAP_E_ARG, "mocap_encode_jpeg: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)n_images, b_in = n * T * H * W * 3;
  uint8_t *d_in, *d_out;
  int64_t* d_sizes;
  int32_t* d_status;
  auto lay = [&](void* base) {
    Carver c(base);
    d_in = c.take<uint8_t>(b_in);
    d_out = c.take<uint8_t>(n * (size_t)capacity);
    d_sizes = c.take<int64_t>(n);
    d_status = c.take<int32_t>(n);
    return c.off;
  };
  const size_t total = lay(nullptr);
  if (ctx->jpeg_stage.reserve(total)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%zu) failed", total);
  lay(ctx->jpeg_stage.ptr);
  HIP_TRY(ctx, hipMemcpyAsync(d_in, bgr, b_in, hipMemcpyHostToDevice, ctx->stream));
  const int rc = jpeg_dev_locked(ctx, "mocap_encode_jpeg", n_images, T, H, W, d_in, quality, d_out, capacity, d_sizes, d_status);
  if (rc) return rc;
  return fetch_streams(ctx, n_images, d_out, capacity, d_sizes, d_status, jpeg, sizes, status);
}

extern "C" int mocap_find_blobs_jpeg(mocap_ctx* ctx, int64_t n_frames, const uint8_t* images, int M_max, float* blobs,
                                     int32_t* counts, int32_t* status, int32_t* n_contours, int quality, uint8_t* jpeg,
                                     int64_t capacity, int64_t* jpeg_size) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->img_C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_image_params has not been called");
  const int C = ctx->img_C, S = ctx->img_S;
  const char* bad = jpeg::check_args(n_frames, C, S, S, quality, capacity);
  if (bad) return ctx->fail(MOCAP_E_ARG, "mocap_find_blobs_jpeg: %s", bad);
  if (M_max < 1 || (n_frames > 0 && (!images || !blobs || !counts || !status || !jpeg || !jpeg_size)))
    return ctx->fail(MOCAP_E_ARG, "mocap_find_blobs_jpeg: bad argument");
  if (n_frames == 0) return MOCAP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, n_img = F * C;
  const size_t b_raw = n_img * ctx->img_rows * ctx->img_cols * 3, b_blobs = n_img * M_max * 2 * sizeof(float), b_i32 = n_img * sizeof(int32_t);
  uint8_t *d_raw, *d_proc, *d_out;
  float* d_blobs;
  int32_t *d_counts, *d_status, *d_ncont, *d_jstat;
  int64_t* d_sizes;
  auto lay = [&](void* base) {
    Carver c(base);
    d_raw = c.take<uint8_t>(b_raw);
    d_blobs = c.take<float>(n_img * M_max * 2);
    d_counts = c.take<int32_t>(n_img);
    d_status = c.take<int32_t>(n_img);
    d_ncont = c.take<int32_t>(n_img);
    d_proc = c.take<uint8_t>(n_img * S * S * 3);  // the processed frames never leave the device
    d_out = c.take<uint8_t>(F * (size_t)capacity);
    d_sizes = c.take<int64_t>(F);
    d_jstat = c.take<int32_t>(F);
    return c.off;
  };
  const size_t total = lay(nullptr);
  if (ctx->jpeg_stage.reserve(total)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%zu) failed", total);
  lay(ctx->jpeg_stage.ptr);
  HIP_TRY(ctx, hipMemcpyAsync(d_raw, images, b_raw, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_blobs, 0, b_blobs, ctx->stream));
  int rc = mocap_blob_stage_locked(ctx, n_frames, d_raw, M_max, d_blobs, d_counts, d_status, d_proc, d_ncont);
  if (rc) return rc;
  rc = jpeg_dev_locked(ctx, "mocap_find_blobs_jpeg", n_frames, C, S, S, d_proc, quality, d_out, capacity, d_sizes, d_jstat);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(blobs, d_blobs, b_blobs, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts, b_i32, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(status, d_status, b_i32, hipMemcpyDeviceToHost, ctx->stream));
  if (n_contours) HIP_TRY(ctx, hipMemcpyAsync(n_contours, d_ncont, b_i32, hipMemcpyDeviceToHost, ctx->stream));
  return fetch_streams(ctx, n_frames, d_out, capacity, d_sizes, d_jstat, jpeg, jpeg_size, nullptr);
}
