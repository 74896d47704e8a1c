// overlay_capi.hip -- C ABI of the preview overlays (include/mocap_core.h, "preview overlays"): the option, the argument
// checks, and the kernels of overlay_kernels.hip on the context's stream.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "../../include/mocap_core.h"
#include "ctx.hpp"

using namespace mocap;

static_assert(MOCAP_OVERLAY_CONTOURS == (int)kOverlayContours && MOCAP_OVERLAY_CENTRES == (int)kOverlayCentres &&
                  MOCAP_OVERLAY_EPILINES == (int)kOverlayEpilines,
              "kernels.hpp mirrors the overlay bits of mocap_core.h");

extern "C" int mocap_set_preview_overlay(mocap_ctx* ctx, uint32_t flags) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (flags & ~(uint32_t)(MOCAP_OVERLAY_CONTOURS | MOCAP_OVERLAY_CENTRES | MOCAP_OVERLAY_EPILINES))
    return ctx->fail(MOCAP_E_ARG, "mocap_set_preview_overlay: unknown bit in %#x", flags);
  ctx->preview_overlay = flags;
  return MOCAP_OK;
}

int overlay_blobs_locked(mocap_ctx* ctx, uint32_t flags, int64_t n_images, int S, int M_max, const float* d_blobs,
                         const int32_t* d_counts, const int32_t* d_status, uint8_t* d_bgr) {
  OverlayArgs a;
  a.n_images = n_images;
  a.S = S;
  a.M_max = M_max;
  a.flags = flags & (kOverlayContours | kOverlayCentres);
  a.mask = (const unsigned long long*)ctx->img_mask.ptr;
  a.blobs = d_blobs;
  a.counts = d_counts;
  a.status = d_status;
  a.bgr = d_bgr;
  HIP_TRY(ctx, launch_overlay_blobs(a, ctx->stream));
  return MOCAP_OK;
}

int epilines_dev_locked(mocap_ctx* ctx, const char* who, int64_t n_frames, int S, uint8_t* d_bgr, int M_max, const float* d_blobs,
                        const int32_t* d_counts, int K_max, const int16_t* d_corr, const int32_t* d_n_pts, const int32_t* d_status) {
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
  // S <= 65535: a coefficient (24 bits) times a column or row number stays exact in double
  if (n_frames < 0 || S < 1 || S > 65535 || M_max < 1 || K_max < 1) return ctx->fail(MOCAP_E_ARG, "%s: bad size argument", who);
  if (n_frames == 0) return MOCAP_OK;
  if (!d_bgr || !d_blobs || !d_counts || !d_corr || !d_n_pts || !d_status) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  EpilineArgs a;
  a.n_frames = n_frames;
  a.C = ctx->C;
  a.S = S;
  a.M_max = M_max;
  a.K_max = K_max;
  a.f32_rounding = ctx->cv.f32_rounding;
  a.F = ctx->cv.F;
  a.blobs = d_blobs;
  a.counts = d_counts;
  a.corr = d_corr;
  a.n_pts = d_n_pts;
  a.status = d_status;
  a.bgr = d_bgr;
  HIP_TRY(ctx, launch_overlay_epilines(a, ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_draw_epilines_dev(mocap_ctx* ctx, int64_t n_frames, int S, uint8_t* d_bgr, int M_max, const float* d_blobs,
                                       const int32_t* d_counts, int K_max, const int16_t* d_corr, const int32_t* d_n_pts,
                                       const int32_t* d_status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = epilines_dev_locked(ctx, "mocap_draw_epilines_dev", n_frames, S, d_bgr, M_max, d_blobs, d_counts, K_max, d_corr,
                                     d_n_pts, d_status);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_draw_epilines(mocap_ctx* ctx, int64_t n_frames, int S, uint8_t* bgr, int M_max, const float* blobs,
                                   const int32_t* counts, int K_max, const int16_t* corr, const int32_t* n_pts,
                                   const int32_t* status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
  if (n_frames < 0 || S < 1 || S > 65535 || M_max < 1 || K_max < 1) return ctx->fail(MOCAP_E_ARG, "mocap_draw_epilines: bad size argument");
  if (n_frames == 0) return MOCAP_OK;
  if (!bgr || !blobs || !counts || !corr || !n_pts || !status) return ctx->fail(MOCAP_E_ARG, "mocap_draw_epilines: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, C = (size_t)ctx->C;
  const size_t b_bgr = F * C * S * S * 3, n_blobs = F * C * M_max * 2, n_corr = F * K_max * C;
  uint8_t* d_bgr;
  float* d_blobs;
  int16_t* d_corr;
  int32_t *d_counts, *d_n_pts, *d_status;
  auto lay = [&](void* base) {
    Carver c(base);
    d_bgr = c.take<uint8_t>(b_bgr);
    d_blobs = c.take<float>(n_blobs);
    d_counts = c.take<int32_t>(F * C);
    d_corr = c.take<int16_t>(n_corr);
    d_n_pts = c.take<int32_t>(F);
    d_status = c.take<int32_t>(F);
    return c.off;
  };
  const size_t total = lay(nullptr);
  if (ctx->overlay_stage.reserve(total)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%zu) failed", total);
  lay(ctx->overlay_stage.ptr);
  HIP_TRY(ctx, hipMemcpyAsync(d_bgr, bgr, b_bgr, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_blobs, blobs, sizeof(float) * n_blobs, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_counts, counts, sizeof(int32_t) * F * C, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_corr, corr, sizeof(int16_t) * n_corr, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_n_pts, n_pts, sizeof(int32_t) * F, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_status, status, sizeof(int32_t) * F, hipMemcpyHostToDevice, ctx->stream));
  const int rc = epilines_dev_locked(ctx, "mocap_draw_epilines", n_frames, S, d_bgr, M_max, d_blobs, d_counts, K_max, d_corr, d_n_pts, d_status);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(bgr, d_bgr, b_bgr, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
