// object_filter_capi.hip -- the "object filter" section of include/mocap_core.h: set-up, reset and the filter over the
// locator's outputs (kernels: object_filter.hip).  Host runtime only; the one piece of host arithmetic is the impulse
// response of the caller's low-pass coefficients.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/mocap_core.h"
#include "ctx.hpp"

using namespace mocap;

namespace {

struct StateLayout {
  ObjFilterState* state;
  double* h;
  double* hist[2];
};

size_t lay_state(void* base, int D, int B, StateLayout& l) {
  Carver c(base);
  l.state = c.take<ObjFilterState>(1);
  l.h = c.take<double>(B);
  l.hist[0] = c.take<double>((size_t)D * 4 * B);
  l.hist[1] = c.take<double>((size_t)D * 4 * B);
  return c.off;
}

}  // namespace

extern "C" int mocap_set_object_filter(mocap_ctx* ctx, int num_objects, int n_taps, const double* b, const double* a,
                                       int buffer_size, double process_noise, double measurement_noise) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (num_objects < 0) return ctx->fail(MOCAP_E_ARG, "mocap_set_object_filter: num_objects < 0");
  if (num_objects == 0) {
    ctx->objf_D = 0;
    return MOCAP_OK;
  }
  if (n_taps < 1 || buffer_size < 2 || !b || !a || a[0] == 0.0 || !(measurement_noise > 0.0) || !(process_noise >= 0.0))
    return ctx->fail(MOCAP_E_ARG, "mocap_set_object_filter: bad argument (n_taps >= 1, buffer_size >= 2, a[0] != 0, measurement_noise > 0)");
  if (num_objects > kObjFilterMaxObjects || n_taps > kObjFilterMaxTaps || buffer_size > kObjFilterMaxBuffer)
    return ctx->fail(MOCAP_E_LIMIT, "mocap_set_object_filter: num_objects=%d n_taps=%d buffer_size=%d exceed %d / %d / %d", num_objects,
                     n_taps, buffer_size, kObjFilterMaxObjects, kObjFilterMaxTaps, kObjFilterMaxBuffer);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int D = num_objects, B = buffer_size;
  // impulse response of (b, a) from a zero state, truncated to the longest window the reference ever filters
  std::vector<double> h((size_t)B);
  for (int n = 0; n < B; n++) {
    double acc = n < n_taps ? b[n] : 0.0;
    for (int k = 1; k < n_taps && k <= n; k++) acc -= a[k] * h[(size_t)(n - k)];
    h[(size_t)n] = acc / a[0];
  }
  StateLayout l;
  const size_t total = lay_state(nullptr, D, B, l);
  ctx->objf_D = 0;
  if (ctx->objf_state.reserve(total)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%zu) failed", total);
  lay_state(ctx->objf_state.ptr, D, B, l);
  HIP_TRY(ctx, hipMemsetAsync(ctx->objf_state.ptr, 0, total, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(l.h, h.data(), sizeof(double) * B, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (h is a local)
  ctx->objf_D = D;
  ctx->objf_B = B;
  ctx->objf_q = (float)process_noise;
  ctx->objf_r = (float)measurement_noise;
  ctx->objf_calls = 0;
  return MOCAP_OK;
}

extern "C" int mocap_reset_object_filter(mocap_ctx* ctx, double now) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->objf_D) return ctx->fail(MOCAP_E_ARG, "mocap_reset_object_filter: mocap_set_object_filter has not been called");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  StateLayout l;
  lay_state(ctx->objf_state.ptr, ctx->objf_D, ctx->objf_B, l);
  HIP_TRY(ctx, launch_object_filter_reset(l.state, ctx->objf_D, now, ctx->stream));
  return ctx->mark_enqueued();
}

int filter_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int O_max, const FilterIO& io) {
  if (!ctx->objf_D) return ctx->fail(MOCAP_E_ARG, "%s: mocap_set_object_filter has not been called", who);
  if (n_frames < 0 || O_max < 1) return ctx->fail(MOCAP_E_ARG, "%s: bad size argument", who);
  if (O_max > kObjFilterMaxSlots) return ctx->fail(MOCAP_E_LIMIT, "%s: O_max=%d exceeds %d with the object filter on", who, O_max, kObjFilterMaxSlots);
  if (n_frames > ((int64_t)1 << 27)) return ctx->fail(MOCAP_E_LIMIT, "%s: more than 2^27 frames in one call", who);
  if (n_frames > 0 && (!io.t || !io.fpos || !io.fvel || !io.fheading || !io.chosen)) return ctx->fail(MOCAP_E_ARG, "%s: null filter buffer", who);
  return MOCAP_OK;
}

// (arguments checked by filter_check; context lock held by the caller)
int filter_dev_locked(mocap_ctx* ctx, int64_t n_frames, int O_max, const double* d_pos, const double* d_heading,
                      const int32_t* d_drone, const int32_t* d_n_obj, const FilterIO& io) {
  if (n_frames == 0) return MOCAP_OK;
  const int D = ctx->objf_D, B = ctx->objf_B;
  const size_t F = (size_t)n_frames;
  ObjFilterArgs a;
  auto lay_ws = [&](void* base) {
    Carver c(base);
    a.samp = c.take<double>((size_t)D * 4 * F);
    a.slot = c.take<int32_t>(F * D * 2);
    a.n_samp = c.take<int32_t>(D);
    return c.off;
  };
  if (ctx->objf_ws.reserve(lay_ws(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(object filter workspace) failed");
  lay_ws(ctx->objf_ws.ptr);
  StateLayout l;
  lay_state(ctx->objf_state.ptr, D, B, l);
  a.n_frames = n_frames;
  a.D = D;
  a.O_max = O_max;
  a.B = B;
  a.keep = (B + 1) / 2;  // LowPassFilter.py:21: buffered_data[-buffer_size//2:], Python's (-B)//2
  a.q = ctx->objf_q;
  a.r = ctx->objf_r;
  a.t = io.t;
  a.pos = d_pos;
  a.heading = d_heading;
  a.drone = d_drone;
  a.n_obj = d_n_obj;
  a.state = l.state;
  a.h = l.h;
  a.hist_in = l.hist[ctx->objf_calls & 1];
  a.hist_out = l.hist[(ctx->objf_calls & 1) ^ 1];
  a.fpos = io.fpos;
  a.fvel = io.fvel;
  a.fheading = io.fheading;
  a.chosen = io.chosen;
  ctx->objf_calls++;
  HIP_TRY(ctx, launch_object_filter(a, ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_filter_objects_dev(mocap_ctx* ctx, int64_t n_frames, const double* d_t, int O_max, const double* d_pos,
                                        const double* d_heading, const int32_t* d_drone, const int32_t* d_n_obj, float* d_fpos,
                                        float* d_fvel, double* d_fheading, int32_t* d_chosen) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const FilterIO io{d_t, d_fpos, d_fvel, d_fheading, d_chosen};
  int rc = filter_check(ctx, "mocap_filter_objects", n_frames, O_max, io);
  if (rc) return rc;
  if (n_frames == 0) return MOCAP_OK;
  if (!d_pos || !d_heading || !d_drone || !d_n_obj) return ctx->fail(MOCAP_E_ARG, "mocap_filter_objects: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = filter_dev_locked(ctx, n_frames, O_max, d_pos, d_heading, d_drone, d_n_obj, io);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_filter_objects(mocap_ctx* ctx, int64_t n_frames, const double* t, int O_max, const double* pos,
                                    const double* heading, const int32_t* drone, const int32_t* n_obj, float* fpos, float* fvel,
                                    double* fheading, int32_t* chosen) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const FilterIO io{t, fpos, fvel, fheading, chosen};
  int rc = filter_check(ctx, "mocap_filter_objects", n_frames, O_max, io);
  if (rc) return rc;
  if (n_frames == 0) return MOCAP_OK;
  if (!pos || !heading || !drone || !n_obj) return ctx->fail(MOCAP_E_ARG, "mocap_filter_objects: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, O = (size_t)O_max;
  const IoDims n{F, 0, 0, (size_t)ctx->objf_D};
  double *d_pos, *d_head;
  int32_t *d_drone, *d_nobj;
  FilterIO d{};
  auto lay = [&](void* base) {
    Carver c(base);
    d_pos = c.take<double>(F * O * 3);
    d_head = c.take<double>(F * O);
    d_drone = c.take<int32_t>(F * O);
    d_nobj = c.take<int32_t>(F);
    carve(c, d, n);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  HIP_TRY(ctx, hipMemcpyAsync(d_pos, pos, sizeof(double) * F * O * 3, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_head, heading, sizeof(double) * F * O, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_drone, drone, sizeof(int32_t) * F * O, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_nobj, n_obj, sizeof(int32_t) * F, hipMemcpyHostToDevice, ctx->stream));
  rc = copy_fields<true>(d, io, n, StreamCopy{ctx, hipMemcpyHostToDevice});
  if (!rc) rc = filter_dev_locked(ctx, n_frames, O_max, d_pos, d_head, d_drone, d_nobj, d);
  if (!rc) rc = copy_fields<false>(io, d, n, StreamCopy{ctx, hipMemcpyDeviceToHost});
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
