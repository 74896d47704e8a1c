// track_stitch_capi.hip -- the "track stitching" section of include/mocap_core.h: the rows of a gathered session linked into one
// chain per marker (kernels: track_stitch.hip).  The host form uploads, runs and downloads; the _dev form reads the rows where they lie.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>

#include "../../include/mocap_core.h"
#include "ctx.hpp"
#include "track_stitch.hpp"

using namespace mocap;

static_assert(kStMaxFit == MOCAP_ST_MAX_FIT, "limits");

namespace {

int stitch_check(mocap_ctx* ctx, int64_t n_frames, int R, const double* t, const double* traj, int fit_frames, double max_dt,
                 double gate, double gate_rate, const int32_t* ext, const int32_t* next, const int32_t* prev, const double* cost,
                 const int32_t* chain, const int32_t* row_of, const int32_t* n_chains) {
  const char* who = "mocap_stitch_tracks";
  if (n_frames < 1) return ctx->fail(MOCAP_E_ARG, "%s: n_frames must be at least 1", who);
  if (R < 1 || R > MOCAP_TS_MAX_ROWS) return ctx->fail(MOCAP_E_ARG, "%s: R must be 1 .. %d", who, MOCAP_TS_MAX_ROWS);
  if (n_frames > ((int64_t)1 << 31) / R) return ctx->fail(MOCAP_E_ARG, "%s: R * n_frames must be at most 2^31", who);
  if (fit_frames < 1 || fit_frames > MOCAP_ST_MAX_FIT) return ctx->fail(MOCAP_E_ARG, "%s: fit_frames must be 1 .. %d", who, MOCAP_ST_MAX_FIT);
  if (!(max_dt > 0.0)) return ctx->fail(MOCAP_E_ARG, "%s: max_dt must be > 0 (+inf = any)", who);
  if (!(gate > 0.0 && std::isfinite(gate))) return ctx->fail(MOCAP_E_ARG, "%s: gate must be finite and > 0", who);
  if (!(gate_rate >= 0.0 && std::isfinite(gate_rate))) return ctx->fail(MOCAP_E_ARG, "%s: gate_rate must be finite and >= 0", who);
  if (!t || !traj || !ext || !next || !prev || !cost || !chain || !row_of || !n_chains) return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  return MOCAP_OK;
}

// (arguments checked; context lock held by the caller; every pointer device-accessible)
int stitch_dev_locked(mocap_ctx* ctx, StitchTracksArgs a) {
  auto lay = [&](void* base) {
    Carver c(base);
    a.tile_max = c.take<double>((size_t)ts_tiles(a.n_frames));
    a.model = c.take<double>((size_t)a.R * 2 * kStModel);
    a.table = c.take<double>((size_t)a.R * a.R);
    a.good = c.take<uint8_t>((size_t)a.n_frames);
    return c.off;
  };
  if (ctx->calib_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(stitching workspace) failed");
  lay(ctx->calib_ws.ptr);
  HIP_TRY(ctx, launch_stitch_tracks(a, ctx->stream));
  return MOCAP_OK;
}

}  // namespace

extern "C" int mocap_stitch_tracks_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_t, const double* d_traj, int fit_frames,
                                       double max_dt, double gate, double gate_rate, int32_t* d_ext, int32_t* d_next, int32_t* d_prev,
                                       double* d_cost, int32_t* d_chain, int32_t* d_row_of, int32_t* d_n_chains) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = stitch_check(ctx, n_frames, R, d_t, d_traj, fit_frames, max_dt, gate, gate_rate, d_ext, d_next, d_prev, d_cost, d_chain,
                            d_row_of, d_n_chains))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const StitchTracksArgs a{n_frames, R, fit_frames, max_dt, gate, gate_rate, d_t, d_traj, nullptr, nullptr, nullptr, nullptr,
                           d_ext, d_next, d_prev, d_cost, d_chain, d_row_of, d_n_chains};
  const int rc = stitch_dev_locked(ctx, a);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_stitch_tracks(mocap_ctx* ctx, int64_t n_frames, int R, const double* t, const double* traj, int fit_frames,
                                   double max_dt, double gate, double gate_rate, int32_t* ext, int32_t* next, int32_t* prev,
                                   double* cost, int32_t* chain, int32_t* row_of, int32_t* n_chains) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = stitch_check(ctx, n_frames, R, t, traj, fit_frames, max_dt, gate, gate_rate, ext, next, prev, cost, chain, row_of, n_chains))
    return rc;
  bool any_finite = false;
  for (int64_t f = 0; f < n_frames && !any_finite; f++) any_finite = std::isfinite(t[f]);
  if (!any_finite) return ctx->fail(MOCAP_E_ARG, "mocap_stitch_tracks: t has no finite entry");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, Rz = (size_t)R;
  StitchTracksArgs a{n_frames, R, fit_frames, max_dt, gate, gate_rate};
  double *d_t, *d_traj;
  auto lay = [&](void* base) {
    Carver c(base);
    d_t = c.take<double>(F);
    d_traj = c.take<double>(Rz * F * 3);
    a.cost = c.take<double>(Rz);
    a.ext = c.take<int32_t>(Rz * 3);
    a.next = c.take<int32_t>(Rz);
    a.prev = c.take<int32_t>(Rz);
    a.chain = c.take<int32_t>(Rz);
    a.row_of = c.take<int32_t>(Rz);
    a.n_chains = c.take<int32_t>(1);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  a.t = d_t;
  a.traj = d_traj;
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if (up(d_t, t, sizeof(double) * F) || up(d_traj, traj, sizeof(double) * Rz * F * 3)) return MOCAP_E_HIP;
  if (int rc = stitch_dev_locked(ctx, a)) return rc;
  if (down(ext, a.ext, sizeof(int32_t) * Rz * 3) || down(next, a.next, sizeof(int32_t) * Rz) || down(prev, a.prev, sizeof(int32_t) * Rz) ||
      down(cost, a.cost, sizeof(double) * Rz) || down(chain, a.chain, sizeof(int32_t) * Rz) ||
      down(row_of, a.row_of, sizeof(int32_t) * Rz) || down(n_chains, a.n_chains, sizeof(int32_t)))
    return MOCAP_E_HIP;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
