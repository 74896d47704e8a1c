// rigid_groups_capi.hip -- the "rigid groups" section of include/mocap_core.h: the rows of a gathered session that keep their mutual
// distances (kernels: rigid_groups.hip).  The host form uploads, runs and downloads; the _dev form reads the rows where they lie.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>

#include "../../include/mocap_core.h"
#include "ctx.hpp"
#include "rigid_groups.hpp"

using namespace mocap;

static_assert(kRgMaxRows == MOCAP_RG_MAX_ROWS && kRgMaxFrames == MOCAP_RG_MAX_FRAMES, "limits");

namespace {

constexpr size_t kSlabBudget = (size_t)192 << 20;  // bytes of the two slabs of one round of launches
constexpr size_t kRoundPairs = 256;                // block pairs of one round at most: R = 256 (528 of them) always takes three rounds

int groups_check(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int min_common, double tol, double max_dist,
                 double min_travel, const int32_t* cnt, const double* dist, const double* spread, const double* travel,
                 const int32_t* group_of, const int32_t* gsize, const int32_t* ghead, const int32_t* gconf, const double* gspread,
                 const int32_t* n_groups) {
  const char* who = "mocap_rigid_groups";
  if (n_frames < 1 || n_frames > MOCAP_RG_MAX_FRAMES) return ctx->fail(MOCAP_E_ARG, "%s: n_frames must be 1 .. %d", who, MOCAP_RG_MAX_FRAMES);
  if (R < 1 || R > MOCAP_RG_MAX_ROWS) return ctx->fail(MOCAP_E_ARG, "%s: R must be 1 .. %d", who, MOCAP_RG_MAX_ROWS);
  if (min_common < 2) return ctx->fail(MOCAP_E_ARG, "%s: min_common must be at least 2", who);
  if (!(tol > 0.0 && std::isfinite(tol))) return ctx->fail(MOCAP_E_ARG, "%s: tol must be finite and > 0", who);
  if (!(max_dist > 0.0)) return ctx->fail(MOCAP_E_ARG, "%s: max_dist must be > 0 (+inf = any)", who);
  if (!(min_travel >= 0.0 && std::isfinite(min_travel))) return ctx->fail(MOCAP_E_ARG, "%s: min_travel must be finite and >= 0", who);
  if (!traj || !cnt || !dist || !spread || !travel || !group_of || !gsize || !ghead || !gconf || !gspread || !n_groups)
    return ctx->fail(MOCAP_E_ARG, "%s: null buffer", who);
  return MOCAP_OK;
}

// (arguments checked; context lock held by the caller; every pointer device-accessible)
int groups_dev_locked(mocap_ctx* ctx, RigidGroupsArgs a) {
  const size_t P = (size_t)rg_tiles(a.n_frames), per_pair = (size_t)kRgSlots * P * (sizeof(double) + sizeof(int32_t));
  const size_t fit = kSlabBudget / per_pair, pairs = (size_t)rg_block_pairs(a.R);
  const size_t most = pairs < kRoundPairs ? pairs : kRoundPairs;
  a.round_pairs = (int)(fit < 1 ? 1 : fit > most ? most : fit);
  auto lay = [&](void* base) {
    Carver c(base);
    a.slab = c.take<double>((size_t)a.round_pairs * kRgSlots * P);
    a.bounds = c.take<unsigned long long>((size_t)a.R * 6);
    a.cslab = c.take<int32_t>((size_t)a.round_pairs * kRgSlots * P);
    return c.off;
  };
  if (ctx->calib_ws.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(rigid groups workspace) failed");
  lay(ctx->calib_ws.ptr);
  HIP_TRY(ctx, launch_rigid_groups(a, ctx->stream));
  return MOCAP_OK;
}

}  // namespace

extern "C" int mocap_rigid_groups_dev(mocap_ctx* ctx, int64_t n_frames, int R, const double* d_traj, int min_common, double tol,
                                      double max_dist, double min_travel, int32_t* d_cnt, double* d_dist, double* d_spread,
                                      double* d_travel, int32_t* d_group_of, int32_t* d_gsize, int32_t* d_ghead, int32_t* d_gconf,
                                      double* d_gspread, int32_t* d_n_groups) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = groups_check(ctx, n_frames, R, d_traj, min_common, tol, max_dist, min_travel, d_cnt, d_dist, d_spread, d_travel,
                            d_group_of, d_gsize, d_ghead, d_gconf, d_gspread, d_n_groups))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  RigidGroupsArgs a{n_frames, R, min_common, tol, max_dist, min_travel, d_traj};
  a.cnt = d_cnt;
  a.dist = d_dist;
  a.spread = d_spread;
  a.travel = d_travel;
  a.group_of = d_group_of;
  a.gsize = d_gsize;
  a.ghead = d_ghead;
  a.gconf = d_gconf;
  a.gspread = d_gspread;
  a.n_groups = d_n_groups;
  const int rc = groups_dev_locked(ctx, a);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_rigid_groups(mocap_ctx* ctx, int64_t n_frames, int R, const double* traj, int min_common, double tol,
                                  double max_dist, double min_travel, int32_t* cnt, double* dist, double* spread, double* travel,
                                  int32_t* group_of, int32_t* gsize, int32_t* ghead, int32_t* gconf, double* gspread,
                                  int32_t* n_groups) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = groups_check(ctx, n_frames, R, traj, min_common, tol, max_dist, min_travel, cnt, dist, spread, travel, group_of, gsize,
                            ghead, gconf, gspread, n_groups))
    return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames, Rz = (size_t)R;
  RigidGroupsArgs a{n_frames, R, min_common, tol, max_dist, min_travel};
  double* d_traj;
  auto lay = [&](void* base) {
    Carver c(base);
    d_traj = c.take<double>(Rz * F * 3);
    a.dist = c.take<double>(Rz * Rz);
    a.spread = c.take<double>(Rz * Rz);
    a.travel = c.take<double>(Rz);
    a.gspread = c.take<double>(Rz);
    a.cnt = c.take<int32_t>(Rz * Rz);
    a.group_of = c.take<int32_t>(Rz);
    a.gsize = c.take<int32_t>(Rz);
    a.ghead = c.take<int32_t>(Rz);
    a.gconf = c.take<int32_t>(Rz);
    a.n_groups = c.take<int32_t>(1);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  a.traj = d_traj;
  const StreamCopy up{ctx, hipMemcpyHostToDevice}, down{ctx, hipMemcpyDeviceToHost};
  if (up(d_traj, traj, sizeof(double) * Rz * F * 3)) return MOCAP_E_HIP;
  if (int rc = groups_dev_locked(ctx, a)) return rc;
  if (down(cnt, a.cnt, sizeof(int32_t) * Rz * Rz) || down(dist, a.dist, sizeof(double) * Rz * Rz) ||
      down(spread, a.spread, sizeof(double) * Rz * Rz) || down(travel, a.travel, sizeof(double) * Rz) ||
      down(group_of, a.group_of, sizeof(int32_t) * Rz) || down(gsize, a.gsize, sizeof(int32_t) * Rz) ||
      down(ghead, a.ghead, sizeof(int32_t) * Rz) || down(gconf, a.gconf, sizeof(int32_t) * Rz) ||
      down(gspread, a.gspread, sizeof(double) * Rz) || down(n_groups, a.n_groups, sizeof(int32_t)))
    return MOCAP_E_HIP;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
