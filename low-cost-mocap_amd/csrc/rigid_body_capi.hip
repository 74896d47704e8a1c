// rigid_body_capi.hip -- the "rigid bodies" section of include/mocap_core.h: registration (checks, pair distances and the
// posability mask of every marker subset, tabulated once on the host) and the locator over a batch's points (kernel:
// rigid_body.hip).  Host runtime only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/mocap_core.h"
#include "ctx.hpp"

using namespace mocap;

static_assert(kRbMaxBodies == MOCAP_RB_MAX_BODIES && kRbMaxMarkers == MOCAP_RB_MAX_MARKERS && kRbMaxPoints == MOCAP_RB_MAX_POINTS,
              "kernels.hpp mirrors include/mocap_core.h");
static_assert(RB_ST_RMS_ == MOCAP_RB_ST_RMS && RB_ST_WORK_CAP_ == MOCAP_RB_ST_WORK_CAP && kRbDefaultWorkCap == MOCAP_RB_DEFAULT_WORK_CAP,
              "kernels.hpp mirrors include/mocap_core.h");
static_assert(BodiesIO::kAssign == MOCAP_RB_MAX_MARKERS, "io_fields.hpp mirrors include/mocap_core.h");

namespace {

// D of the contract: sqrt(dx dx + dy dy + dz dz), summed in x, y, z order (unfused: -ffp-contract=off)
double rb_dist(const double* p, const double* q) {
  const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return std::sqrt((dx * dx + dy * dy) + dz * dz);
}

// |(q_j - q_i) x (q_k - q_i)| >= 0.1 |q_j - q_i| |q_k - q_i|
bool rb_triple_spans(const double* qi, const double* qj, const double* qk) {
  const double u[3] = {qj[0] - qi[0], qj[1] - qi[1], qj[2] - qi[2]}, v[3] = {qk[0] - qi[0], qk[1] - qi[1], qk[2] - qi[2]};
  const double c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const double nc = std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  const double nu = std::sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]), nv = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  return nc >= (0.1 * nu) * nv;
}

// bit s of the mask: the marker subset s holds a spanning triple (so it has >= 3 markers)
void rb_posable_mask(int n, const double (*q)[3], unsigned long long mask[4]) {
  mask[0] = mask[1] = mask[2] = mask[3] = 0;
  unsigned char triple[kRbMaxMarkers][kRbMaxMarkers][kRbMaxMarkers];
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++)
      for (int k = j + 1; k < n; k++) triple[i][j][k] = rb_triple_spans(q[i], q[j], q[k]) ? 1 : 0;
  for (unsigned s = 0; s < (1u << n); s++) {
    bool ok = false;
    for (int i = 0; i < n && !ok; i++)
      for (int j = i + 1; j < n && !ok; j++)
        for (int k = j + 1; k < n && !ok; k++) ok = (s >> i & 1) && (s >> j & 1) && (s >> k & 1) && triple[i][j][k];
    if (ok) mask[s >> 6] |= 1ull << (s & 63);
  }
}

}  // namespace

extern "C" int mocap_set_rigid_bodies(mocap_ctx* ctx, int B, const int32_t* n_markers, const double* markers, double tol,
                                      double max_rms, int64_t work_cap) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (B < 0 || B > kRbMaxBodies) return ctx->fail(MOCAP_E_ARG, "mocap_set_rigid_bodies: B=%d outside 0 .. %d", B, kRbMaxBodies);
  if (B == 0) {
    ctx->rb_B = 0;
    return tracked_clear_locked(ctx);  // (the body tracker's slots mean other bodies now; nothing with the tracker off)
  }
  if (!n_markers || !markers) return ctx->fail(MOCAP_E_ARG, "mocap_set_rigid_bodies: null buffer");
  if (!(tol > 0.0) || !(max_rms > 0.0) || !std::isfinite(tol) || !std::isfinite(max_rms) || work_cap < 0)
    return ctx->fail(MOCAP_E_ARG, "mocap_set_rigid_bodies: tol and max_rms must be > 0 and finite, work_cap >= 0");
  std::vector<RigidBodyModel> models((size_t)B);
  for (int b = 0; b < B; b++) {
    RigidBodyModel& m = models[(size_t)b];
    memset(&m, 0, sizeof m);
    const int n = n_markers[b];
    if (n < 3 || n > kRbMaxMarkers) return ctx->fail(MOCAP_E_ARG, "mocap_set_rigid_bodies: body %d has %d markers (3 .. %d)", b, n, kRbMaxMarkers);
    m.n = n;
    for (int i = 0; i < n; i++)
      for (int k = 0; k < 3; k++) {
        const double v = markers[((size_t)b * kRbMaxMarkers + i) * 3 + k];
        if (!std::isfinite(v)) return ctx->fail(MOCAP_E_ARG, "mocap_set_rigid_bodies: body %d, marker %d: non-finite coordinate", b, i);
        m.q[i][k] = v;
      }
    for (int i = 0; i < n; i++)
      for (int j = i + 1; j < n; j++) {
        const double d = rb_dist(m.q[i], m.q[j]);
        if (d < 2.0 * tol)
          return ctx->fail(MOCAP_E_ARG, "mocap_set_rigid_bodies: body %d: markers %d and %d are %g apart, less than 2 tol = %g", b, i, j, d, 2.0 * tol);
        m.d[rb_pair(i, j)] = d;
      }
    rb_posable_mask(n, m.q, m.posable);
    const unsigned full = (1u << n) - 1;
    if (!((m.posable[full >> 6] >> (full & 63)) & 1ull))
      return ctx->fail(MOCAP_E_ARG, "mocap_set_rigid_bodies: body %d is not posable (its markers are collinear)", b);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // (the table is replaced behind everything already queued on the stream, and in place before the call returns)
  if (ctx->rb_models.cap < sizeof(RigidBodyModel) * kRbMaxBodies) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a grown buffer is a new one: nothing queued may still read the old
    if (ctx->rb_models.reserve(sizeof(RigidBodyModel) * kRbMaxBodies)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(rigid body table) failed");
  }
  HIP_TRY(ctx, hipMemcpyAsync(ctx->rb_models.ptr, models.data(), sizeof(RigidBodyModel) * B, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (models is a local)
  ctx->rb_B = B;
  ctx->rb_tol = tol;
  ctx->rb_max_rms = max_rms;
  ctx->rb_work_cap = work_cap > 0 ? (long long)work_cap : kRbDefaultWorkCap;
  return tracked_clear_locked(ctx);  // (the body tracker's slots mean other bodies now; nothing with the tracker off)
}

int bodies_check(mocap_ctx* ctx, const char* who, int64_t n_frames, int K_max, const BodiesIO& io) {
  if (n_frames < 0 || K_max < 1 || io.B_max < 0) return ctx->fail(MOCAP_E_ARG, "%s: bad size argument", who);
  if (io.B_max < ctx->rb_B) return ctx->fail(MOCAP_E_ARG, "%s: B_max=%d is less than the %d registered bodies", who, io.B_max, ctx->rb_B);
  if (ctx->rb_B > 0 && K_max > kRbMaxPoints)
    return ctx->fail(MOCAP_E_ARG, "%s: K_max=%d exceeds the %d points per frame the rigid-body search takes", who, K_max, kRbMaxPoints);
  if (n_frames > 0 && io.B_max > 0 && (!io.found || !io.n_used || !io.assign || !io.R || !io.t || !io.rms || !io.score || !io.status))
    return ctx->fail(MOCAP_E_ARG, "%s: null body buffer", who);
  return MOCAP_OK;
}

// (arguments checked by bodies_check; context lock held by the caller)
int bodies_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts, const BodiesIO& io) {
  if (n_frames == 0 || io.B_max == 0) return MOCAP_OK;
  RigidBodyArgs a;
  a.n_frames = n_frames;
  a.K_max = K_max;
  a.B = ctx->rb_B;
  a.B_max = io.B_max;
  a.tol = ctx->rb_tol;
  a.max_rms = ctx->rb_max_rms;
  a.work_cap = ctx->rb_work_cap;
  a.models = (const RigidBodyModel*)ctx->rb_models.ptr;
  a.xyz = d_xyz;
  a.n_pts = d_n_pts;
  a.found = io.found;
  a.n_used = io.n_used;
  a.assign = io.assign;
  a.R = io.R;
  a.t = io.t;
  a.rms = io.rms;
  a.score = io.score;
  a.status = io.status;
  HIP_TRY(ctx, launch_rigid_bodies(a, ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_locate_rigid_bodies_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const int32_t* d_n_pts,
                                             int B_max, int32_t* d_found, int32_t* d_n_used, int8_t* d_assign, double* d_R,
                                             double* d_t, double* d_rms, double* d_score, int32_t* d_status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const BodiesIO io{B_max, d_found, d_n_used, d_assign, d_R, d_t, d_rms, d_score, d_status};
  int rc = bodies_check(ctx, "mocap_locate_rigid_bodies_dev", n_frames, K_max, io);
  if (rc) return rc;
  if (n_frames == 0 || B_max == 0) return MOCAP_OK;
  if (!d_xyz || !d_n_pts) return ctx->fail(MOCAP_E_ARG, "mocap_locate_rigid_bodies_dev: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = bodies_dev_locked(ctx, n_frames, K_max, d_xyz, d_n_pts, io);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_locate_rigid_bodies(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const int32_t* n_pts, int B_max,
                                         int32_t* found, int32_t* n_used, int8_t* assign, double* R, double* t, double* rms,
                                         double* score, int32_t* status) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const BodiesIO io{B_max, found, n_used, assign, R, t, rms, score, status};
  int rc = bodies_check(ctx, "mocap_locate_rigid_bodies", n_frames, K_max, io);
  if (rc) return rc;
  if (n_frames == 0 || B_max == 0) return MOCAP_OK;
  if (!xyz || !n_pts) return ctx->fail(MOCAP_E_ARG, "mocap_locate_rigid_bodies: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const IoDims n{(size_t)n_frames, (size_t)K_max, (size_t)B_max};
  double* d_xyz;
  int32_t* d_n;
  BodiesIO d{B_max};
  auto lay = [&](void* base) {
    Carver c(base);
    d_xyz = c.take<double>(n.F * n.K * 3);
    d_n = c.take<int32_t>(n.F);
    carve(c, d, n);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  HIP_TRY(ctx, hipMemcpyAsync(d_xyz, xyz, sizeof(double) * n.F * n.K * 3, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_n, n_pts, sizeof(int32_t) * n.F, hipMemcpyHostToDevice, ctx->stream));
  rc = bodies_dev_locked(ctx, n_frames, K_max, d_xyz, d_n, d);
  if (!rc) rc = copy_fields<false>(io, d, n, StreamCopy{ctx, hipMemcpyDeviceToHost});
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
