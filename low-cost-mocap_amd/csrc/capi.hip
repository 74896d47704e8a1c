// capi.hip -- the C ABI of include/mocap_core.h: context, options, camera tables, triangulation, object
// locator, track compaction (the frame path: frame_capi.hip; the blob stage: blob_capi.hip).  Host runtime only;
// all arithmetic of the hot path happens in the HIP kernels (frame_kernel.hip, tri_kernel.hip, ba_kernels.hip).
// The only host-side numerics are the frame-invariant camera tables (P = K[R|t], the C x C fundamental table)
// and the n x n trust-region algebra of the LM loop (ba_solve.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mocap_core.h"
#include "ctx.hpp"

using namespace mocap;

// ------------------------------------------------------------------ helpers
int mocap_ctx::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  {
    std::lock_guard<std::mutex> lk(err_mu);
    err = buf;
  }
  return code;
}

int mocap_ctx::hip_fail(hipError_t e, const char* what) {
  frame_q_dirty();  // a launch that failed or aborted may have left the self-cleaning queue counters dirty
  return fail(MOCAP_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

// after a "_dev" entry point enqueued work that is still running when it returns
int mocap_ctx::mark_enqueued() {
  hipError_t e = handover_event.ready();
  if (e != hipSuccess) return hip_fail(e, "hipEventCreateWithFlags(handover)");
  e = hipEventRecord(handover_event.ev, stream);
  if (e != hipSuccess) return hip_fail(e, "hipEventRecord(handover)");
  dev_outstanding = true;
  return MOCAP_OK;
}

int DevBuf::reserve(size_t bytes) {
  if (bytes <= cap) return 0;
  if (ptr) (void)hipFree(ptr);
  ptr = nullptr;
  cap = 0;
  size_t want = bytes + bytes / 4 + 256;
  hipError_t e = hipMalloc(&ptr, want);
  if (e != hipSuccess) {
    ptr = nullptr;
    return -1;
  }
  cap = want;
  return 0;
}

hipError_t PinBuf::reserve(size_t need, size_t want, unsigned flags) {
  if (need <= cap) return hipSuccess;
  if (ptr) (void)hipHostFree(ptr);
  ptr = nullptr;
  cap = 0;
  const hipError_t e = hipHostMalloc(&ptr, want, flags);
  if (e == hipSuccess) cap = want;
  return e;
}

int spin_wait(mocap_ctx* ctx, Event& event) {
  HIP_TRY(ctx, event.ready());
  HIP_TRY(ctx, hipEventRecord(event.ev, ctx->stream));
  for (long spins = 0;; spins++) {
    const hipError_t e = hipEventQuery(event.ev);
    if (e == hipSuccess) return MOCAP_OK;
    if (e != hipErrorNotReady) return ctx->hip_fail(e, "hipEventQuery");
    if (spins > 2000000) {  // seconds of polling: something is badly stuck, fall back to a blocking wait
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      return MOCAP_OK;
    }
  }
}

// ------------------------------------------------------------------ lifetime
extern "C" int mocap_create(int device_id, mocap_ctx** out) {
  if (!out) return MOCAP_E_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return MOCAP_E_HIP;
  mocap_ctx* c = new mocap_ctx();
  c->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreate(&c->own_stream) != hipSuccess) {
    delete c;
    return MOCAP_E_HIP;
  }
  c->stream = c->own_stream;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) c->num_cus = prop.multiProcessorCount;
  const char* t = getenv("MOCAP_FRAME_THREADS");
  if (t) {
    int v = atoi(t);
    if (v == 64 || v == 128 || v == 256) c->frame_threads = v;
  }
  if ((t = getenv("MOCAP_HEAVY_THRESHOLD"))) c->heavy_threshold = atoi(t);  // 0 disables splitting
  if ((t = getenv("MOCAP_SLICE_SIZE"))) c->slice_size = atoi(t);
  if ((t = getenv("MOCAP_FORCE_WIDE"))) c->force_wide = atoi(t) ? 1 : 0;
  if ((t = getenv("MOCAP_PRUNE"))) c->prune = atoi(t) ? 1 : 0;
  if ((t = getenv("MOCAP_EIGCUT"))) c->eigcut = atoi(t) ? 1 : 0;
  if ((t = getenv("MOCAP_EVAL_BB"))) c->eval_bb = atoi(t) ? 1 : 0;
  if ((t = getenv("MOCAP_BB_PL_MIN")) && atoi(t) >= 1 && atoi(t) <= 64) c->bb_pl_min = atoi(t);
  if ((t = getenv("MOCAP_BB_NB_MAX")) && atoi(t) >= 1) c->bb_nb_max = atoi(t);
  if (c->bb_pl_min > c->bb_pl) c->bb_pl_min = c->bb_pl;
  if ((t = getenv("MOCAP_BB_PL")) && atoi(t) >= 1 && atoi(t) <= 64) c->bb_pl = c->bb_pl_min = atoi(t);  // one size for every root: at least this many candidates per block
  if ((t = getenv("MOCAP_BB_FLUSH")) && atoi(t) >= 1) c->bb_flush = atoi(t);
  if ((t = getenv("MOCAP_BB_MIN_G")) && atoi(t) >= 0) c->bb_min_g = atoi(t);
  if ((t = getenv("MOCAP_FRAME_LAUNCHES"))) c->frame_launches = atoi(t) == 3 ? 3 : 1;  // 3: main / slice / merge launches (A/B)  // 0: every group is reprojected in full (A/B)
  *out = c;
  return MOCAP_OK;
}

extern "C" void mocap_destroy(mocap_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;  // every buffer and event is freed by the member that holds it
}

// The message is copied, under the error string's own lock, into a buffer owned by the CALLING thread: another thread's
// failing call may rewrite ctx->err at any time (Flask-SocketIO handlers vs the MJPEG generator share one context).
extern "C" const char* mocap_last_error(const mocap_ctx* ctx) {
  if (!ctx) return "null context";
  static thread_local std::string mine;
  {
    std::lock_guard<std::mutex> lk(const_cast<mocap_ctx*>(ctx)->err_mu);
    mine = ctx->err;
  }
  return mine.c_str();
}
extern "C" const char* mocap_version(void) { return "mocap_core 0.1 (gfx950)"; }

extern "C" int mocap_set_stream(mocap_ctx* ctx, void* hip_stream) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  hipStream_t ns = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  // The per-context workspaces (work queues that clean themselves at the END of a launch, scratch) are shared by whatever
  // stream is current: work a "_dev" entry point left running on the previous stream must finish before the first launch
  // on the new one.  Ordered on the DEVICE (the new stream waits for the event recorded behind that work): the previous
  // stream belongs to the caller and may be destroyed by now, the host does not block under the context lock, and the
  // calling thread's current device is put back.
  if (ns != ctx->stream && ctx->dev_outstanding) {
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipError_t e = hipStreamWaitEvent(ns, ctx->handover_event.ev, 0);
    if (prev_dev >= 0 && prev_dev != ctx->device) (void)hipSetDevice(prev_dev);
    if (e != hipSuccess) return ctx->hip_fail(e, "hipStreamWaitEvent(handover)");
    ctx->frame_q_dirty();
  }
  ctx->stream = ns;
  return MOCAP_OK;
}

extern "C" const char* mocap_last_frame_kernel(mocap_ctx* ctx) {
  if (!ctx) return "none";
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ctx->last_frame_kernel;  // string literals: valid for the life of the library
}

extern "C" int mocap_synchronize(mocap_ctx* ctx) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->dev_outstanding = false;
  return MOCAP_OK;
}

extern "C" int mocap_set_options(mocap_ctx* ctx, uint32_t flags) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->flags = flags;
  ctx->cv.f32_rounding = (flags & MOCAP_OPT_F32_ROUNDING) ? 1 : 0;
  ctx->exhaustive = (flags & MOCAP_OPT_EXHAUSTIVE_WALK) ? 1 : 0;
  return MOCAP_OK;
}

extern "C" int mocap_set_tuning(mocap_ctx* ctx, int frame_threads, int heavy_threshold, int slice_size) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (frame_threads != 0 && frame_threads != 64 && frame_threads != 128 && frame_threads != 256)
    return ctx->fail(MOCAP_E_ARG, "mocap_set_tuning: frame_threads must be 0, 64, 128 or 256");
  ctx->frame_threads = frame_threads;  // 0 = automatic
  ctx->heavy_threshold = heavy_threshold < 0 ? -1 : heavy_threshold;
  ctx->slice_size = slice_size < 0 ? 0 : slice_size;
  return MOCAP_OK;
}

extern "C" int mocap_set_frame_limits(mocap_ctx* ctx, int hit_cap, int force_wide) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (hit_cap < 0 || hit_cap > kMaxBlobs) return ctx->fail(MOCAP_E_ARG, "mocap_set_frame_limits: hit_cap must be 0..%d", kMaxBlobs);
  if (hit_cap) ctx->hit_cap = hit_cap;
  ctx->force_wide = force_wide ? 1 : 0;
  return MOCAP_OK;
}

extern "C" void mocap_limits(int* max_cameras, int* max_blobs) {
  if (max_cameras) *max_cameras = kMaxCameras;
  if (max_blobs) *max_blobs = kMaxBlobs;
}

// ------------------------------------------------------------------ cameras
namespace {

// cv::determinant for a 4x4 CV_64F (OpenCV core/src/lapack.cpp -> hal::LU64f, partial pivoting,
// eps = 100*DBL_EPSILON, p * prod(diag)); used by cv.sfm.fundamentalFromProjections (helpers.py:362).
// This TU is compiled with -ffp-contract=off so the loop rounds like the scalar x86-64 build.
double det4_lu(const double* M) {
  double A[16];
  memcpy(A, M, sizeof A);
  double p = 1.0;
  const double eps = 2.220446049250313e-16 * 100;
  for (int i = 0; i < 4; i++) {
    int k = i;
    for (int j = i + 1; j < 4; j++)
      if (std::fabs(A[j * 4 + i]) > std::fabs(A[k * 4 + i])) k = j;
    if (std::fabs(A[k * 4 + i]) < eps) return 0.0;
    if (k != i) {
      for (int j = i; j < 4; j++) std::swap(A[i * 4 + j], A[k * 4 + j]);
      p = -p;
    }
    const double d = -1.0 / A[i * 4 + i];
    for (int j = i + 1; j < 4; j++) {
      const double alpha = A[j * 4 + i] * d;
      for (int kk = i + 1; kk < 4; kk++) A[j * 4 + kk] = A[j * 4 + kk] + alpha * A[i * 4 + kk];
    }
  }
  double r = p;
  for (int i = 0; i < 4; i++) r = r * A[i * 4 + i];
  return r;
}

void projection(const double* K, const double* R, const double* t, double* P) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) {
      const double r0 = c < 3 ? R[c] : t[0], r1 = c < 3 ? R[3 + c] : t[1], r2 = c < 3 ? R[6 + c] : t[2];
      P[r * 4 + c] = K[r * 3 + 0] * r0 + K[r * 3 + 1] * r1 + K[r * 3 + 2] * r2;
    }
}

void fundamental(const double* P1, const double* P2, double* F) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double XY[16];
      memcpy(XY + 0, P1 + 4 * ((j + 1) % 3), 32);
      memcpy(XY + 4, P1 + 4 * ((j + 2) % 3), 32);
      memcpy(XY + 8, P2 + 4 * ((i + 1) % 3), 32);
      memcpy(XY + 12, P2 + 4 * ((i + 2) % 3), 32);
      F[i * 3 + j] = det4_lu(XY);
    }
}

}  // namespace

extern "C" int mocap_set_cameras(mocap_ctx* ctx, int C, const double* K, const double* R, const double* t) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!K || !R || !t || C < 1) return ctx->fail(MOCAP_E_ARG, "mocap_set_cameras: bad argument");
  if (C > kMaxCameras) return ctx->fail(MOCAP_E_LIMIT, "mocap_set_cameras: C=%d exceeds %d", C, kMaxCameras);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->hK.assign(K, K + 9 * C);
  ctx->hR.assign(R, R + 9 * C);
  ctx->ht.assign(t, t + 3 * C);
  bool uniform = true;
  for (int i = 1; i < C && uniform; i++) uniform = memcmp(K, K + 9 * i, 72) == 0;
  // layout of the device table block (doubles): Pq | RT | K4 | F | K9 | P
  const size_t nPq = uniform ? (size_t)12 * C : (size_t)12 * C * C;
  const size_t nRT = (size_t)12 * C, nK4 = (size_t)4 * C, nF = (size_t)9 * C * C, nK9 = (size_t)9 * C;
  std::vector<double> h(nPq + nRT + nK4 + nF + nK9 + nRT, 0.0);
  double* Pq = h.data();
  double* RT = Pq + nPq;
  double* K4 = RT + nRT;
  double* F = K4 + nK4;
  double* K9 = F + nF;
  std::vector<double> Ptrue((size_t)12 * C);
  for (int c = 0; c < C; c++) {
    projection(K + 9 * c, R + 9 * c, t + 3 * c, Ptrue.data() + 12 * c);
    memcpy(RT + 12 * c, R + 9 * c, 72);
    memcpy(RT + 12 * c + 9, t + 3 * c, 24);
    K4[4 * c + 0] = K[9 * c + 0];
    K4[4 * c + 1] = K[9 * c + 4];
    K4[4 * c + 2] = K[9 * c + 2];
    K4[4 * c + 3] = K[9 * c + 5];
  }
  if (uniform) {
    memcpy(Pq, Ptrue.data(), sizeof(double) * 12 * C);
  } else {
    // intrinsics by compacted view index j, pose by camera (helpers.py:296-298,305-307)
    for (int j = 0; j < C; j++)
      for (int c = j; c < C; c++) projection(K + 9 * j, R + 9 * c, t + 3 * c, Pq + 12 * ((size_t)j * C + c));
  }
  for (int a = 0; a < C; a++)
    for (int b = 0; b < C; b++)
      if (a != b) fundamental(Ptrue.data() + 12 * a, Ptrue.data() + 12 * b, F + 9 * ((size_t)a * C + b));
  memcpy(K9, K, sizeof(double) * 9 * C);
  memcpy(K9 + nK9, Ptrue.data(), sizeof(double) * 12 * C);  // each camera's own K: the table of the point refinement
  ctx->hF.assign(F, F + nF);
  ctx->hPown = Ptrue;

  // a frame call may be in flight on another stream of the same context: the mutex serialises
  // host calls; wait for queued device work before replacing the tables it reads.
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->tables.reserve(h.size() * sizeof(double))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(camera tables) failed");
  HIP_TRY(ctx, hipMemcpyAsync(ctx->tables.ptr, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const double* d = (const double*)ctx->tables.ptr;
  ctx->C = C;
  ctx->cv.C = C;
  ctx->cv.uniformK = uniform ? 1 : 0;
  ctx->cv.f32_rounding = (ctx->flags & MOCAP_OPT_F32_ROUNDING) ? 1 : 0;
  ctx->cv.Pq = d;
  ctx->cv.RT = d + nPq;
  ctx->cv.K4 = ctx->cv.RT + nRT;
  ctx->cv.F = ctx->cv.K4 + nK4;
  ctx->d_K9 = ctx->cv.F + nF;
  ctx->d_Pown = ctx->d_K9 + nK9;
  // EigCut (mocap_device.hpp): the bound equates the DLT rows' residual with cv.projectPoints', which holds when every
  // K is [[fx,0,cx],[0,fy,cy],[0,0,1]] (projectPoints reads fx, fy, cx, cy only); then P[2] = (R[2], t[2])
  bool plainK = true;
  double p3 = 0.0;
  for (int c = 0; c < C; c++) {
    const double* k = K + 9 * c;
    plainK = plainK && k[1] == 0.0 && k[3] == 0.0 && k[6] == 0.0 && k[7] == 0.0 && k[8] == 1.0;
    const double* r = R + 9 * c;
    p3 = std::fmax(p3, r[6] * r[6] + r[7] * r[7] + r[8] * r[8] + t[3 * c + 2] * t[3 * c + 2]);
  }
  ctx->p3max2 = plainK && std::isfinite(p3) ? p3 * (1.0 + 1e-5) : 0.0;
  // the branch and bound takes its bounds in a frame whose origin is the point closest (least squares) to all optical
  // axes -- any point gives a valid bound, one inside the working volume gives a tight one (eigcut_s1_shifted)
  double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bb[3] = {0, 0, 0};
  for (int c = 0; c < C; c++) {
    const double* r = R + 9 * c;
    const double* tt = t + 3 * c;
    const double d[3] = {r[6], r[7], r[8]};  // optical axis (R is orthonormal up to the user's rounding)
    const double o[3] = {-(r[0] * tt[0] + r[3] * tt[1] + r[6] * tt[2]), -(r[1] * tt[0] + r[4] * tt[1] + r[7] * tt[2]),
                         -(r[2] * tt[0] + r[5] * tt[1] + r[8] * tt[2])};  // camera centre -R^T t
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        const double pij = (i == j ? 1.0 : 0.0) - d[i] * d[j];
        A[3 * i + j] += pij;
        bb[i] += pij * o[j];
      }
  }
  double c0[3] = {0, 0, 0};
  {
    const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    if (std::isfinite(det) && std::fabs(det) > 1e-6 * C * C * C) {  // (parallel axes: keep the world origin)
      c0[0] = (bb[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (bb[1] * A[8] - A[5] * bb[2]) + A[2] * (bb[1] * A[7] - A[4] * bb[2])) / det;
      c0[1] = (A[0] * (bb[1] * A[8] - A[5] * bb[2]) - bb[0] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * bb[2] - bb[1] * A[6])) / det;
      c0[2] = (A[0] * (A[4] * bb[2] - bb[1] * A[7]) - A[1] * (A[3] * bb[2] - bb[1] * A[6]) + bb[0] * (A[3] * A[7] - A[4] * A[6])) / det;
      if (!(std::isfinite(c0[0]) && std::isfinite(c0[1]) && std::isfinite(c0[2]))) c0[0] = c0[1] = c0[2] = 0.0;
    }
  }
  double p3c = 0.0;
  for (int c = 0; c < C; c++) {
    const double* r = R + 9 * c;
    const double w = r[6] * c0[0] + r[7] * c0[1] + r[8] * c0[2] + t[3 * c + 2];
    p3c = std::fmax(p3c, r[6] * r[6] + r[7] * r[7] + r[8] * r[8] + w * w);
  }
  for (int i = 0; i < 3; i++) ctx->eig_c0[i] = c0[i];
  ctx->p3max2c = plainK && std::isfinite(p3c) ? p3c * (1.0 + 1e-5) : 0.0;
  return MOCAP_OK;
}

extern "C" int mocap_set_world_transform(mocap_ctx* ctx, const double* to_world) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!to_world) {
    ctx->world_on = false;
    return MOCAP_OK;
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a queued frame batch may still read the old matrix
  if (ctx->world.reserve(16 * sizeof(double))) return ctx->fail(MOCAP_E_HIP, "hipMalloc(world matrix) failed");
  HIP_TRY(ctx, hipMemcpyAsync(ctx->world.ptr, to_world, 16 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->world_on = true;
  return MOCAP_OK;
}

extern "C" int mocap_get_fundamental(mocap_ctx* ctx, double* F) {
  if (!ctx || !F) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
  memcpy(F, ctx->hF.data(), ctx->hF.size() * sizeof(double));
  return MOCAP_OK;
}

// ------------------------------------------------------------------ triangulation
static int triangulate_dev_locked(mocap_ctx* ctx, int64_t N, const double* d_obs, double* d_xyz, double* d_err) {
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
  if (N < 0 || (N > 0 && !d_obs)) return ctx->fail(MOCAP_E_ARG, "mocap_triangulate: bad argument");
  TriArgs a;
  a.cv = ctx->cv;
  a.N = N;
  a.P = 1;
  a.stride_Pq = a.stride_RT = 0;
  a.obs = d_obs;
  a.xyz = d_xyz;
  a.err = d_err;
  a.xyz_in = nullptr;
  HIP_TRY(ctx, launch_triangulate(a, ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_triangulate_dev(mocap_ctx* ctx, int64_t N, const double* d_obs, double* d_xyz, double* d_err) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = triangulate_dev_locked(ctx, N, d_obs, d_xyz, d_err);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_triangulate(mocap_ctx* ctx, int64_t N, const double* obs, double* xyz, double* err) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
  if (N < 0 || (N > 0 && (!obs || !xyz))) return ctx->fail(MOCAP_E_ARG, "mocap_triangulate: bad argument");
  if (N == 0) return MOCAP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int C = ctx->C;
  const size_t b_obs = sizeof(double) * (size_t)N * C * 2, b_xyz = sizeof(double) * (size_t)N * 3,
               b_err = sizeof(double) * (size_t)N;
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(b_obs + b_xyz + b_err)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%zu) failed", b_obs + b_xyz + b_err);
  double* d_obs = (double*)s.ptr;
  double* d_xyz = d_obs + (size_t)N * C * 2;
  double* d_err = d_xyz + (size_t)N * 3;
  HIP_TRY(ctx, hipMemcpyAsync(d_obs, obs, b_obs, hipMemcpyHostToDevice, ctx->stream));
  int rc = triangulate_dev_locked(ctx, N, d_obs, d_xyz, d_err);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(xyz, d_xyz, b_xyz, hipMemcpyDeviceToHost, ctx->stream));
  if (err) HIP_TRY(ctx, hipMemcpyAsync(err, d_err, b_err, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

extern "C" int mocap_reproject(mocap_ctx* ctx, int64_t N, const double* obs, const double* xyz, double* err) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
  if (N < 0 || (N > 0 && (!obs || !xyz || !err))) return ctx->fail(MOCAP_E_ARG, "mocap_reproject: bad argument");
  if (N == 0) return MOCAP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int C = ctx->C;
  const size_t b_obs = sizeof(double) * (size_t)N * C * 2, b_xyz = sizeof(double) * (size_t)N * 3,
               b_err = sizeof(double) * (size_t)N;
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(b_obs + b_xyz + b_err)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(%zu) failed", b_obs + b_xyz + b_err);
  double* d_obs = (double*)s.ptr;
  double* d_xyz = d_obs + (size_t)N * C * 2;
  double* d_err = d_xyz + (size_t)N * 3;
  HIP_TRY(ctx, hipMemcpyAsync(d_obs, obs, b_obs, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_xyz, xyz, b_xyz, hipMemcpyHostToDevice, ctx->stream));
  TriArgs a;
  a.cv = ctx->cv;
  a.N = N;
  a.P = 1;
  a.stride_Pq = a.stride_RT = 0;
  a.obs = d_obs;
  a.xyz = nullptr;
  a.err = d_err;
  a.xyz_in = d_xyz;
  HIP_TRY(ctx, launch_triangulate(a, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(err, d_err, b_err, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}

// ------------------------------------------------------------------ object locator
// (internal, ctx.hpp: mocap_track_frame_dev in frame_capi.hip enqueues it behind the frame path)
int locate_dev_locked(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz, const double* d_err,
                      const int32_t* d_n_pts, int O_max, double* d_pos, double* d_heading, double* d_oerr,
                      int32_t* d_drone, int32_t* d_lead, int32_t* d_n_obj) {
  if (n_frames < 0 || K_max < 1 || O_max < 1) return ctx->fail(MOCAP_E_ARG, "mocap_locate_objects: bad size argument");
  if (K_max > 256) return ctx->fail(MOCAP_E_LIMIT, "mocap_locate_objects: K_max=%d exceeds 256", K_max);
  if (n_frames == 0) return MOCAP_OK;
  if (!d_xyz || !d_err || !d_n_pts || !d_pos || !d_heading || !d_oerr || !d_drone || !d_n_obj)
    return ctx->fail(MOCAP_E_ARG, "mocap_locate_objects: null buffer");
  LocateArgs a;
  a.n_frames = n_frames;
  a.K_max = K_max;
  a.O_max = O_max;
  a.xyz = d_xyz;
  a.err = d_err;
  a.n_pts = d_n_pts;
  a.obj_pos = d_pos;
  a.obj_heading = d_heading;
  a.obj_err = d_oerr;
  a.obj_drone = d_drone;
  a.obj_lead = d_lead;
  a.n_obj = d_n_obj;
  // small batches: one wave per frame (latency); big ones: one lane per frame (throughput).  Same results (tested);
  // MOCAP_LOCATE_KERNEL=lane|wave forces one.
  bool wave = n_frames < 16384;
  if (const char* k = getenv("MOCAP_LOCATE_KERNEL")) wave = k[0] == 'w';
  if (wave) {
    TrackExportArgs e;
    memset(&e, 0, sizeof e);
    HIP_TRY(ctx, launch_track_export(a, e, ctx->stream));
  } else {
    HIP_TRY(ctx, launch_locate_objects(a, ctx->stream));
  }
  return MOCAP_OK;
}

extern "C" int mocap_track_record_bytes(int C) { return C < 1 ? 0 : (32 + 2 * C + 7) / 8 * 8; }

extern "C" int mocap_compact_tracks_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const int32_t* d_n_out,
                                        const double* d_xyz, const double* d_err, const int16_t* d_corr,
                                        int64_t* d_offsets, void* d_records, int64_t capacity, int64_t* d_total) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->C) return ctx->fail(MOCAP_E_NOCAMS, "mocap_set_cameras has not been called");
  if (n_frames < 0 || K_max < 1 || capacity < 0) return ctx->fail(MOCAP_E_ARG, "mocap_compact_tracks: bad size argument");
  if (n_frames == 0) return MOCAP_OK;
  if (!d_n_out || !d_xyz || !d_err || !d_corr || !d_offsets || (!d_records && capacity > 0))
    return ctx->fail(MOCAP_E_ARG, "mocap_compact_tracks: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n_blocks = (size_t)((n_frames + 1023) / 1024);
  if (ctx->compact_ws.reserve(sizeof(int64_t) * n_blocks)) return ctx->fail(MOCAP_E_HIP, "hipMalloc(scan workspace) failed");
  CompactArgs a;
  a.n_frames = n_frames;
  a.K_max = K_max;
  a.C = ctx->C;
  a.stride = mocap_track_record_bytes(ctx->C);
  a.n_out = d_n_out;
  a.xyz = d_xyz;
  a.err = d_err;
  a.corr = d_corr;
  a.offsets = d_offsets;
  a.block_sums = (int64_t*)ctx->compact_ws.ptr;
  a.records = (unsigned char*)d_records;
  a.capacity = capacity;
  a.total = d_total;
  HIP_TRY(ctx, launch_compact_tracks(a, ctx->stream));
  return ctx->mark_enqueued();
}

extern "C" int mocap_locate_objects_dev(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* d_xyz,
                                        const double* d_err, const int32_t* d_n_pts, int O_max, double* d_pos,
                                        double* d_heading, double* d_oerr, int32_t* d_drone, int32_t* d_lead,
                                        int32_t* d_n_obj) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = locate_dev_locked(ctx, n_frames, K_max, d_xyz, d_err, d_n_pts, O_max, d_pos, d_heading, d_oerr, d_drone,
                                   d_lead, d_n_obj);
  return rc ? rc : ctx->mark_enqueued();
}

extern "C" int mocap_locate_objects(mocap_ctx* ctx, int64_t n_frames, int K_max, const double* xyz, const double* err,
                                    const int32_t* n_pts, int O_max, double* pos, double* heading, double* oerr,
                                    int32_t* drone, int32_t* lead, int32_t* n_obj) {
  if (!ctx) return MOCAP_E_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n_frames < 0 || K_max < 1 || O_max < 1) return ctx->fail(MOCAP_E_ARG, "mocap_locate_objects: bad size argument");
  if (n_frames == 0) return MOCAP_OK;
  if (!xyz || !err || !n_pts || !pos || !heading || !oerr || !drone || !n_obj)
    return ctx->fail(MOCAP_E_ARG, "mocap_locate_objects: null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t F = (size_t)n_frames;
  double *d_xyz, *d_err, *d_pos, *d_head, *d_oerr;
  int32_t *d_n, *d_nobj, *d_drone, *d_lead;
  auto lay = [&](void* base) {
    Carver c(base);
    d_xyz = c.take<double>(F * K_max * 3);
    d_err = c.take<double>(F * K_max);
    d_pos = c.take<double>(F * O_max * 3);
    d_head = c.take<double>(F * O_max);
    d_oerr = c.take<double>(F * O_max);
    d_n = c.take<int32_t>(F);
    d_nobj = c.take<int32_t>(F);
    d_drone = c.take<int32_t>(F * O_max);
    d_lead = c.take<int32_t>(F * O_max);
    return c.off;
  };
  DevBuf& s = ctx->scratch[0];
  if (s.reserve(lay(nullptr))) return ctx->fail(MOCAP_E_HIP, "hipMalloc failed");
  lay(s.ptr);
  HIP_TRY(ctx, hipMemcpyAsync(d_xyz, xyz, sizeof(double) * F * K_max * 3, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_err, err, sizeof(double) * F * K_max, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_n, n_pts, sizeof(int32_t) * F, hipMemcpyHostToDevice, ctx->stream));
  int rc = locate_dev_locked(ctx, n_frames, K_max, d_xyz, d_err, d_n, O_max, d_pos, d_head, d_oerr, d_drone, d_lead, d_nobj);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(pos, d_pos, sizeof(double) * F * O_max * 3, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(heading, d_head, sizeof(double) * F * O_max, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(oerr, d_oerr, sizeof(double) * F * O_max, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(drone, d_drone, sizeof(int32_t) * F * O_max, hipMemcpyDeviceToHost, ctx->stream));
  if (lead) HIP_TRY(ctx, hipMemcpyAsync(lead, d_lead, sizeof(int32_t) * F * O_max, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(n_obj, d_nobj, sizeof(int32_t) * F, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MOCAP_OK;
}
