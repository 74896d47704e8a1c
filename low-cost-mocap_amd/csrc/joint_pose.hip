// joint_pose.hip -- bodies with hidden markers posed through their joints (include/mocap_core.h, "joint poses").
//   put      the host's table of directed joints into device memory: a chunk of 24 per launch travels as a kernel argument, as
//            body_session.hip's bodies do, so a "_dev" call needs neither a host buffer that outlives it nor a wait.
//   init     round 0, one lane per (body, frame): a POSED frame's pose is copied with hops = 0, every other frame starts at -1.
//   round    one launch per round r, bp_pose_kernel's layout: one lane per (body y, frame), grid ceil(F / 256) x B, frames along the
//            lanes.  The body, its joints and their masks are the same for the whole workgroup: scalar loads.  A lane that is a
//            candidate walks y's joints in ascending index and tries those whose other body x has hops = r - 1; a try is
//            bp_pose_kernel's fit over the present markers and the joint's one or two virtual points, the markers' points read
//            three times instead of being kept, for that kernel's reason.  Centroids, cross-covariance and residual are written
//            out here with the points in list order; Horn's matrix, the Jacobi sweep, the top eigenvector and quaternion -> R are
//            rb_pose.hpp's own functions.
//            hops has ONE plane.  A lane reads hops[x][f] while the workgroup of body x may be setting it from -1 to r in the same
//            launch: either value differs from r - 1, so the lane does not try that joint either way, and x's pose is read only
//            where hops[x][f] = r - 1, which an earlier launch wrote.  The outcome does not depend on the race.
//   sign     sign_walk.hpp over the frames whose flag_j is POSED or JOINTED: the tiles' last such frame, then stage 1's four launches.
// FP64 throughout, nothing fused (-ffp-contract=off is the build's rule), / and sqrt correctly rounded.
#include "joint_pose.hpp"
#include "mocap_device.hpp"
#include "rb_pose.hpp"
#include "sign_walk.hpp"

namespace mocap {

namespace {

constexpr int kT = kTsTile;

struct JpOnPosedOrJointed {  // the frames that carry a quaternion (sign_walk.hpp)
  __device__ static bool on(int32_t flag) { return flag == kBpPosed || flag == kBpJointed; }
};

// ------------------------------------------------------------------------------------------------------------------ joint table
__global__ __launch_bounds__(64) void jp_put_kernel(JpDirChunk c, int count, JpDir* dst) {
  constexpr int kWords = (int)(sizeof(JpDir) / sizeof(unsigned long long));
  static_assert(sizeof(JpDir) % sizeof(unsigned long long) == 0, "copied as 64-bit words");
  static_assert(sizeof(JpDirChunk) + sizeof(int) + sizeof(JpDir*) <= 4096, "the chunk travels as a kernel argument");
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&c);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(dst);
  for (int i = threadIdx.x; i < count * kWords; i += 64) out[i] = src[i];
}

// ------------------------------------------------------------------------------------------------------------------ round 0
__global__ __launch_bounds__(kT) void jp_init_kernel(PoseJointsArgs a) {
  const int b = blockIdx.y;
  const int64_t F = a.n_frames, f = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (f >= F) return;
  const size_t o = (size_t)b * F + f;
  const double nan = __builtin_nan("");
  const int flag = a.flag[o];
  const bool posed = flag == kBpPosed;
  a.flag_j[o] = flag;
  a.hops[o] = posed ? 0 : -1;
  a.via[o] = -1;
  a.rms_j[o] = nan;
#pragma unroll
  for (int i = 0; i < 4; i++) a.quat_j[4 * o + i] = posed ? a.quat[4 * o + i] : nan;
#pragma unroll
  for (int i = 0; i < 9; i++) a.Rm_j[9 * o + i] = posed ? a.Rm[9 * o + i] : nan;
#pragma unroll
  for (int i = 0; i < 3; i++) a.t_j[3 * o + i] = posed ? a.t_pose[3 * o + i] : nan;
}

// ------------------------------------------------------------------------------------------------------------------ round r
// one point of the list into the cross-covariance, and into the residual: stage 1's lines
__device__ __forceinline__ void jp_cov(double S[3][3], const double* q, const double* qb, const double* p, const double* pb) {
  double mq[3], wp[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    mq[k] = q[k] - qb[k];
    wp[k] = p[k] - pb[k];
  }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) S[i][j] = S[i][j] + mq[i] * wp[j];
}

__device__ __forceinline__ void jp_res(double& ss, const double* R, const double* q, const double* qb, const double* p, const double* pb) {
  double mq[3];
#pragma unroll
  for (int k = 0; k < 3; k++) mq[k] = q[k] - qb[k];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double r = ((R[3 * i] * mq[0] + R[3 * i + 1] * mq[1]) + R[3 * i + 2] * mq[2]) - (p[i] - pb[i]);
    ss = ss + r * r;
  }
}

__global__ __launch_bounds__(kT) void jp_round_kernel(PoseJointsArgs a, int r) {
  const int y = blockIdx.y;
  const int64_t F = a.n_frames, f = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int d0 = a.first[y], d1 = a.first[y + 1];
  if (f >= F || d0 == d1) return;
  const size_t o = (size_t)y * F + f;
  if (a.hops[o] != -1) return;
  const int flag = a.flag[o];
  if (flag != kBpFew && flag != kBpDegenerate) return;  // (an RMS frame is never a candidate)

  const BpBody* __restrict__ body = a.bodies + y;
  const int N = body->n;
  const double* __restrict__ P = a.traj + (size_t)f * 3;
  const size_t rs = (size_t)F * 3;  // doubles per row
  double qs[3] = {0, 0, 0}, ps[3] = {0, 0, 0};  // the sums over the present markers: the same at every try
  unsigned pres = 0;
  int k = 0;
#pragma unroll
  for (int m = 0; m < kBpMaxMarkers; m++)
    if (m < N) {
      const double* p = P + (size_t)body->rows[m] * rs;
      const double px = p[0], py = p[1], pz = p[2];
      if (finite1(px) && finite1(py) && finite1(pz)) {
        pres |= 1u << m;
        k++;
        qs[0] = qs[0] + body->q[m][0];
        qs[1] = qs[1] + body->q[m][1];
        qs[2] = qs[2] + body->q[m][2];
        ps[0] = ps[0] + px;
        ps[1] = ps[1] + py;
        ps[2] = ps[2] + pz;
      }
    }

  for (int d = d0; d < d1; d++) {
    const JpDir* __restrict__ jt = a.dirs + d;
    const size_t ox = (size_t)jt->x * F + f;
    // (the one racy read: -1 or r while x's workgroup runs, never r - 1 unless an earlier launch wrote it)
    if (__hip_atomic_load(a.hops + ox, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != r - 1) continue;
    if (!((jt->mask[pres >> 6] >> (pres & 63)) & 1ull)) continue;  // not possible
    const bool hinge = jt->kind == kJtHinge;
    const double* Rx = a.Rm_j + 9 * ox;
    const double* tx = a.t_j + 3 * ox;
    double w0[3], w1[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      w0[i] = ((Rx[3 * i] * jt->c_x[0] + Rx[3 * i + 1] * jt->c_x[1]) + Rx[3 * i + 2] * jt->c_x[2]) + tx[i];
      const double u = (Rx[3 * i] * jt->ax_x[0] + Rx[3 * i + 1] * jt->ax_x[1]) + Rx[3 * i + 2] * jt->ax_x[2];
      w1[i] = w0[i] + a.axis_len * u;
    }
    const int count = k + (hinge ? 2 : 1);
    const double inv_c = 1.0 / (double)count;
    double qb[3], pb[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      qb[i] = qs[i] + jt->v0[i];
      pb[i] = ps[i] + w0[i];
      if (hinge) {
        qb[i] = qb[i] + jt->v1[i];
        pb[i] = pb[i] + w1[i];
      }
      qb[i] = qb[i] * inv_c;
      pb[i] = pb[i] * inv_c;
    }
    double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // S[i][j] = sum (q - qb)_i (p - pb)_j
#pragma unroll
    for (int m = 0; m < kBpMaxMarkers; m++)
      if (m < N && (pres >> m & 1u)) jp_cov(S, body->q[m], qb, P + (size_t)body->rows[m] * rs, pb);
    jp_cov(S, jt->v0, qb, w0, pb);
    if (hinge) jp_cov(S, jt->v1, qb, w1, pb);
    double A[4][4], V[4][4];
    rb_horn_matrix(S, A);
    rb_jacobi4(A, V);
    double qw, qx, qy, qz, R[9], t[3];
    rb_top_quat(A, V, qw, qx, qy, qz);
    rb_quat_to_R(qw, qx, qy, qz, R);
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = pb[i] - ((R[3 * i] * qb[0] + R[3 * i + 1] * qb[1]) + R[3 * i + 2] * qb[2]);
    double ss = 0.0;
#pragma unroll
    for (int m = 0; m < kBpMaxMarkers; m++)
      if (m < N && (pres >> m & 1u)) jp_res(ss, R, body->q[m], qb, P + (size_t)body->rows[m] * rs, pb);
    jp_res(ss, R, jt->v0, qb, w0, pb);
    if (hinge) jp_res(ss, R, jt->v1, qb, w1, pb);
    const double rms = sqrt(ss * inv_c);
    if (!(finite1(qw) && finite1(qx) && finite1(qy) && finite1(qz) && rms <= a.max_rms)) continue;  // (a NaN rms fails)
    a.flag_j[o] = kBpJointed;
    a.via[o] = jt->j;
    a.rms_j[o] = rms;
    a.quat_j[4 * o] = qw;
    a.quat_j[4 * o + 1] = qx;
    a.quat_j[4 * o + 2] = qy;
    a.quat_j[4 * o + 3] = qz;
#pragma unroll
    for (int i = 0; i < 9; i++) a.Rm_j[9 * o + i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) a.t_j[3 * o + i] = t[i];
    a.hops[o] = r;
    break;
  }
}

}  // namespace

hipError_t launch_put_dirs(const JpDir* host, int n, JpDir* dev, hipStream_t stream) {
  for (int d0 = 0; d0 < n; d0 += kJpPutDirs) {
    JpDirChunk c{};
    const int count = n - d0 < kJpPutDirs ? n - d0 : kJpPutDirs;
    for (int i = 0; i < count; i++) c.d[i] = host[d0 + i];
    hipLaunchKernelGGL(jp_put_kernel, dim3(1), dim3(64), 0, stream, c, count, dev + d0);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

hipError_t launch_pose_joints(const PoseJointsArgs& a, int max_rounds, hipStream_t stream) {
  const dim3 block(kT), grid((unsigned)ts_tiles(a.n_frames), (unsigned)a.B);
  hipLaunchKernelGGL(jp_init_kernel, grid, block, 0, stream, a);
  if (hipError_t e = hipGetLastError()) return e;
  for (int r = 1; r <= max_rounds; r++) {
    hipLaunchKernelGGL(jp_round_kernel, grid, block, 0, stream, a, r);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return launch_sign_walk<JpOnPosedOrJointed>(SignWalkArgs{a.n_frames, a.flag_j, a.quat_j, a.tile_i32, a.parity}, a.B, true, stream);
}

}  // namespace mocap
