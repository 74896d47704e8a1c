// skeleton_fit.hip -- all joints of a frame closed at once (include/mocap_core.h, "skeleton fit").
//   put       the host's table of directed joints into device memory, 32 per launch inside a kernel argument, as joint_pose.hip's.
//   init      one lane per (body, frame): ACTIVE or not, the start pose (or NaN) into quat_s and t_s, lam and steps of the frame.
//   assemble  one lane per (body, frame), grid ceil(nf / 256) x B, frames along the lanes: the body's own block, gradient and cost
//             share at the current pose, and the coupling and cost share of the joint to its parent.  The lane walks the body's
//             directed joints as jp_round_kernel does, so every term has one writer and nothing is an atomic.
//   solve     one lane per frame, 64 lanes per workgroup: the frame's cost, then the elimination order serially -- L D L^T of
//             the block, M^-1 g, M^-1 C column by column, the complement and reduced gradient pushed into the parent's planes --
//             then the steps in reverse order and the trial poses.  The factors (21 doubles), the coupling (16) and one column
//             (6) live in registers with constant indices; nothing of a 6 x 6 block is in scratch.
//   trial     assemble's cost shares alone at the trial poses.
//   accept    one lane per frame: the trial cost, the decision, the poses and lam selected.
//   finish    one lane per (body, frame): Rm_s and rms_s at the returned pose, NaN for an inactive body.
//   sign      sign_walk.hpp over the frames whose input flag is POSED or JOINTED.
// The tables of the forest travel inside the kernel argument (SkArgs::fr): scalar loads, the same for the whole grid.
// FP64 throughout, nothing fused (-ffp-contract=off is the build's rule), / and sqrt correctly rounded.
#include "skeleton_fit.hpp"
#include "mocap_device.hpp"
#include "rb_pose.hpp"
#include "sign_walk.hpp"
#include "skeleton_fit_math.hpp"

namespace mocap {

namespace {

constexpr int kT = kTsTile;
constexpr int kSolveLanes = 64;

struct SkOnPosedOrJointed {  // the frames that carry a quaternion (sign_walk.hpp)
  __device__ static bool on(int32_t flag) { return flag == kBpPosed || flag == kBpJointed; }
};

__global__ __launch_bounds__(64) void sk_put_kernel(SkDirChunk c, int count, SkDir* dst) {
  constexpr int kWords = (int)(sizeof(SkDir) / sizeof(unsigned long long));
  static_assert(sizeof(SkDir) % sizeof(unsigned long long) == 0, "copied as 64-bit words");
  static_assert(sizeof(SkDirChunk) + sizeof(int) + sizeof(SkDir*) <= 4096, "the chunk travels as a kernel argument");
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&c);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(dst);
  for (int i = threadIdx.x; i < count * kWords; i += 64) out[i] = src[i];
}

static_assert(sizeof(SkArgs) + 16 <= 4096, "the forest travels as a kernel argument");

// plane k of body b, frame fl of the round
__device__ __forceinline__ double* sk_plane(const SkArgs& a, int b, int k, int64_t fl) {
  return a.ws + ((size_t)b * kSkPlanes + k) * (size_t)a.cap + fl;
}

// the current pose (quat_s, t_s) or the trial pose (the workspace) of body x
template <bool kTrial>
__device__ __forceinline__ void sk_load_pose(const SkArgs& a, int x, int64_t f, int64_t fl, double* q, double* t) {
  if (kTrial) {
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = *sk_plane(a, x, kSkTrial + i, fl);
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = *sk_plane(a, x, kSkTrial + 4 + i, fl);
  } else {
    const size_t o = (size_t)x * a.n_frames + f;
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = a.quat_s[4 * o + i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = a.t_s[3 * o + i];
  }
}

// ------------------------------------------------------------------------------------------------------------------ init
__global__ __launch_bounds__(kT) void sk_init_kernel(SkArgs a) {
  const int b = blockIdx.y;
  const int64_t fl = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (fl >= a.nf) return;
  const int64_t f = a.f0 + fl;
  const size_t o = (size_t)b * a.n_frames + f;
  const int flag = a.flag[o];
  bool on = flag == kBpPosed || flag == kBpJointed;
  double q[4], t[3];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    q[i] = a.quat[4 * o + i];
    on = on && finite1(q[i]);
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    t[i] = a.t_pose[3 * o + i];
    on = on && finite1(t[i]);
  }
  const double nan = __builtin_nan("");
#pragma unroll
  for (int i = 0; i < 4; i++) a.quat_s[4 * o + i] = on ? q[i] : nan;
#pragma unroll
  for (int i = 0; i < 3; i++) a.t_s[3 * o + i] = on ? t[i] : nan;
  a.act[(size_t)b * a.cap + fl] = on ? 1 : 0;
  if (b == 0) {
    a.lam[fl] = 1e-3;
    a.steps[f] = 0;
  }
}

// ------------------------------------------------------------------------------------------------------------------ a body's terms
// kGrad: block, gradient and coupling as well as the cost shares.  kTrial: at the trial poses, shares into the trial planes.
// kFinish: Rm_s and rms_s instead of shares.
template <bool kGrad, bool kTrial, bool kFinish>
__device__ __forceinline__ void sk_body(const SkArgs& a) {
  const int b = blockIdx.y;
  const int64_t fl = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (fl >= a.nf) return;
  const int64_t F = a.n_frames, f = a.f0 + fl;
  const size_t o = (size_t)b * F + f;
  const bool on = a.act[(size_t)b * a.cap + fl] != 0;
  if (kFinish && !on) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int i = 0; i < 9; i++) a.Rm_s[9 * o + i] = nan;
    a.rms_s[o] = nan;
    return;
  }
  if (!on) return;
  double q[4], t[3], R[9];
  sk_load_pose<kTrial>(a, b, f, fl, q, t);
  rb_quat_to_R(q[0], q[1], q[2], q[3], R);

  const BpBody* __restrict__ body = a.bodies + b;
  const int N = body->n;
  const double* __restrict__ P = a.traj + (size_t)f * 3;
  const size_t rs = (size_t)F * 3;  // doubles per row
  SkOwn own;
  sk_own_zero(own);
  double cb = 0.0;
  int k = 0;
#pragma unroll
  for (int m = 0; m < kBpMaxMarkers; m++)
    if (m < N) {
      const double* p = P + (size_t)body->rows[m] * rs;
      const double px = p[0], py = p[1], pz = p[2];
      if (finite1(px) && finite1(py) && finite1(pz)) {
        double y[3], r[3];
        sk_rot(R, body->q[m], y);
        r[0] = (y[0] + t[0]) - px;
        r[1] = (y[1] + t[1]) - py;
        r[2] = (y[2] + t[2]) - pz;
        cb = cb + ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
        k++;
        if (kGrad) sk_own_add(own, y, r, 1.0);
      }
    }
  if (kFinish) {
#pragma unroll
    for (int i = 0; i < 9; i++) a.Rm_s[9 * o + i] = R[i];
    a.rms_s[o] = k > 0 ? sqrt(cb / (double)k) : __builtin_nan("");
    return;
  }

  const double w = a.w_joint, len = a.axis_len;
  for (int d = a.fr.first[b]; d < a.fr.first[b + 1]; d++) {
    const SkDir* __restrict__ jt = a.dirs + d;
    const int x = jt->x;
    if (!a.act[(size_t)x * a.cap + fl]) continue;
    const bool hinge = jt->kind == kJtHinge;
    double qx[4], tx[3], Rx[9];
    sk_load_pose<kTrial>(a, x, f, fl, qx, tx);
    rb_quat_to_R(qx[0], qx[1], qx[2], qx[3], Rx);
    double yb[3], yx[3], ub[3], ux[3], y1b[3], y1x[3], r0[3], r1[3];
    sk_rot(R, jt->c_y, yb);
    sk_rot(Rx, jt->c_x, yx);
    sk_rot(R, jt->ax_y, ub);
    sk_rot(Rx, jt->ax_x, ux);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double wy = yb[i] + t[i], wx = yx[i] + tx[i];
      r0[i] = wy - wx;
      y1b[i] = yb[i] + len * ub[i];
      y1x[i] = yx[i] + len * ux[i];
      r1[i] = (wy + len * ub[i]) - (wx + len * ux[i]);
    }
    if (kGrad) {
      sk_own_add(own, yb, r0, w);
      if (hinge) sk_own_add(own, y1b, r1, w);
    }
    if (jt->up) {
      const double e0 = (r0[0] * r0[0] + r0[1] * r0[1]) + r0[2] * r0[2], e1 = (r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2];
      *sk_plane(a, b, kSkShare + (kTrial ? 3 : 1), fl) = hinge ? w * e0 + w * e1 : w * e0;
      if (kGrad) {
        SkUp c;
        sk_up_make(c, yb, yx, y1b, y1x, hinge, w);
#pragma unroll
        for (int e = 0; e < 9; e++) *sk_plane(a, b, kSkUp + e, fl) = c.G[e];
#pragma unroll
        for (int e = 0; e < 3; e++) {
          *sk_plane(a, b, kSkUp + 9 + e, fl) = c.u[e];
          *sk_plane(a, b, kSkUp + 12 + e, fl) = c.v[e];
        }
        *sk_plane(a, b, kSkUp + 15, fl) = c.n;
      }
    }
  }
  *sk_plane(a, b, kSkShare + (kTrial ? 2 : 0), fl) = cb;
  if (kGrad) {
    double H[21];
    sk_own_block(own, a.lam[fl], H);
#pragma unroll
    for (int e = 0; e < 21; e++) *sk_plane(a, b, kSkH + e, fl) = H[e];
#pragma unroll
    for (int e = 0; e < 6; e++) *sk_plane(a, b, kSkG + e, fl) = own.g[e];
  }
}

__global__ __launch_bounds__(kT) void sk_assemble_kernel(SkArgs a) { sk_body<true, false, false>(a); }
__global__ __launch_bounds__(kT) void sk_trial_kernel(SkArgs a) { sk_body<false, true, false>(a); }
__global__ __launch_bounds__(kT) void sk_finish_kernel(SkArgs a) { sk_body<false, false, true>(a); }

// the frame's cost from the shares: the active bodies in ascending b, then the active joints in ascending joint index
template <bool kTrial>
__device__ __forceinline__ double sk_frame_cost(const SkArgs& a, int64_t fl, int& n_act) {
  double c = 0.0;
  for (int b = 0; b < a.B; b++)
    if (a.act[(size_t)b * a.cap + fl]) c = c + *sk_plane(a, b, kSkShare + (kTrial ? 2 : 0), fl);
  n_act = 0;
  for (int j = 0; j < a.J; j++) {
    const int ch = a.fr.child_of[j], p = a.fr.parent[ch];
    if (a.act[(size_t)ch * a.cap + fl] && a.act[(size_t)p * a.cap + fl]) {
      c = c + *sk_plane(a, ch, kSkShare + (kTrial ? 3 : 1), fl);
      n_act++;
    }
  }
  return c;
}

// ------------------------------------------------------------------------------------------------------------------ solve
__global__ __launch_bounds__(kSolveLanes) void sk_solve_kernel(SkArgs a, int first) {
  const int64_t fl = (int64_t)blockIdx.x * kSolveLanes + threadIdx.x;
  if (fl >= a.nf) return;
  const int64_t f = a.f0 + fl;
  int n_act;
  const double cost = sk_frame_cost<false>(a, fl, n_act);
  if (first) {
    a.cost0[f] = cost;
    a.n_act[f] = n_act;
  }
  a.cost[f] = cost;

  bool piv = true;
  for (int n = 0; n < a.B; n++) {
    const int i = a.fr.order[n];
    if (!a.act[(size_t)i * a.cap + fl]) continue;
    const int p = a.fr.parent[i];
    const bool up = p >= 0 && a.act[(size_t)p * a.cap + fl] != 0;
    double H[21], g[6], L[15], dg[6], z[6];
#pragma unroll
    for (int e = 0; e < 21; e++) H[e] = *sk_plane(a, i, kSkH + e, fl);
#pragma unroll
    for (int e = 0; e < 6; e++) g[e] = *sk_plane(a, i, kSkG + e, fl);
    const bool ok = sk_ldl6(H, L, dg);
    piv = piv && ok;
    sk_solve6(L, dg, g, z);
#pragma unroll
    for (int e = 0; e < 6; e++) *sk_plane(a, i, kSkZ + e, fl) = z[e];
    if (!up) continue;
    SkUp c;
#pragma unroll
    for (int e = 0; e < 9; e++) c.G[e] = *sk_plane(a, i, kSkUp + e, fl);
#pragma unroll
    for (int e = 0; e < 3; e++) {
      c.u[e] = *sk_plane(a, i, kSkUp + 9 + e, fl);
      c.v[e] = *sk_plane(a, i, kSkUp + 12 + e, fl);
    }
    c.n = *sk_plane(a, i, kSkUp + 15, fl);
    double C[6][6];
    sk_up_block(c, C);
#pragma unroll
    for (int col = 0; col < 6; col++) {
      double bc[6], wc[6];
#pragma unroll
      for (int e = 0; e < 6; e++) bc[e] = C[e][col];
      sk_solve6(L, dg, bc, wc);
#pragma unroll
      for (int e = 0; e < 6; e++) *sk_plane(a, i, kSkW + 6 * e + col, fl) = wc[e];
#pragma unroll
      for (int r = col; r < 6; r++) {
        double s = C[0][r] * wc[0];
#pragma unroll
        for (int e = 1; e < 6; e++) s = s + C[e][r] * wc[e];
        double* hp = sk_plane(a, p, kSkH + sk_tri(r, col), fl);
        *hp = *hp - s;
      }
    }
#pragma unroll
    for (int r = 0; r < 6; r++) {
      double s = C[0][r] * z[0];
#pragma unroll
      for (int e = 1; e < 6; e++) s = s + C[e][r] * z[e];
      double* gp = sk_plane(a, p, kSkG + r, fl);
      *gp = *gp - s;
    }
  }
  a.piv[fl] = piv ? 1 : 0;

  for (int n = a.B - 1; n >= 0; n--) {
    const int i = a.fr.order[n];
    if (!a.act[(size_t)i * a.cap + fl]) continue;
    const int p = a.fr.parent[i];
    const bool up = p >= 0 && a.act[(size_t)p * a.cap + fl] != 0;
    double delta[6];
#pragma unroll
    for (int e = 0; e < 6; e++) delta[e] = *sk_plane(a, i, kSkZ + e, fl);
    if (up) {
      double dp[6];
#pragma unroll
      for (int e = 0; e < 6; e++) dp[e] = *sk_plane(a, p, kSkZ + e, fl);
#pragma unroll
      for (int e = 0; e < 6; e++) {
        double s = *sk_plane(a, i, kSkW + 6 * e, fl) * dp[0];
#pragma unroll
        for (int m = 1; m < 6; m++) s = s + *sk_plane(a, i, kSkW + 6 * e + m, fl) * dp[m];
        delta[e] = delta[e] + s;
      }
    }
#pragma unroll
    for (int e = 0; e < 6; e++) {
      delta[e] = -delta[e];
      *sk_plane(a, i, kSkZ + e, fl) = delta[e];
    }
    double q[4], t[3], qn[4], tn[3];
    sk_load_pose<false>(a, i, f, fl, q, t);
    sk_update(q, t, delta, qn, tn);
#pragma unroll
    for (int e = 0; e < 4; e++) *sk_plane(a, i, kSkTrial + e, fl) = qn[e];
#pragma unroll
    for (int e = 0; e < 3; e++) *sk_plane(a, i, kSkTrial + 4 + e, fl) = tn[e];
  }
}

// ------------------------------------------------------------------------------------------------------------------ accept
__global__ __launch_bounds__(kT) void sk_accept_kernel(SkArgs a) {
  const int64_t fl = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (fl >= a.nf) return;
  const int64_t f = a.f0 + fl;
  int n_act;
  const double trial = sk_frame_cost<true>(a, fl, n_act), cur = a.cost[f], lam = a.lam[fl];
  const bool take = a.piv[fl] != 0 && finite1(a.cost0[f]) && finite1(trial) && trial < cur;
  for (int b = 0; b < a.B; b++) {
    if (!a.act[(size_t)b * a.cap + fl]) continue;
    const size_t o = (size_t)b * a.n_frames + f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const double tr = *sk_plane(a, b, kSkTrial + i, fl), was = a.quat_s[4 * o + i];
      a.quat_s[4 * o + i] = take ? tr : was;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double tr = *sk_plane(a, b, kSkTrial + 4 + i, fl), was = a.t_s[3 * o + i];
      a.t_s[3 * o + i] = take ? tr : was;
    }
  }
  a.cost[f] = take ? trial : cur;
  a.lam[fl] = take ? lam / 10.0 : lam * 10.0;
  a.steps[f] = a.steps[f] + (take ? 1 : 0);
}

}  // namespace

hipError_t launch_put_sk_dirs(const SkDir* host, int n, SkDir* dev, hipStream_t stream) {
  for (int d0 = 0; d0 < n; d0 += kSkPutDirs) {
    SkDirChunk c{};
    const int count = n - d0 < kSkPutDirs ? n - d0 : kSkPutDirs;
    for (int i = 0; i < count; i++) c.d[i] = host[d0 + i];
    hipLaunchKernelGGL(sk_put_kernel, dim3(1), dim3(64), 0, stream, c, count, dev + d0);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

hipError_t launch_fit_skeleton_round(const SkArgs& a, int iters, hipStream_t stream) {
  const dim3 block(kT), grid((unsigned)ts_tiles(a.nf), (unsigned)a.B), per_frame((unsigned)ts_tiles(a.nf));
  const dim3 solve_block(kSolveLanes), solve_grid((unsigned)((a.nf + kSolveLanes - 1) / kSolveLanes));
  hipError_t e;
  hipLaunchKernelGGL(sk_init_kernel, grid, block, 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (int it = 0; it < iters; it++) {
    hipLaunchKernelGGL(sk_assemble_kernel, grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(sk_solve_kernel, solve_grid, solve_block, 0, stream, a, it == 0 ? 1 : 0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(sk_trial_kernel, grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(sk_accept_kernel, per_frame, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(sk_finish_kernel, grid, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_fit_skeleton_signs(const SkArgs& a, hipStream_t stream) {
  return launch_sign_walk<SkOnPosedOrJointed>(SignWalkArgs{a.n_frames, a.flag, a.quat_s, a.tile_i32, a.parity}, a.B, true, stream);
}

}  // namespace mocap
