// sign_walk.hpp -- the sign-continuous quaternions of a session's bodies (include/mocap_core.h, "body trajectories" item 1, "Sign
// continuity") as the stages that write quaternions per (body, frame) launch it: mocap_pose_rows over the POSED frames
// (body_session.hip), mocap_pose_joints over the POSED and JOINTED ones (joint_pose.hip).  Which frames carry a quaternion is the
// template parameter On: a struct with  __device__ static bool on(int32_t flag).  The previous frame that carries one is a prefix
// maximum (the tile's last such frame, one workgroup per body over the tiles, then within the tile), the flip against it, and the
// flips' prefix parity the same way: four small launches, no walk over frames (block_scan.hpp's prefix and tile scan).  Maximum
// and XOR are exact in any order.  Device code only.
#pragma once
#include "block_scan.hpp"

namespace mocap {

struct SignWalkArgs {
  int64_t n_frames;
  const int32_t* flag;  // [B][F]
  double* quat;         // [B][F][4]: as computed in, sign-continuous out
  int32_t* tile_i32;    // workspace [B][ts_tiles(F)]: the last carrying frame of a tile, then of the tiles before it; then the parities
  uint8_t* parity;      // workspace [B][F]: the flips' parity within the tile, up to and including the frame
};

// the last carrying frame of every tile (-1 = none), for a stage whose own kernel does not leave it behind
template <class On>
__global__ __launch_bounds__(kTsTile) void sw_last_kernel(SignWalkArgs a) {
  __shared__ int s_last;
  const int b = blockIdx.y, lane = threadIdx.x;
  const int64_t F = a.n_frames, f = (int64_t)blockIdx.x * kTsTile + lane;
  if (lane == 0) s_last = -1;
  __syncthreads();
  if (f < F && On::on(a.flag[(size_t)b * F + f])) atomicMax(&s_last, lane);  // (an integer maximum in LDS: exact in any order)
  __syncthreads();
  if (lane == 0) a.tile_i32[(size_t)b * gridDim.x + blockIdx.x] = s_last < 0 ? -1 : (int32_t)(blockIdx.x * kTsTile + s_last);
}

// the flip of every carrying frame against the carrying frame before it, and the flips' parity within the tile
template <class On>
__global__ __launch_bounds__(kTsTile) void sw_flip_kernel(SignWalkArgs a) {
  __shared__ int32_t s[kTsTile];
  const int b = blockIdx.y, lane = threadIdx.x;
  const int64_t F = a.n_frames, f = (int64_t)blockIdx.x * kTsTile + lane;
  const size_t o = (size_t)b * F + (f < F ? f : 0), tp = (size_t)b * gridDim.x + blockIdx.x;
  const bool posed = f < F && On::on(a.flag[o]);
  block_prefix<OpMaxI32>(posed ? (int32_t)f : -1, s);
  const int32_t in_tile = lane > 0 ? s[lane - 1] : -1, before_tile = a.tile_i32[tp];
  const int32_t prev = in_tile > before_tile ? in_tile : before_tile;
  int32_t flip = 0;
  if (posed) {
    const double* q = a.quat + 4 * o;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    if (prev < 0) {
      const double lead = w != 0.0 ? w : x != 0.0 ? x : y != 0.0 ? y : z;
      flip = lead < 0.0;
    } else {
      const double* u = a.quat + 4 * ((size_t)b * F + prev);
      const double d = ((u[0] * w + u[1] * x) + u[2] * y) + u[3] * z;
      flip = d < 0.0;
    }
  }
  __syncthreads();  // (s is read above and rewritten below)
  const int32_t par = block_prefix<OpXor>(flip, s);
  if (f < F) a.parity[o] = (uint8_t)par;
  __syncthreads();  // every lane has read tile_i32[tp]
  if (lane == kTsTile - 1) a.tile_i32[tp] = par;
}

template <class On>
__global__ __launch_bounds__(kTsTile) void sw_sign_kernel(SignWalkArgs a) {
  const int b = blockIdx.y;
  const int64_t F = a.n_frames, f = (int64_t)blockIdx.x * kTsTile + threadIdx.x;
  if (f >= F) return;
  const size_t o = (size_t)b * F + f;
  if (!On::on(a.flag[o])) return;
  if (!((a.parity[o] ^ a.tile_i32[(size_t)b * gridDim.x + blockIdx.x]) & 1)) return;
  double* q = a.quat + 4 * o;
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = -q[i];
}

// four launches behind the kernel that left every tile's last carrying frame in tile_i32; with `find_last`, five: that kernel first
template <class On>
inline hipError_t launch_sign_walk(const SignWalkArgs& a, int B, bool find_last, hipStream_t stream) {
  const int64_t P = ts_tiles(a.n_frames);
  const dim3 block(kTsTile), grid((unsigned)P, (unsigned)B), per_body((unsigned)B);
  hipError_t e;
  if (find_last) {
    hipLaunchKernelGGL(sw_last_kernel<On>, grid, block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(tile_scan_kernel<OpMaxI32>, per_body, block, 0, stream, a.tile_i32, P);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(sw_flip_kernel<On>, grid, block, 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(tile_scan_kernel<OpXor>, per_body, block, 0, stream, a.tile_i32, P);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(sw_sign_kernel<On>, grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace mocap
