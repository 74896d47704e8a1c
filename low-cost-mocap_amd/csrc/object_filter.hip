// object_filter.hip -- `filtered_objects` of the reference's live loop (computer_code/api/helpers.py:109):
// KalmanFilter.predict_location (KalmanFilter.py:50-100) with its three LowPassFilter.filter calls per drone
// (LowPassFilter.py:15-25), restated for a run of frames whose time stamps are an argument.
//
// Two kernels.  The Kalman recurrence is sequential in the frames and independent between drone indices: one workgroup,
// one wave per drone index, walks the frames (object_filter_scan_kernel).  The low-pass is not a recurrence at all: the
// reference runs lfilter from a ZERO state over its whole buffer on every call and keeps the last sample, i.e. the dot
// product of the buffer with the truncated impulse response h -- one wave per (frame, drone, channel), all independent
// (object_filter_lowpass_kernel).  The scan kernel only has to say which samples a frame's window spans.
//
// Arithmetic of the Kalman step: cv::KalmanFilter(9, 6, CV_32F) stores every member and temporary as float32; each
// matrix product below is accumulated in double (products of two float32 are exact there) and rounded to float32 once per
// stored entry, the 6 x 6 system S X = H P- is solved by a Cholesky factorisation in double and X rounded to float32.  F has
// three non-zero entries per row (1, dt, dt^2/2) and H is the first six rows of the identity: the zero terms of the dense
// products add nothing and are not formed.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace mocap {

namespace {

constexpr int kD = kObjFilterMaxObjects;

struct FrameIn {  // a frame's inputs as lane o (< O_max) of every wave holds them
  double t, px, py, pz, hd;
  int n, dr;
};

__device__ __forceinline__ FrameIn load_frame(const ObjFilterArgs& a, int64_t f, int lane) {
  FrameIn r;
  r.t = a.t[f];
  const int n = a.n_obj[f];
  r.n = n < 0 ? 0 : (n > a.O_max ? a.O_max : n);  // the locator counts the objects it had no slot for: they do not exist here
  r.dr = -1;
  r.px = r.py = r.pz = r.hd = 0.0;
  if (lane < a.O_max) {  // (every slot of the buffer is readable; slots >= n are masked by the consumer)
    const size_t i = (size_t)f * a.O_max + lane;
    r.dr = a.drone[i];
    r.px = a.pos[i * 3 + 0];
    r.py = a.pos[i * 3 + 1];
    r.pz = a.pos[i * 3 + 2];
    r.hd = a.heading[i];
  }
  return r;
}

}  // namespace

__global__ __launch_bounds__(64 * kD) void object_filter_scan_kernel(ObjFilterArgs a) {
  __shared__ float sP[kD][2][81];  // errorCovPost / errorCovPre (ping-pong: the correction reads one and writes the other)
  __shared__ float sT[kD][81];     // temp1 = F P
  __shared__ float sK[kD][54];     // gain [9][6]
  const int d = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e0 = lane, e1 = lane + 64;  // the (up to) two entries of a 9 x 9 matrix this lane owns
  const bool has1 = e1 < 81;
  const int i0 = e0 / 9, j0 = e0 % 9, i1 = has1 ? e1 / 9 : 0, j1 = has1 ? e1 % 9 : 0;
  ObjFilterDrone* st = &a.state->drone[d];
  int cur = 0;
  sP[d][0][e0] = st->P[e0];
  if (has1) sP[d][0][e1] = st->P[e1];
  float x[9];  // statePost, the same in every lane
#pragma unroll
  for (int k = 0; k < 9; k++) x[k] = st->x[k];
  float pp[3] = {st->prev_pos[0], st->prev_pos[1], st->prev_pos[2]};
  int len = st->buf_len, n_s = 0;
  double t_prev = a.state->prev_time;
  double* samp = a.samp + (size_t)d * 4 * a.n_frames;
  __syncthreads();

  FrameIn nxt = load_frame(a, 0, lane);
  for (int64_t f = 0; f < a.n_frames; f++) {
    const FrameIn in = nxt;
    if (f + 1 < a.n_frames) nxt = load_frame(a, f + 1, lane);  // (inputs do not depend on the state: one frame ahead)
    const double dt = in.t - t_prev;  // KalmanFilter.py:53-54: on every call, candidates or not
    t_prev = in.t;
    const bool mine = lane < in.n && in.dr == d;
    const unsigned long long m = __ballot(mine);
    const size_t fd = (size_t)f * a.D + d;
    if (m == 0 && lane == 0) {  // KalmanFilter.py:60-61: no candidate, the drone is skipped, its state untouched
      a.chosen[fd] = -1;
      a.slot[fd * 2] = -1;
      a.slot[fd * 2 + 1] = 0;
    }
    if (m == 0 && lane < 3) a.fpos[fd * 3 + lane] = __builtin_nanf("");
    // every wave sees the same object list: the test is uniform over the workgroup, and so are the barriers behind it
    if (__ballot(lane < in.n && in.dr >= 0 && in.dr < a.D) == 0) continue;
    const bool act = m != 0;
    const int c0 = act ? __ffsll(m) - 1 : 0;

    // ---- transition matrix entries (KalmanFilter.py:65-67: float32 members, dt^2/2 computed in double)
    const float dtf = (float)dt, hf = (float)(0.5 * (dt * dt));
    // ---- KalmanFilter.py:69-73: an all-zero statePost is "not initialised" and takes candidate 0's position
    const float c0x = (float)__shfl(in.px, c0), c0y = (float)__shfl(in.py, c0), c0z = (float)__shfl(in.pz, c0);
    bool allz = true;
#pragma unroll
    for (int k = 0; k < 9; k++) allz = allz && x[k] == 0.0f;
    if (act && allz) {
      x[0] = c0x;
      x[1] = c0y;
      x[2] = c0z;
    }
    // ---- predict: statePre = F statePost
    float xp[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
      double acc = (double)x[i];
      if (i < 6) acc += (double)dtf * (double)x[i + 3];
      if (i < 3) acc += (double)hf * (double)x[i + 6];
      xp[i] = (float)acc;
    }
    // temp1 = F errorCovPost
    if (act) {
      const float* P = sP[d][cur];
      auto t1 = [&](int i, int j) {
        double acc = (double)P[i * 9 + j];
        if (i < 6) acc += (double)dtf * (double)P[(i + 3) * 9 + j];
        if (i < 3) acc += (double)hf * (double)P[(i + 6) * 9 + j];
        return (float)acc;
      };
      sT[d][e0] = t1(i0, j0);
      if (has1) sT[d][e1] = t1(i1, j1);
    }
    __syncthreads();
    // errorCovPre = temp1 F^T + Q   (copied to errorCovPost by predict())
    if (act) {
      const float* T = sT[d];
      auto pre = [&](int i, int j) {
        double acc = (double)T[i * 9 + j];
        if (j < 6) acc += (double)T[i * 9 + j + 3] * (double)dtf;
        if (j < 3) acc += (double)T[i * 9 + j + 6] * (double)hf;
        if (i == j) acc += (double)a.q;
        return (float)acc;
      };
      sP[d][cur][e0] = pre(i0, j0);
      if (has1) sP[d][cur][e1] = pre(i1, j1);
    }
    __syncthreads();
    float y[6];
    int sel = c0;
    if (act) {
      // ---- association (KalmanFilter.py:76-77): float64 distance to the predicted position, first minimum
      const double ex = in.px - (double)xp[0], ey = in.py - (double)xp[1], ez = in.pz - (double)xp[2];
      double dist = mine ? sqrt((ex * ex + ey * ey) + ez * ez) : __builtin_inf();
      int idx = lane;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const double od = __shfl_xor(dist, off);
        const int oi = __shfl_xor(idx, off);
        if (od < dist || (od == dist && oi < idx)) {
          dist = od;
          idx = oi;
        }
      }
      sel = __shfl(idx, 0);
      if (!((m >> sel) & 1ull)) sel = c0;  // (only a NaN position gets here)
      // ---- measurement (KalmanFilter.py:78-80)
      const float np_[3] = {(float)__shfl(in.px, sel), (float)__shfl(in.py, sel), (float)__shfl(in.pz, sel)};
      float z[6];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        z[k] = np_[k];
        z[k + 3] = (np_[k] - pp[k]) / dtf;
        pp[k] = np_[k];
      }
#pragma unroll
      for (int k = 0; k < 6; k++) y[k] = z[k] - xp[k];  // temp5 = z - H statePre
      // ---- correct(): S = H P- H^T + R, factorised by every lane; lane j solves column j of S X = H P-
      const float* P = sP[d][cur];
      double L[6][6];
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
          double s = (double)(i == j ? P[i * 9 + j] + a.r : P[i * 9 + j]);
#pragma unroll
          for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
          L[i][j] = i == j ? sqrt(s) : s / L[j][j];
        }
      const int jj = lane < 9 ? lane : 8;
      double w[6];
#pragma unroll
      for (int i = 0; i < 6; i++) {
        double s = (double)P[i * 9 + jj];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[i][k] * w[k];
        w[i] = s / L[i][i];
      }
      float g[6];  // row jj of the gain = column jj of X
#pragma unroll
      for (int i = 5; i >= 0; i--) {
        double s = w[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s -= L[k][i] * w[k];
        w[i] = s / L[i][i];
        g[i] = (float)w[i];
      }
      // statePost = statePre + gain temp5
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) acc += (double)g[k] * (double)y[k];
      const float xn = (float)(acc + (double)xp[jj]);
#pragma unroll
      for (int k = 0; k < 9; k++) x[k] = __shfl(xn, k);
      if (lane < 9) {
#pragma unroll
        for (int k = 0; k < 6; k++) sK[d][lane * 6 + k] = g[k];
      }
      // ---- what the frame hands on: KalmanFilter.py:83-91 reads the PREDICTED state
      const double hd_sel = __shfl(in.hd, sel);
      const int L_win = len + 1;            // LowPassFilter.py:16: append, then filter the whole buffer
      len = L_win >= a.B ? a.keep : L_win;  // LowPassFilter.py:20-21
      if (lane == 0) {
        a.chosen[fd] = sel;
        a.slot[fd * 2] = n_s;
        a.slot[fd * 2 + 1] = L_win;
        a.fpos[fd * 3 + 0] = xp[0];
        a.fpos[fd * 3 + 1] = xp[1];
        a.fpos[fd * 3 + 2] = xp[2];
        samp[0 * a.n_frames + n_s] = hd_sel;
        samp[1 * a.n_frames + n_s] = (double)xp[3];
        samp[2 * a.n_frames + n_s] = (double)xp[4];
        samp[3 * a.n_frames + n_s] = (double)xp[5];
      }
      n_s++;
    }
    __syncthreads();
    // errorCovPost = errorCovPre - gain (H errorCovPre)
    if (act) {
      const float* P = sP[d][cur];
      const float* K = sK[d];
      auto post = [&](int i, int j) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) acc += (double)K[i * 6 + k] * (double)P[k * 9 + j];
        return (float)((double)P[i * 9 + j] - acc);
      };
      sP[d][cur ^ 1][e0] = post(i0, j0);
      if (has1) sP[d][cur ^ 1][e1] = post(i1, j1);
      cur ^= 1;
    }
    __syncthreads();
  }

  st->P[e0] = sP[d][cur][e0];
  if (has1) st->P[e1] = sP[d][cur][e1];
#pragma unroll
  for (int k = 0; k < 9; k++)
    if (lane == k) st->x[k] = x[k];
#pragma unroll
  for (int k = 0; k < 3; k++)
    if (lane == k) st->prev_pos[k] = pp[k];
  if (lane == 0) {
    st->buf_len = len;
    a.n_samp[d] = n_s;
  }
  __syncthreads();  // (every wave has read prev_time)
  if (threadIdx.x == 0) a.state->prev_time = t_prev;
}

// One 256-lane workgroup per (frame, drone): wave c filters channel c (heading, vx, vy, vz).  The window of the frame's
// sample j is samples j-L+1 .. j of the drone's sequence, which runs from the stored history (the last B samples before
// this call) into this call's samples.  The lane partition and the reduction tree depend on L alone: the result does not
// depend on how a session was cut into calls.  Workgroups beyond F*D hand the history on to the next call.
__global__ __launch_bounds__(256) void object_filter_lowpass_kernel(ObjFilterArgs a) {
  const int64_t FD = a.n_frames * a.D;
  const int64_t blk = blockIdx.x;
  const int F = (int)a.n_frames, B = a.B;
  if (blk >= FD) {
    const int d = (int)(blk - FD);
    const int n = a.n_samp[d];
    for (int idx = threadIdx.x; idx < 4 * B; idx += 256) {
      const int c = idx / B, i = idx % B;
      const int s = n - B + i;
      const size_t ch = (size_t)d * 4 + c;
      a.hist_out[ch * B + i] = s >= 0 ? a.samp[ch * F + s] : a.hist_in[ch * B + (B + s)];
    }
    return;
  }
  const int d = (int)(blk % a.D), c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = a.slot[blk * 2], L = a.slot[blk * 2 + 1];
  double acc = 0.0;
  if (j >= 0) {
    const size_t ch = (size_t)d * 4 + c;
    const double* cs = a.samp + ch * F;
    const double* hs = a.hist_in + ch * B + B;  // hs[-1] = the sample before this call's first
    for (int k = lane; k < L; k += 64) {
      const int i = j - k;
      acc += a.h[k] * (i >= 0 ? cs[i] : hs[i]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
  } else {
    acc = __builtin_nan("");
  }
  if (lane == 0) {
    if (c == 0) a.fheading[blk] = acc;                 // KalmanFilter.py:86: kept as float64
    else a.fvel[blk * 3 + (c - 1)] = (float)acc;       // KalmanFilter.py:90-91: assigned into the float32 state slice
  }
}

__global__ __launch_bounds__(64) void object_filter_reset_kernel(ObjFilterState* s, int D, double now) {
  // KalmanFilter.py:103-108: the clock is set back 20 s, statePost and prev_position are zeroed; covariances and low-pass buffers stay
  const int lane = threadIdx.x;
  for (int d = 0; d < D; d++) {
    if (lane < 9) s->drone[d].x[lane] = 0.0f;
    if (lane < 3) s->drone[d].prev_pos[lane] = 0.0f;
  }
  if (lane == 0) s->prev_time = now - 20.0;
}

hipError_t launch_object_filter(const ObjFilterArgs& a, hipStream_t stream) {
  if (a.n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(object_filter_scan_kernel, dim3(1), dim3(64 * a.D), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t blocks = a.n_frames * a.D + a.D;
  hipLaunchKernelGGL(object_filter_lowpass_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_object_filter_reset(ObjFilterState* state, int D, double now, hipStream_t stream) {
  hipLaunchKernelGGL(object_filter_reset_kernel, dim3(1), dim3(64), 0, stream, state, D, now);
  return hipGetLastError();
}

}  // namespace mocap
