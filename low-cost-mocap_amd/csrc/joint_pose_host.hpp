// joint_pose_host.hpp -- the host's part of "joint poses" (include/mocap_core.h): the argument rules of mocap_pose_joints, the forest
// check of its joints, and the table of directed joints with each one's 256-bit mask.  Plain C++ with no HIP in it, so that a
// stand-alone program can include it and run under the host sanitizers (tests/native/joint_pose_host_check.cpp);
// joint_pose_capi.hip calls these and nothing else decides a refusal of the joints or the three parameters (the bodies and the
// session are refused by "body trajectories"' own checks).  Each function returns nullptr when the arguments stand, else the
// sentence for mocap_last_error.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "joints_host.hpp"
#include "span_rule.hpp"

namespace mocap {

constexpr int kJpMaxBodies = 64;   // mirrored from include/mocap_core.h (MOCAP_BP_MAX_BODIES)
constexpr int kJpMaxMarkers = 8;   // (MOCAP_RB_MAX_MARKERS)
constexpr int kJpMaxRounds = 16;   // (MOCAP_JP_MAX_ROUNDS)
constexpr int kBpJointed = 16;     // (MOCAP_BP_JOINTED)

// One joint as one of its two bodies sees it: y is the body that may be posed through it, x the body on the other side.
struct JpDir {               // 144 bytes
  int32_t j, x, kind, pad;   // the joint's index in the call, the other body, MOCAP_JT_HINGE or MOCAP_JT_BALL
  double v0[3], v1[3];       // the virtual points in y's coordinates: c_y, and under HINGE c_y + axis_len * axis_y (else 0)
  double c_x[3], ax_x[3];    // the centre and (HINGE; else 0) the axis in x's coordinates
  unsigned long long mask[4];  // bit s: the markers s of y (bit m = marker m) with the virtual points hold a spanning triple
};

inline const char* jp_args_check(int B, int J, double axis_len, double max_rms, int max_rounds) {
  if (B < 2 || B > kJpMaxBodies) return "B must be 2 .. 64";
  if (J < 1 || J > B - 1) return "J must be 1 .. B-1";
  if (!(axis_len > 0.0) || !std::isfinite(axis_len)) return "axis_len must be finite and > 0";
  if (!(max_rms > 0.0)) return "max_rms must be > 0 (+inf = any)";
  if (max_rounds < 1 || max_rounds > kJpMaxRounds) return "max_rounds must be 1 .. 16";
  return nullptr;
}

// the joints of a call, every array with J entries ([J][3] for the centres and axes): ranges, kinds, values, and that they form a
// forest (a union-find over the bodies: a joint whose two bodies are already connected closes a cycle or repeats a pair)
inline const char* jp_joints_check(int B, int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind, const double* c_a,
                                   const double* c_b, const double* axis_a, const double* axis_b) {
  if (!body_a || !body_b || !kind || !c_a || !c_b || !axis_a || !axis_b) return "null buffer";
  int top[kJpMaxBodies];
  for (int b = 0; b < B; b++) top[b] = b;
  for (int j = 0; j < J; j++) {
    const int a = body_a[j], b = body_b[j];
    if (a < 0 || a >= B || b < 0 || b >= B) return "a joint's body lies outside 0 .. B-1";
    if (a == b) return "a joint joins two different bodies";
    if (kind[j] != kJtHinge && kind[j] != kJtBall) return "a joint's kind is neither MOCAP_JT_HINGE nor MOCAP_JT_BALL";
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(c_a[3 * (size_t)j + k]) || !std::isfinite(c_b[3 * (size_t)j + k])) return "a joint's centre is not finite";
    if (kind[j] == kJtHinge)
      for (const double* ax : {axis_a + 3 * (size_t)j, axis_b + 3 * (size_t)j}) {
        if (!std::isfinite(ax[0]) || !std::isfinite(ax[1]) || !std::isfinite(ax[2])) return "a hinge's axis is not finite";
        const double n2 = (ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2];
        if (!(std::fabs(n2 - 1.0) <= 1e-6)) return "a hinge's axis is not a unit vector (|a|^2 within 1e-6 of 1)";
      }
    int ra = a, rb = b;
    while (top[ra] != ra) ra = top[ra];
    while (top[rb] != rb) rb = top[rb];
    if (ra == rb) return "the joints are no forest (a pair appears twice, or a cycle)";
    top[ra > rb ? ra : rb] = ra > rb ? rb : ra;
  }
  return nullptr;
}

// bit s of the mask: the n markers' subset s, together with the nv virtual points, holds a spanning triple (posable_mask's rule
// over the augmented set; n in 3 .. 8, nv in 1 .. 2)
inline void jp_dir_mask(int n, const double (*q)[3], int nv, const double (*v)[3], unsigned long long mask[4]) {
  mask[0] = mask[1] = mask[2] = mask[3] = 0;
  constexpr int kP = kJpMaxMarkers + 2;
  const int np = n + nv;
  const double* p[kP];
  for (int i = 0; i < n; i++) p[i] = q[i];
  for (int i = 0; i < nv; i++) p[n + i] = v[i];
  unsigned char triple[kP][kP][kP];
  for (int i = 0; i < np; i++)
    for (int j = i + 1; j < np; j++)
      for (int k = j + 1; k < np; k++) triple[i][j][k] = triple_spans(p[i], p[j], p[k]) ? 1 : 0;
  const unsigned virt = ((1u << nv) - 1) << n;
  for (unsigned s = 0; s < (1u << n); s++) {
    const unsigned all = s | virt;
    bool ok = false;
    for (int i = 0; i < np && !ok; i++)
      for (int j = i + 1; j < np && !ok; j++)
        for (int k = j + 1; k < np && !ok; k++) ok = (all >> i & 1) && (all >> j & 1) && (all >> k & 1) && triple[i][j][k];
    if (ok) mask[s >> 6] |= 1ull << (s & 63);
  }
}

// The directed joints of a call, ordered by (y, joint index): table[first[y] .. first[y + 1]) are the joints of body y in
// ascending joint index.  n_markers [B] and markers [B][8][3] are the bodies as "body trajectories" has checked them; the joints
// are checked here (jp_joints_check).  first has B + 1 entries.
inline const char* jp_dir_table(int B, const int32_t* n_markers, const double* markers, int J, const int32_t* body_a,
                                const int32_t* body_b, const int32_t* kind, const double* c_a, const double* c_b, const double* axis_a,
                                const double* axis_b, double axis_len, std::vector<JpDir>& table, int32_t* first) {
  if (const char* why = jp_joints_check(B, J, body_a, body_b, kind, c_a, c_b, axis_a, axis_b)) return why;
  table.clear();
  table.reserve(2 * (size_t)J);
  for (int y = 0; y < B; y++) {
    first[y] = (int32_t)table.size();
    const double(*q)[3] = reinterpret_cast<const double(*)[3]>(markers + (size_t)y * kJpMaxMarkers * 3);
    for (int j = 0; j < J; j++) {
      if (body_a[j] != y && body_b[j] != y) continue;
      const bool is_a = body_a[j] == y;
      const double *c_y = (is_a ? c_a : c_b) + 3 * (size_t)j, *cx = (is_a ? c_b : c_a) + 3 * (size_t)j;
      const double *ax_y = (is_a ? axis_a : axis_b) + 3 * (size_t)j, *axx = (is_a ? axis_b : axis_a) + 3 * (size_t)j;
      JpDir d{};
      d.j = j;
      d.x = is_a ? body_b[j] : body_a[j];
      d.kind = kind[j];
      const bool hinge = d.kind == kJtHinge;
      for (int k = 0; k < 3; k++) {
        d.v0[k] = c_y[k];
        d.v1[k] = hinge ? c_y[k] + axis_len * ax_y[k] : 0.0;
        d.c_x[k] = cx[k];
        d.ax_x[k] = hinge ? axx[k] : 0.0;
      }
      const double v[2][3] = {{d.v0[0], d.v0[1], d.v0[2]}, {d.v1[0], d.v1[1], d.v1[2]}};
      jp_dir_mask(n_markers[y], q, hinge ? 2 : 1, v, d.mask);
      table.push_back(d);
    }
  }
  first[B] = (int32_t)table.size();
  return nullptr;
}

}  // namespace mocap
