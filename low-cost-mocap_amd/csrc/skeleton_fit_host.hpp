// skeleton_fit_host.hpp -- the host's part of "skeleton fit" (include/mocap_core.h): the argument rules of mocap_fit_skeleton and
// the tables the kernels walk -- every body's directed joints, and the forest as an elimination order (parents, depths, leaves
// first).  The joints themselves are refused by "joint poses"' own check (joint_pose_host.hpp, jp_joints_check): one function, two
// callers.  Plain C++ with no HIP in it, so that a stand-alone program can include it and run under the host sanitizers
// (tests/native/skeleton_fit_host_check.cpp).  Each function returns nullptr when the arguments stand, else the sentence for
// mocap_last_error.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "joint_pose_host.hpp"

namespace mocap {

constexpr int kSkMaxBodies = kJpMaxBodies;  // mirrored from include/mocap_core.h (MOCAP_BP_MAX_BODIES)
constexpr int kSkMaxIters = 16;             // (MOCAP_SK_MAX_ITERS)

// One joint as one of its two bodies sees it: y is the body whose block the terms go into, x the body on the other side.
struct SkDir {               // 112 bytes
  int32_t j, x, kind, up;    // the joint's index in the call, the other body, MOCAP_JT_HINGE or MOCAP_JT_BALL, 1 = x is y's parent
  double c_y[3], ax_y[3];    // the centre and (HINGE; else 0) the axis in y's coordinates
  double c_x[3], ax_x[3];    // the same in x's coordinates
};

struct SkForest {
  int32_t first[kSkMaxBodies + 1];  // dirs[first[y] .. first[y + 1]) are the joints of body y in ascending joint index
  int32_t parent[kSkMaxBodies];     // -1 = the root of its component (the component's lowest body)
  int32_t depth[kSkMaxBodies];      // joints between the body and its root
  int32_t joint_up[kSkMaxBodies];   // the joint to the parent, -1 for a root
  int32_t order[kSkMaxBodies];      // the elimination order: by (depth descending, index ascending)
  int32_t child_of[kSkMaxBodies];   // [J]: the body whose joint_up the joint is
};

inline const char* sk_args_check(int B, int J, double axis_len, double w_joint, int iters) {
  if (B < 2 || B > kSkMaxBodies) return "B must be 2 .. 64";
  if (J < 1 || J > B - 1) return "J must be 1 .. B-1";
  if (!(axis_len > 0.0) || !std::isfinite(axis_len)) return "axis_len must be finite and > 0";
  if (!(w_joint > 0.0) || !std::isfinite(w_joint)) return "w_joint must be finite and > 0";
  if (iters < 1 || iters > kSkMaxIters) return "iters must be 1 .. 16";
  return nullptr;
}

// The joints of a call (every array with J entries, [J][3] for the centres and axes; B and J as sk_args_check passed them) checked
// by jp_joints_check, then tabulated.  dirs gets 2 J entries ordered by (y, joint index).
inline const char* sk_tables(int B, int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind, const double* c_a,
                             const double* c_b, const double* axis_a, const double* axis_b, std::vector<SkDir>& dirs, SkForest& fr) {
  if (const char* why = jp_joints_check(B, J, body_a, body_b, kind, c_a, c_b, axis_a, axis_b)) return why;
  // the forest from its roots: a component's lowest body is reached first, the others through the body that found them
  for (int b = 0; b < kSkMaxBodies; b++) fr.parent[b] = fr.joint_up[b] = fr.child_of[b] = -1, fr.depth[b] = 0, fr.order[b] = 0;
  bool seen[kSkMaxBodies] = {};
  int queue[kSkMaxBodies];
  for (int root = 0; root < B; root++) {
    if (seen[root]) continue;
    int head = 0, tail = 0;
    queue[tail++] = root;
    seen[root] = true;
    while (head < tail) {
      const int p = queue[head++];
      for (int j = 0; j < J; j++) {
        const int c = body_a[j] == p ? body_b[j] : body_b[j] == p ? body_a[j] : -1;
        if (c < 0 || seen[c]) continue;
        seen[c] = true;
        fr.parent[c] = p;
        fr.depth[c] = fr.depth[p] + 1;
        fr.joint_up[c] = j;
        fr.child_of[j] = c;
        queue[tail++] = c;
      }
    }
  }
  int n = 0;
  for (int d = B - 1; d >= 0; d--)
    for (int b = 0; b < B; b++)
      if (fr.depth[b] == d) fr.order[n++] = b;
  dirs.clear();
  dirs.reserve(2 * (size_t)J);
  for (int y = 0; y < B; y++) {
    fr.first[y] = (int32_t)dirs.size();
    for (int j = 0; j < J; j++) {
      if (body_a[j] != y && body_b[j] != y) continue;
      const bool is_a = body_a[j] == y;
      const double *cy = (is_a ? c_a : c_b) + 3 * (size_t)j, *cx = (is_a ? c_b : c_a) + 3 * (size_t)j;
      const double *ay = (is_a ? axis_a : axis_b) + 3 * (size_t)j, *ax = (is_a ? axis_b : axis_a) + 3 * (size_t)j;
      SkDir d{};
      d.j = j;
      d.x = is_a ? body_b[j] : body_a[j];
      d.kind = kind[j];
      d.up = fr.joint_up[y] == j ? 1 : 0;
      const bool hinge = d.kind == kJtHinge;
      for (int k = 0; k < 3; k++) {
        d.c_y[k] = cy[k];
        d.c_x[k] = cx[k];
        d.ax_y[k] = hinge ? ay[k] : 0.0;
        d.ax_x[k] = hinge ? ax[k] : 0.0;
      }
      dirs.push_back(d);
    }
  }
  for (int y = B; y <= kSkMaxBodies; y++) fr.first[y] = (int32_t)dirs.size();
  return nullptr;
}

}  // namespace mocap
