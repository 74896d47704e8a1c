// joints_host.hpp -- the host's part of "joints" (include/mocap_core.h): the argument rules of mocap_find_joints and the joint table
// of mocap_joint_series, checked and tabulated.  Plain C++ with no HIP in it, so that a stand-alone program can include it and run
// under the host sanitizers (tests/native/joints_host_check.cpp); joints_capi.hip calls these and nothing else decides a refusal.
// Each function returns nullptr when the arguments stand, else the sentence for mocap_last_error.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace mocap {

constexpr int kJtMaxBodies = 64;           // mirrored from include/mocap_core.h (MOCAP_BP_MAX_BODIES)
constexpr int64_t kJtMaxFrames = 1 << 22;  // mirrored from include/mocap_core.h (MOCAP_RG_MAX_FRAMES)
constexpr int kJtMaxJoints = 64;           // mirrored from include/mocap_core.h (MOCAP_JT_MAX_JOINTS)
constexpr int kJtUnseen = 0, kJtSingular = 1, kJtFixed = 2, kJtHinge = 3, kJtBall = 4;  // MOCAP_JT_*

struct JtJoint {        // one joint of a mocap_joint_series call, as the host tabulates it (128 bytes)
  int32_t a, b, kind, pad;
  double c_a[3], c_b[3], axis_b[3], q_ref[4];
  double pad2;
};

inline const char* jt_find_check(int64_t n_frames, int B, int min_common, double tol_rank, double max_sep) {
  if (n_frames < 1 || n_frames > kJtMaxFrames) return "n_frames must be 1 .. 4194304";
  if (B < 2 || B > kJtMaxBodies) return "B must be 2 .. 64";
  if (min_common < 6) return "min_common must be at least 6";
  if (!(tol_rank > 0.0 && tol_rank < 1.0)) return "tol_rank must lie in (0, 1)";
  if (!(max_sep > 0.0)) return "max_sep must be > 0 (+inf = any)";
  return nullptr;
}

inline const char* jt_series_check(int64_t n_frames, int B) {
  if (n_frames < 1 || n_frames > kJtMaxFrames) return "n_frames must be 1 .. 4194304";
  if (B < 2 || B > kJtMaxBodies) return "B must be 2 .. 64";
  return nullptr;
}

// the joints of a call: every array has J entries (c_a, c_b, axis_b [J][3], q_ref [J][4]); axis_b is read under HINGE alone
inline const char* jt_joint_table(int B, int J, const int32_t* body_a, const int32_t* body_b, const int32_t* kind, const double* c_a,
                                  const double* c_b, const double* axis_b, const double* q_ref, std::vector<JtJoint>& table) {
  if (J < 1 || J > kJtMaxJoints) return "J must be 1 .. 64";
  if (!body_a || !body_b || !kind || !c_a || !c_b || !axis_b || !q_ref) return "null buffer";
  table.assign((size_t)J, JtJoint{});
  for (int j = 0; j < J; j++) {
    JtJoint& t = table[(size_t)j];
    t.a = body_a[j];
    t.b = body_b[j];
    t.kind = kind[j];
    if (t.a < 0 || t.a >= B || t.b < 0 || t.b >= B) return "a joint's body lies outside 0 .. B-1";
    if (t.a == t.b) return "a joint joins two different bodies";
    if (t.kind < kJtUnseen || t.kind > kJtBall) return "a joint's kind is no MOCAP_JT_* value";
    double n2 = 0.0;
    for (int k = 0; k < 3; k++) {
      t.c_a[k] = c_a[3 * (size_t)j + k];
      t.c_b[k] = c_b[3 * (size_t)j + k];
      t.axis_b[k] = t.kind == kJtHinge ? axis_b[3 * (size_t)j + k] : 0.0;
      if (!std::isfinite(t.c_a[k]) || !std::isfinite(t.c_b[k])) return "a joint's centre is not finite";
      if (!std::isfinite(t.axis_b[k])) return "a hinge's axis is not finite";
    }
    for (int k = 0; k < 4; k++) {
      t.q_ref[k] = q_ref[4 * (size_t)j + k];
      if (!std::isfinite(t.q_ref[k])) return "a joint's q_ref is not finite";
      n2 += t.q_ref[k] * t.q_ref[k];
    }
    if (!(std::fabs(n2 - 1.0) <= 1e-6)) return "a joint's q_ref is not a unit quaternion (|q|^2 within 1e-6 of 1)";
  }
  return nullptr;
}

}  // namespace mocap
