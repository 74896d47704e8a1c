// span_rule.hpp -- the rigid-body section's rule for three points that span a plane (include/mocap_core.h, "rigid bodies"), for the
// host tables that are built from it: a body's posable mask (body_session_capi.hip) and a directed joint's (joint_pose_host.hpp).
// Plain C++ with no HIP in it.
#pragma once
#include <cmath>

namespace mocap {

// |(q_j - q_i) x (q_k - q_i)| >= 0.1 |q_j - q_i| |q_k - q_i|, in the section's order
inline bool triple_spans(const double* qi, const double* qj, const double* qk) {
  const double u[3] = {qj[0] - qi[0], qj[1] - qi[1], qj[2] - qi[2]}, v[3] = {qk[0] - qi[0], qk[1] - qi[1], qk[2] - qi[2]};
  const double c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const double nc = std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  const double nu = std::sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]), nv = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  return nc >= (0.1 * nu) * nv;
}

}  // namespace mocap
