// joint_pose_host_check.cpp -- the host's part of "joint poses" (csrc/joint_pose_host.hpp: the argument rules of mocap_pose_joints,
// the forest check and the table of directed joints with their masks) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_joint_pose_native_cpu.py and run as a process of its own.  Every array handed to the
// code under test is a heap block of exactly the size the contract names, so a read past it is seen.
//   joint_pose_host_check args    stdin: B J axis_len max_rms max_rounds per line                 stdout: 1 (stands) or 0 (refused)
//   joint_pose_host_check table   stdin: B axis_len J, then per body n and 24 coordinates, then per joint a b kind c_a[3] c_b[3]
//                                 axis_a[3] axis_b[3], all on one line
//                                 stdout: 0, or 1, first[0 .. B], and per directed joint j x kind v0 v1 c_x ax_x mask[4]
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../low-cost-mocap_amd/csrc/joint_pose_host.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const bool args = !std::strcmp(argv[1], "args");
  if (!args && std::strcmp(argv[1], "table")) return 2;
  std::string line;
  long lines = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    auto number = [&in]() {
      std::string s;
      in >> s;
      return std::strtod(s.c_str(), nullptr);  // (reads nan and inf)
    };
    if (args) {
      const int B = (int)number(), J = (int)number();
      const double axis_len = number(), max_rms = number();
      const int max_rounds = (int)number();
      std::printf("%d\n", mocap::jp_args_check(B, J, axis_len, max_rms, max_rounds) ? 0 : 1);
    } else {
      const int B = (int)number();
      const double axis_len = number();
      const int J = (int)number();
      if (B < 1 || B > mocap::kJpMaxBodies || J < 0) return 3;
      const size_t nb = (size_t)B, n = (size_t)J;
      std::vector<int32_t> n_markers(nb), a(n), b(n), kind(n), first(nb + 1);
      std::vector<double> markers(nb * 24), c_a(3 * n), c_b(3 * n), axis_a(3 * n), axis_b(3 * n);
      for (size_t i = 0; i < nb; i++) {
        n_markers[i] = (int32_t)number();
        for (int k = 0; k < 24; k++) markers[24 * i + k] = number();
      }
      for (size_t j = 0; j < n; j++) {
        a[j] = (int32_t)number();
        b[j] = (int32_t)number();
        kind[j] = (int32_t)number();
        for (int k = 0; k < 3; k++) c_a[3 * j + k] = number();
        for (int k = 0; k < 3; k++) c_b[3 * j + k] = number();
        for (int k = 0; k < 3; k++) axis_a[3 * j + k] = number();
        for (int k = 0; k < 3; k++) axis_b[3 * j + k] = number();
      }
      std::vector<mocap::JpDir> table;
      const char* why = mocap::jp_dir_table(B, n_markers.data(), markers.data(), J, a.data(), b.data(), kind.data(), c_a.data(), c_b.data(),
                                            axis_a.data(), axis_b.data(), axis_len, table, first.data());
      if (why) {
        std::printf("0\n");
      } else {
        std::printf("1");
        for (int32_t v : first) std::printf(" %d", v);
        for (const mocap::JpDir& d : table) {
          std::printf(" %d %d %d", d.j, d.x, d.kind);
          for (const double* p : {d.v0, d.v1, d.c_x, d.ax_x})
            for (int k = 0; k < 3; k++) std::printf(" %.17g", p[k]);
          for (int k = 0; k < 4; k++) std::printf(" %llu", d.mask[k]);
        }
        std::printf("\n");
      }
    }
    lines++;
  }
  std::fprintf(stderr, "%ld lines ok\n", lines);
  return 0;
}
