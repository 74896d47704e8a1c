// skeleton_fit_host_check.cpp -- the host's part of "skeleton fit" (csrc/skeleton_fit_host.hpp: the argument rules of
// mocap_fit_skeleton, the joints' check shared with "joint poses", the directed joints and the forest's elimination tables) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_skeleton_fit_native_cpu.py and run as a process of its
// own.  Every array handed to the code under test is a heap block of exactly the size the contract names, so a read past it is seen.
//   skeleton_fit_host_check args    stdin: B J axis_len w_joint iters per line                      stdout: 1 (stands) or 0 (refused)
//   skeleton_fit_host_check table   stdin: B J, then per joint a b kind c_a[3] c_b[3] axis_a[3] axis_b[3], all on one line
//                                   stdout: 0, or 1, first[0 .. B], parent, depth, joint_up, order [B] each, child_of [J], and per
//                                   directed joint j x kind up c_y ax_y c_x ax_x
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../low-cost-mocap_amd/csrc/skeleton_fit_host.hpp"

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
      const double axis_len = number(), w_joint = number();
      const int iters = (int)number();
      std::printf("%d\n", mocap::sk_args_check(B, J, axis_len, w_joint, iters) ? 0 : 1);
    } else {
      const int B = (int)number(), J = (int)number();
      if (B < 2 || B > mocap::kSkMaxBodies || J < 1 || J > B - 1) return 3;  // (sk_args_check's part, always called first)
      const size_t n = (size_t)J;
      std::vector<int32_t> a(n), b(n), kind(n);
      std::vector<double> c_a(3 * n), c_b(3 * n), axis_a(3 * n), axis_b(3 * n);
      for (size_t j = 0; j < n; j++) {
        a[j] = (int32_t)number();
        b[j] = (int32_t)number();
        kind[j] = (int32_t)number();
        for (int k = 0; k < 3; k++) c_a[3 * j + k] = number();
        for (int k = 0; k < 3; k++) c_b[3 * j + k] = number();
        for (int k = 0; k < 3; k++) axis_a[3 * j + k] = number();
        for (int k = 0; k < 3; k++) axis_b[3 * j + k] = number();
      }
      std::vector<mocap::SkDir> dirs;
      std::vector<mocap::SkForest> fr(1);
      const char* why = mocap::sk_tables(B, J, a.data(), b.data(), kind.data(), c_a.data(), c_b.data(), axis_a.data(), axis_b.data(), dirs, fr[0]);
      if (why) {
        std::printf("0\n");
      } else {
        std::printf("1");
        for (int y = 0; y <= B; y++) std::printf(" %d", fr[0].first[y]);
        for (const int32_t* tab : {fr[0].parent, fr[0].depth, fr[0].joint_up, fr[0].order})
          for (int y = 0; y < B; y++) std::printf(" %d", tab[y]);
        for (int j = 0; j < J; j++) std::printf(" %d", fr[0].child_of[j]);
        for (const mocap::SkDir& d : dirs) {
          std::printf(" %d %d %d %d", d.j, d.x, d.kind, d.up);
          for (const double* p : {d.c_y, d.ax_y, d.c_x, d.ax_x})
            for (int k = 0; k < 3; k++) std::printf(" %.17g", p[k]);
        }
        std::printf("\n");
      }
    }
    lines++;
  }
  std::fprintf(stderr, "%ld lines ok\n", lines);
  return 0;
}
