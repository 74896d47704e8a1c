// Stand-alone host build of csrc/refine_lm.hpp (tests/test_point_refine_reference_cpu.py builds and runs it; no GPU, no library):
// the Levenberg-Marquardt arithmetic of the point refinement on cases read from stdin, the results printed as bit patterns, which
// the test compares with tests/point_refine_reference.py.  Every double travels as 16 hex digits.
//   input   C, then 12 C words (the camera table), then the number of cases; per case: iters, n, the start (3 words), then n
//           lines "camera u v" in ascending camera order
//   output  per case one line: "0" (start not finite or not valid), or "1 x y z err accepted"
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "refine_lm.hpp"

static bool read_word(double& d) {
  uint64_t w;
  if (std::scanf("%" SCNx64, &w) != 1) return false;
  std::memcpy(&d, &w, 8);
  return true;
}

static uint64_t bits(double d) {
  uint64_t w;
  std::memcpy(&w, &d, 8);
  return w;
}

int main() {
  int C = 0;
  if (std::scanf("%d", &C) != 1 || C < 1 || C > 64) return 2;
  std::vector<double> P((size_t)12 * C);
  for (double& p : P)
    if (!read_word(p)) return 2;
  long cases = 0;
  if (std::scanf("%ld", &cases) != 1 || cases < 0) return 2;
  std::vector<double> u((size_t)C), v((size_t)C);
  std::vector<char> seen((size_t)C);
  for (long i = 0; i < cases; i++) {
    int iters = 0, n = 0;
    double X[3];
    if (std::scanf("%d %d", &iters, &n) != 2 || iters < 0 || iters > mocap::kRefineMaxIters || n < 0 || n > C) return 2;
    if (!read_word(X[0]) || !read_word(X[1]) || !read_word(X[2])) return 2;
    std::fill(seen.begin(), seen.end(), 0);
    for (int k = 0; k < n; k++) {
      int c = -1;
      double uu, vv;
      if (std::scanf("%d", &c) != 1 || c < 0 || c >= C || seen[(size_t)c] || !read_word(uu) || !read_word(vv)) return 2;
      seen[(size_t)c] = 1;
      u[(size_t)c] = uu;
      v[(size_t)c] = vv;
    }
    auto obs = [&](int c, double& x, double& y) -> bool {
      if (!seen[(size_t)c]) return false;
      x = u[(size_t)c];
      y = v[(size_t)c];
      return true;
    };
    double cost = 0.0;
    int accepted = 0;
    const double* table = P.data();
    if (!mocap::refine_lm(C, table, obs, iters, X, cost, accepted)) {
      std::printf("0\n");
      continue;
    }
    const double err = cost / (double)(2 * n);
    std::printf("1 %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d\n", bits(X[0]), bits(X[1]), bits(X[2]), bits(err), accepted);
  }
  std::printf("refine checks done\n");
  return 0;
}
