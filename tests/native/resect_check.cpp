// Stand-alone host build of csrc/resect_math.hpp (tests/test_resection_reference_cpu.py builds and runs it; no GPU, no library): the
// arithmetic of the camera resection on inputs read from stdin, the results printed as bit patterns, which the test compares with
// tests/resection_reference.py.  Every double travels as 16 hex digits.
//   input   fx fy cx cy threshold (5 words), the number of rows, then 5 words per row (X, u, v); then commands, one per line:
//             sample SEED H N            -> "i0 i1 i2"
//             score POSE[12]             -> "count mask" (the mask as a string of 0 and 1)
//             row I POSE[12]             -> the 31 words one inlier row contributes to a linearisation
//             refine MAX_ITER POSE[12]   -> "POSE[12] accepted linearisations": the two rounds, the sums folded in row order
//             p3p I0 I1 I2               -> "n" and 12 n words
//             end
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "resect_math.hpp"

static bool read_word(double& d) {
  uint64_t w;
  if (std::scanf("%" SCNx64, &w) != 1) return false;
  std::memcpy(&d, &w, 8);
  return true;
}

static void print_word(double d) {
  uint64_t w;
  std::memcpy(&w, &d, 8);
  std::printf("%016" PRIx64, w);
}

static bool read_pose(double* p) {
  for (int k = 0; k < 12; k++)
    if (!read_word(p[k])) return false;
  return true;
}

int main() {
  using namespace mocap;
  double k4[4], thr;
  for (double& k : k4)
    if (!read_word(k)) return 2;
  if (!read_word(thr)) return 2;
  const double thr2 = thr * thr;
  long n = 0;
  if (std::scanf("%ld", &n) != 1 || n < 0 || n > kRsMaxPoints) return 2;
  std::vector<double> rows((size_t)n * 5);
  for (double& r : rows)
    if (!read_word(r)) return 2;
  std::vector<char> mask((size_t)n);
  const double* K = k4;
  auto view_of = [&](const double* pose, long i, RsView& w) {
    const double* r = rows.data() + 5 * (size_t)i;
    rs_view(pose, K, r[0], r[1], r[2], r[3], r[4], w);
  };
  char cmd[16];
  while (std::scanf("%15s", cmd) == 1) {
    const std::string c(cmd);
    double pose[12];
    if (c == "end") {
      std::printf("resect checks done\n");
      return 0;
    } else if (c == "sample") {
      uint64_t seed;
      unsigned h, m;
      if (std::scanf("%" SCNu64 " %u %u", &seed, &h, &m) != 3 || m < 3) return 2;
      int idx[3];
      rs_sample(seed, h, m, idx);
      std::printf("%d %d %d\n", idx[0], idx[1], idx[2]);
    } else if (c == "score") {
      if (!read_pose(pose)) return 2;
      long count = 0;
      std::string bits((size_t)n, '0');
      for (long i = 0; i < n; i++) {
        RsView w;
        view_of(pose, i, w);
        if (rs_inlier(w, thr2)) {
          bits[(size_t)i] = '1';
          count++;
        }
      }
      std::printf("%ld %s\n", count, bits.c_str());
    } else if (c == "row") {
      long i;
      if (std::scanf("%ld", &i) != 1 || i < 0 || i >= n || !read_pose(pose)) return 2;
      RsView w;
      view_of(pose, i, w);
      double s[kRsSums];
      rs_row(w, K, s);
      for (int k = 0; k < kRsSums; k++) {
        print_word(s[k]);
        std::printf(k + 1 < kRsSums ? " " : "\n");
      }
    } else if (c == "refine") {
      int max_iter;
      if (std::scanf("%d", &max_iter) != 1 || max_iter < 0 || !read_pose(pose)) return 2;
      auto lin = [&](const double* p, const double* base, const double* inc, double* sums) {
        for (int k = 0; k < kRsSums; k++) sums[k] = 0.0;
        for (long i = 0; i < n; i++) {
          RsView w;
          view_of(p, i, w);
          if (!base) mask[(size_t)i] = rs_inlier(w, thr2) ? 1 : 0;
          if (!mask[(size_t)i]) continue;
          double s[kRsSums];
          rs_row(w, K, s);
          if (base) {
            RsView b;
            view_of(base, i, b);
            s[kRsDelta] = rs_delta_row(b, inc, K);
          }
          for (int k = 0; k < kRsSums; k++) sums[k] = sums[k] + s[k];
        }
        return true;
      };
      int accepted = 0, lins = 0;
      for (int round = 0; round < 2; round++) {
        RsRound out;
        if (!rs_round(pose, max_iter, lin, out)) return 3;
        accepted += out.accepted;
        lins += out.linearisations;
      }
      for (int k = 0; k < 12; k++) {
        print_word(pose[k]);
        std::printf(" ");
      }
      std::printf("%d %d\n", accepted, lins);
    } else if (c == "p3p") {
      long i[3];
      if (std::scanf("%ld %ld %ld", &i[0], &i[1], &i[2]) != 3) return 2;
      double P[3][3], uv[3][2], poses[48];
      for (int k = 0; k < 3; k++) {
        if (i[k] < 0 || i[k] >= n) return 2;
        const double* r = rows.data() + 5 * (size_t)i[k];
        for (int e = 0; e < 3; e++) P[k][e] = r[e];
        uv[k][0] = r[3];
        uv[k][1] = r[4];
      }
      const int ns = rs_p3p(P, uv, K, poses);
      std::printf("%d", ns);
      for (int k = 0; k < 12 * ns; k++) {
        std::printf(" ");
        print_word(poses[k]);
      }
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 2;
}
