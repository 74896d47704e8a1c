// Stand-alone host build of csrc/precision_host.hpp and csrc/precision_math.hpp (tests/test_precision_native_cpu.py builds it with
// AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a process of its own; no GPU, no library): the fold of the caller's
// coordinates, the argument rules and the per-point arithmetic of "predicted precision" on cases read from stdin, the results printed
// as bit patterns, which the test compares with tests/precision_reference.py.  Every double travels as 16 hex digits; every array is
// a heap block of exactly the contract's size.
//   fold    C, 12 C words, has_frame, then 12 words when it has one                 -> 12 C words
//   args    lines  "common sigma has_frame [12 words]" | "vis width height near far" | "points N" | "frames n_frames K_max" |
//           "map nx ny nz min_views max_sigma"  -> "1" the rule stands, "0" refused;   "init nx ny nz" -> the 72 integers
//   point   C, 12 C words, sigma, by_vis, width height near far (words), the number of cases; per case x y z (words) and the view
//           mask (hex)  -> "info n_views seen sig[3] axis[3] cov[6]"
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "precision_host.hpp"
#include "precision_math.hpp"

using namespace mocap;

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

static bool read_table(int& C, std::vector<double>& P) {
  if (std::scanf("%d", &C) != 1 || C < 1 || C > 64) return false;
  P.resize((size_t)12 * C);
  for (double& p : P)
    if (!read_word(p)) return false;
  return true;
}

static int run_fold() {
  int C = 0, has = 0;
  std::vector<double> P;
  if (!read_table(C, P) || std::scanf("%d", &has) != 1) return 2;
  std::vector<double> frame(has ? 12 : 0), out((size_t)12 * C);
  for (double& f : frame)
    if (!read_word(f)) return 2;
  pm_fold(C, P.data(), has ? frame.data() : nullptr, out.data());
  for (double o : out) std::printf("%016" PRIx64 " ", bits(o));
  std::printf("\n");
  return 0;
}

static int run_args() {
  char kind[16];
  long lines = 0;
  while (std::scanf("%15s", kind) == 1) {
    const std::string k = kind;
    const char* why = nullptr;
    if (k == "common") {
      double sigma;
      int has = 0;
      if (!read_word(sigma) || std::scanf("%d", &has) != 1) return 2;
      std::vector<double> frame(has ? 12 : 0);
      for (double& f : frame)
        if (!read_word(f)) return 2;
      why = pm_common_check(sigma, has ? frame.data() : nullptr);
    } else if (k == "vis") {
      int w, h;
      double near, far;
      if (std::scanf("%d %d", &w, &h) != 2 || !read_word(near) || !read_word(far)) return 2;
      why = pm_vis_check(w, h, near, far);
    } else if (k == "points") {
      long long N;
      if (std::scanf("%lld", &N) != 1) return 2;
      why = pm_points_check(N);
    } else if (k == "frames") {
      long long F;
      int K;
      if (std::scanf("%lld %d", &F, &K) != 2) return 2;
      why = pm_frames_check(F, K);
    } else if (k == "map") {
      int nx, ny, nz, mv;
      double ms;
      if (std::scanf("%d %d %d %d", &nx, &ny, &nz, &mv) != 4 || !read_word(ms)) return 2;
      why = pm_map_check(nx, ny, nz, mv, ms);
    } else if (k == "init") {
      int nx, ny, nz;
      if (std::scanf("%d %d %d", &nx, &ny, &nz) != 3) return 2;
      std::vector<int64_t> s((size_t)kPmSummary);
      pm_summary_init(nx, ny, nz, s.data());
      for (int64_t v : s) std::printf("%" PRId64 " ", v);
      std::printf("\n");
      lines++;
      continue;
    } else {
      return 2;
    }
    std::printf("%d\n", why ? 0 : 1);
    lines++;
  }
  std::fprintf(stderr, "%ld lines ok\n", lines);
  return 0;
}

static int run_point() {
  int C = 0, by_vis = 0;
  std::vector<double> P;
  double sigma;
  PmVis vis;
  long cases = 0;
  if (!read_table(C, P) || !read_word(sigma) || std::scanf("%d", &by_vis) != 1 || !read_word(vis.width) || !read_word(vis.height) ||
      !read_word(vis.near) || !read_word(vis.far) || std::scanf("%ld", &cases) != 1 || cases < 0)
    return 2;
  for (long i = 0; i < cases; i++) {
    double x[3];
    uint64_t mask;
    if (!read_word(x[0]) || !read_word(x[1]) || !read_word(x[2]) || std::scanf("%" SCNx64, &mask) != 1) return 2;
    auto named = [&](int c) -> bool { return (mask >> c) & 1; };
    const double* table = P.data();
    PmPoint o;
    pm_point(C, table, by_vis != 0, named, vis, sigma, x[0], x[1], x[2], o);
    std::printf("%d %d %016" PRIx64, o.info, o.n_views, o.seen);
    for (double v : o.sig) std::printf(" %016" PRIx64, bits(v));
    for (double v : o.axis) std::printf(" %016" PRIx64, bits(v));
    for (double v : o.cov) std::printf(" %016" PRIx64, bits(v));
    std::printf("\n");
  }
  std::fprintf(stderr, "%ld cases ok\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "fold") return run_fold();
  if (mode == "args") return run_args();
  if (mode == "point") return run_point();
  return 2;
}
