// Stand-alone host check of csrc/bb_fold.hpp (tests/test_gpu_bb_block_size.py builds and runs it; no GPU, no library):
// wherever the folded float word says "dropped", the double expression of the search, s1 * fma(2e-12, tr, y) < 1, says so too.
// Draws: log-uniform s1, tr, y over the ranges the bench frames produce and far around them; a second family with
// s1 * 2e-12 * tr placed near and above 1; the extremes (s1 above the float range and in the float denormals, y = +inf, y = 0).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include "bb_fold.hpp"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static double uni() {  // xorshift64*, (0, 1)
  state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
  return ((state * 0x2545F4914F6CDD1Dull) >> 11) * 0x1p-53 + 0x1p-54;
}
static double logu(double lo, double hi) { return std::exp(std::log(lo) + (std::log(hi) - std::log(lo)) * uni()); }

static long draws = 0, by_word = 0, by_double = 0, violations = 0;
static long bench_draws = 0, bench_by_word = 0, bench_by_double = 0;  // the plain draws from the bench's ranges: how much the word still drops
static void check(double s1, double tr, double y, bool bench = false) {
  const float q = mocap::bb_fold_bound(s1, tr);
  const bool w = mocap::bb_fold_dropped(q, y);
  const bool d = s1 * std::fma(2e-12, tr, y) < 1.0;
  draws++;
  by_word += w;
  by_double += d;
  if (bench) bench_draws++, bench_by_word += w, bench_by_double += d;
  if (w && !d) {
    if (violations < 10) std::printf("VIOLATION s1 %.17g tr %.17g y %.17g word %.9g\n", s1, tr, y, (double)q);
    violations++;
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  const double ys[] = {0.0, 1e-300, 1e-6, 1.0, 1e6, 1e300, inf};
  for (int i = 0; i < 1500000; i++) {  // the bench's ranges: s1 1e-8 .. 1e2, tr 1e4 .. 1e9, y 1e-6 .. 1e6 -- y placed around 1 / s1, where the decision is
    const double s1 = logu(1e-8, 1e2), tr = logu(1e4, 1e9);
    check(s1, tr, logu(1e-6, 1e6), true);
    check(s1, tr, (1.0 / s1) * (1.0 + (uni() - 0.5) * 1e-5));
    check(s1, tr, (1.0 / s1 - 2e-12 * tr) * (1.0 + (uni() - 0.5) * 0x1p-18));
  }
  for (int i = 0; i < 500000; i++) {  // far around them
    const double s1 = logu(1e-60, 1e60), tr = logu(1e-30, 1e40);
    check(s1, tr, logu(1e-80, 1e80));
    check(s1, tr, (1.0 / s1) * (1.0 + (uni() - 0.5) * 1e-6));
  }
  for (int i = 0; i < 300000; i++) {  // a = s1 2e-12 tr near and above 1
    const double s1 = logu(1e-3, 1e8);
    const double a = i % 3 == 0 ? 1.0 + (uni() - 0.5) * 0x1p-18 : (i % 3 == 1 ? 1.0 - logu(1e-16, 0.5) : logu(1.0, 1e6));
    const double tr = a / (s1 * 2e-12);
    for (double y : ys) check(s1, tr, y);
    check(s1, tr, std::fabs(1.0 - a) / s1 * (1.0 + (uni() - 0.5) * 1e-4));
  }
  for (int i = 0; i < 100000; i++) {  // the float range's ends
    const double tr = logu(1e-3, 1e9);
    for (double s1 : {logu(1e37, 1e40), logu(1e-47, 1e-36), logu(3.3e38, 3.5e38), inf, 0.0, std::nan("")})
      for (double y : ys) check(s1, tr, y);
  }
  std::printf("draws %ld dropped_by_word %ld dropped_by_double %ld violations %ld\n", draws, by_word, by_double, violations);
  std::printf("bench_draws %ld dropped_by_word %ld dropped_by_double %ld\n", bench_draws, bench_by_word, bench_by_double);
  return violations ? 1 : 0;
}
