// bal_view_host.cpp -- the per-view arithmetic of the lens calibration (csrc/ba_lens.hpp: bal_lens, bal_view, bal_undistort) as a
// stand-alone host program, for AddressSanitizer / UndefinedBehaviorSanitizer runs on the CPU (tests/test_ba_lens_native_cpu.py).
//   bal_view_host views < in      lines "24 camera doubles, X 3, u v, huber" -> per line: ok down rho ru rv Bu[3] Bv[3] Au[14] Av[14]
//   bal_view_host undistort < in  lines "K 9, dist 5, u v"                   -> per line: u' v'
// Numbers are written with 17 significant digits: they read back as the same doubles.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../low-cost-mocap_amd/csrc/ba_lens.hpp"

using namespace mocap;

static bool read_doubles(double* v, int n) {
  for (int i = 0; i < n; i++)
    if (std::scanf("%lf", v + i) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  static_assert(bal_row_off(0) == 0 && bal_row_off(1) == 15 && bal_row_off(4) == 25 && bal_row_off(8) == 27 && bal_row_off(13) == 18, "bands");
  static_assert(bal_row_off(1) + 14 == 29 && bal_row_off(4) + 11 == kBalSlab && bal_row_off(8) + 7 == 34 && bal_row_off(13) + 2 == kBalCount,
                "the bands fill 29, 36, 34 and 20 slots");
  long lines = 0;
  if (!std::strcmp(argv[1], "views")) {
    std::vector<double> in(kBalCam + 6);
    while (read_doubles(in.data(), kBalCam + 6)) {
      const double X[3] = {in[kBalCam], in[kBalCam + 1], in[kBalCam + 2]};
      BalView w;
      bal_view((const double*)in.data(), X, in[kBalCam + 3], in[kBalCam + 4], in[kBalCam + 5], w);
      std::printf("%d %d %.17g %.17g %.17g", (int)w.ok, (int)w.down, w.rho, w.ru, w.rv);
      for (int j = 0; j < 3; j++) std::printf(" %.17g", w.Bu[j]);
      for (int j = 0; j < 3; j++) std::printf(" %.17g", w.Bv[j]);
      for (int j = 0; j < kBalPar; j++) std::printf(" %.17g", w.Au[j]);
      for (int j = 0; j < kBalPar; j++) std::printf(" %.17g", w.Av[j]);
      std::printf("\n");
      lines++;
    }
  } else if (!std::strcmp(argv[1], "undistort")) {
    double in[16];
    while (read_doubles(in, 16)) {
      double uo, vo;
      bal_undistort((const double*)in, (const double*)(in + 9), in[14], in[15], uo, vo);
      std::printf("%.17g %.17g\n", uo, vo);
      lines++;
    }
  } else {
    return 2;
  }
  std::fprintf(stderr, "bal_view_host: %ld lines ok\n", lines);
  return 0;
}
