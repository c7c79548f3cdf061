// The threshold of the mirror sweep (mirror_threshold and mirror_prescale, reak_amd/csrc/nn_mirror.h) on the host, for
// tests/test_nn_mirror_band_cpu.py: built with AddressSanitizer and UBSan and run directly.  The header's host part
// uses no HIP: a host compiler reads the arithmetic the thr kernel runs.
//
//   nn_mirror_band_host thr       reads lines  cmin qh2 dq qn dx X  (six numbers, decimal or hexadecimal floats, in the
//                                 mirror's prescaled units) and prints per line the threshold as the kernel stores it:
//                                 rounded up to float, as a hexadecimal float; +inf for cmin = +inf
//   nn_mirror_band_host prescale  reads coordinate bounds, one per line, and prints the prescale of each
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nn_mirror.h"

static float float_up(double v) {  // __double2float_ru
  float f = float(v);
  if (double(f) < v) f = std::nextafterf(f, INFINITY);
  return f;
}

int main(int argc, char** argv) {
  if (argc != 2 || (std::strcmp(argv[1], "thr") != 0 && std::strcmp(argv[1], "prescale") != 0)) {
    std::fprintf(stderr, "usage: nn_mirror_band_host thr|prescale < numbers\n");
    return 2;
  }
  const bool thr = std::strcmp(argv[1], "thr") == 0;
  char line[512];
  while (std::fgets(line, sizeof(line), stdin)) {
    double v[6];
    const int want = thr ? 6 : 1;
    char* p = line;
    for (int i = 0; i < want; ++i) {
      char* end = nullptr;
      v[i] = std::strtod(p, &end);
      if (end == p) {
        std::fprintf(stderr, "nn_mirror_band_host: expected %d numbers in: %s", want, line);
        return 1;
      }
      p = end;
    }
    if (thr) {
      const float t = v[0] < INFINITY ? float_up(rkh::mirror_threshold(v[0], v[1], v[2], v[3], v[4], v[5])) : INFINITY;
      std::printf("%a\n", double(t));
    } else {
      std::printf("%a\n", rkh::mirror_prescale(v[0]));
    }
  }
  return 0;
}
