// svp_rrt_host.cpp -- reak_amd/csrc/svp_rrt_device.h (with svp_device.h) read by a host compiler through the stand-in for
// <hip/hip_runtime.h> in tests/cpp/hip_host, and checked against values worked out by hand.  A program of its own: built
// with -fsanitize=address,undefined -ffp-contract=off and run by tests/test_svp_rrt_cpu.py, which also compares the
// candidates printed at the end, bit for bit, with the Python twin (tests/svp_rrt_ref.py).
//
// The hand-worked cases:
//  generator   std::mt19937's check value: seeded with 5489 its 10000th output is 4123659995; the state regenerated in the
//              three stretches the kernel uses
//  draw        y = 0 -> 0; y = 2^31 -> 0.5; y = 2^32 - 1 -> 1 - 2^-32, below 1
//  mapping     space of two joints, box [-1, 1] x [0, 4], vm = (0.5, 2): coordinate 0 from [-1, 1], 1 from [-0.5, 0.5],
//              2 from [0, 4], 3 from [-2, 2]; u = 0 gives lo, u = 0.25 of [-1, 1] gives -0.5, u = 0.5 of [0, 4] gives 2
//  fraction    asked 2, at most 1: 0.5; asked 0.5: 1; asked exactly 1: 1; asked 0 or below: 1
//  progress    asked 2 x fraction 0.5 = 1, tolerance 0.1: travelled 2 (equal to 2 x) is rejected, the double below 2 passes;
//              travelled 0.1 (equal to tol x) is rejected, the double above passes; +inf and NaN are rejected
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../reak_amd/csrc/svp_rrt_device.h"

using namespace rkh;

static int g_fail = 0;
static void truth(const char* what, bool got, bool want) {
  if (got != want) {
    std::printf("FAIL %s: got %d, want %d\n", what, int(got), int(want));
    ++g_fail;
  }
}
static void same(const char* what, double got, double want) {
  if (!(got == want)) {
    std::printf("FAIL %s: got %.17g, want %.17g\n", what, got, want);
    ++g_fail;
  }
}

struct Mt {  // the generator as the sample kernel keeps it: 624 words and a position
  std::vector<uint32_t> w;
  uint32_t idx;
  explicit Mt(uint32_t seed) : w(kRl1MtN), idx(kRl1MtN) {
    w[0] = seed;
    for (uint32_t k = 1; k < kRl1MtN; ++k) w[k] = rl1rrt_mt_seed_next(w[k - 1], k);
  }
  void stretch(uint32_t a, uint32_t b) {  // all of [a, b) from the words as they stand, then stored: as the lanes do
    std::vector<uint32_t> v(b - a);
    for (uint32_t i = a; i < b; ++i)
      v[i - a] = rl1rrt_mt_twist(w[i], w[i + 1], w[i + kRl1MtM < kRl1MtN ? i + kRl1MtM : i + kRl1MtM - kRl1MtN]);
    for (uint32_t i = a; i < b; ++i) w[i] = v[i - a];
  }
  uint32_t next() {
    if (idx == kRl1MtN) {
      stretch(0, kRl1MtN - kRl1MtM);
      stretch(kRl1MtN - kRl1MtM, 2 * (kRl1MtN - kRl1MtM));
      stretch(2 * (kRl1MtN - kRl1MtM), kRl1MtN - 1);
      w[kRl1MtN - 1] = rl1rrt_mt_twist(w[kRl1MtN - 1], w[0], w[kRl1MtM - 1]);
      idx = 0;
    }
    return rl1rrt_mt_temper(w[idx++]);
  }
};

int main() {
  {
    Mt g(5489u);
    uint32_t y = 0;
    for (int k = 0; k < 10000; ++k) y = g.next();
    truth("mt19937 check value", y == 4123659995u, true);
  }
  same("unit 0", rl1rrt_unit(0u), 0.0);
  same("unit half", rl1rrt_unit(0x80000000u), 0.5);
  same("unit last", rl1rrt_unit(0xFFFFFFFFu), 1.0 - 1.0 / 4294967296.0);
  truth("unit below 1", rl1rrt_unit(0xFFFFFFFFu) < 1.0, true);

  SvpDev sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.n = 2;
  sp.lower[0] = -1, sp.upper[0] = 1, sp.lower[1] = 0, sp.upper[1] = 4;
  sp.speed[0] = 1, sp.accel[0] = 2, sp.vm[0] = 0.5, sp.speed[1] = 4, sp.accel[1] = 2, sp.vm[1] = 2;
  const double want_lo[4] = {-1, -0.5, 0, -2}, want_hi[4] = {1, 0.5, 4, 2};
  for (uint32_t c = 0; c < 4; ++c) {
    double lo = 0, hi = 0;
    rl1rrt_coord_range(sp, c, &lo, &hi);
    same("range lo", lo, want_lo[c]), same("range hi", hi, want_hi[c]);
    same("coord at 0", rl1rrt_coord(lo, hi, 0.0), lo);
    truth("coord below hi", rl1rrt_coord(lo, hi, rl1rrt_unit(0xFFFFFFFFu)) < hi, true);
  }
  same("coord quarter", rl1rrt_coord(-1, 1, 0.25), -0.5);
  same("coord half", rl1rrt_coord(0, 4, 0.5), 2.0);

  same("fraction 2", rl1rrt_fraction(2.0, 1.0), 0.5);
  same("fraction 0.5", rl1rrt_fraction(0.5, 1.0), 1.0);
  same("fraction 1", rl1rrt_fraction(1.0, 1.0), 1.0);
  same("fraction 0", rl1rrt_fraction(0.0, 1.0), 1.0);
  same("fraction negative", rl1rrt_fraction(-3.0, 1.0), 1.0);
  same("fraction 3 of 0.75", rl1rrt_fraction(3.0, 0.75), 0.25);

  truth("progress middle", rl1rrt_progress(1.0, 2.0, 0.5, 0.1), true);
  truth("progress equal to 2x", rl1rrt_progress(2.0, 2.0, 0.5, 0.1), false);
  truth("progress below 2x", rl1rrt_progress(std::nextafter(2.0, 0.0), 2.0, 0.5, 0.1), true);
  truth("progress equal to tol x", rl1rrt_progress(0.1, 2.0, 0.5, 0.1), false);
  truth("progress above tol x", rl1rrt_progress(std::nextafter(0.1, 1.0), 2.0, 0.5, 0.1), true);
  truth("progress below tol x", rl1rrt_progress(0.05, 2.0, 0.5, 0.1), false);
  truth("progress inf", rl1rrt_progress(INFINITY, 2.0, 0.5, 0.1), false);
  truth("progress nan", rl1rrt_progress(NAN, 2.0, 0.5, 0.1), false);
  truth("progress of nothing asked", rl1rrt_progress(0.0, 0.0, 1.0, 0.1), false);

  // 700 candidates of seed 7 (2800 draws: the 624-word boundary four times), for the twin
  Mt g(7u);
  for (int k = 0; k < 700; ++k) {
    double x[4];
    for (uint32_t c = 0; c < 4; ++c) {
      double lo, hi;
      rl1rrt_coord_range(sp, c, &lo, &hi);
      x[c] = rl1rrt_coord(lo, hi, rl1rrt_unit(g.next()));
    }
    std::printf("cand %d %a %a %a %a %d\n", k, x[0], x[1], x[2], x[3], int(svp_in_bounds(sp, x)));
  }
  if (g_fail) return 1;
  std::printf("svp rrt host ok: generator, draw, coordinate mapping, steer fraction, progress rule; 700 candidates printed\n");
  return 0;
}
