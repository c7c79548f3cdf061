// svp_rrt_device.h -- the scalar rules of the batch RRT over the SVP space (svp_planner.hip), as functions a host compiler
// reads too (tests/cpp/svp_rrt_host.cpp) and the Python twin restates (tests/svp_rrt_ref.py):
//   the sample stream     std::mt19937 (seeding, twist, tempering), draw -> u = y 2^-32, coordinate = lo + u (hi - lo) with
//                         the grouping of the other planners' stream; (lo, hi) = the position box for p_i, -+vm_i for v_i.
//                         Candidate k takes draws k D .. k D + D - 1 (D = 2 n) in point order, accepted or not.
//   the steer fraction    min(1, max_edge_time / asked), 1 for asked <= 0
//   the progress test     travelled finite, < 2 asked fraction and > steer_tol asked fraction, both strict
// Only +, -, *, / and comparisons in fp64, written with their grouping; nothing here uses a device builtin.
#pragma once
#include "svp_device.h"

namespace rkh {

constexpr uint32_t kRl1MtN = 624, kRl1MtM = 397;

// word k of the state seeded with `seed`, from word k - 1 (word 0 is the seed): std::mt19937's seeding
RKH_HD uint32_t rl1rrt_mt_seed_next(uint32_t prev, uint32_t k) { return 1812433253u * (prev ^ (prev >> 30)) + k; }

// new[i] from old[i], old[i + 1] and the word (i + 397) mod 624 as it stands when i is reached
RKH_HD uint32_t rl1rrt_mt_twist(uint32_t cur, uint32_t nxt, uint32_t far) {
  const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7fffffffu);
  return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

RKH_HD uint32_t rl1rrt_mt_temper(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}

// a draw as a number in [0, 1): < 1 for every 32-bit y
RKH_HD double rl1rrt_unit(uint32_t y) { return double(y) * (1.0 / 4294967296.0); }

// the interval coordinate c of a candidate is drawn from: even c = position of joint c / 2, odd c = its velocity
RKH_HD void rl1rrt_coord_range(const SvpDev& sp, uint32_t c, double* lo, double* hi) {
  const uint32_t i = c >> 1;
  if (c & 1u) *lo = -sp.vm[i], *hi = sp.vm[i];
  else *lo = sp.lower[i], *hi = sp.upper[i];
}

RKH_HD double rl1rrt_coord(double lo, double hi, double u) { return lo + u * (hi - lo); }

RKH_HD double rl1rrt_fraction(double asked, double max_edge_time) {
  if (!(asked > 0.0)) return 1.0;
  const double f = max_edge_time / asked;
  return (f < 1.0) ? f : 1.0;
}

RKH_HD bool rl1rrt_progress(double travelled, double asked, double fraction, double steer_tol) {
  const double best = asked * fraction;
  return (travelled < INFINITY) && (travelled > -INFINITY) && (travelled < 2.0 * best) && (travelled > steer_tol * best);
}

}  // namespace rkh
