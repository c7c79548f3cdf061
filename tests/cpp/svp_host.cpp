// svp_host.cpp -- reak_amd/csrc/svp_device.h read by a host compiler (through the stand-in for <hip/hip_runtime.h> in
// tests/cpp/hip_host) and checked against values worked out by hand.  A program of its own: built with
// -fsanitize=address,undefined -ffp-contract=off and run by tests/test_svp_space_cpu.py, which also compares the hex
// doubles printed at the end, bit for bit, with the Python twin (tests/svp_ref.py).
//
// The hand-worked cases, one joint, vm = 1 unless said (ramps change the velocity at rate 1, the position at rate v / vm):
//  minimum time
//   M1  same point (0, 0.3) -> (0, 0.3): 0, peak = v0; and (0, 2) -> (0, 2): still 0 -- the shortcut comes before the
//       velocity test
//   M2  (0, 1.5) -> (1, 0): a velocity beyond vm, infeasible
//   M3  (0, 0) -> (3, 0): full-speed cruise; each ramp takes 1 and covers 0.5, the cruise covers 2: T = 4, peak = 1; towards
//       -3: peak = -1
//   M4  (0, 0) -> (0.25, 0): no cruise, peak = sqrt(0.25) = 0.5, T = 1
//   M5  (0, 0.9) -> (0.01, 0.1): too fast to stop short; sqrt(0.01 + 0.405 + 0.005) < 0.9 rules the forward peak out, the
//       peak is -sqrt(0.41 - 0.01) (the joint overshoots and comes back), T = 2 sqrt(0.4) + 1.  (The other sign of this
//       branch needs sqrt(q - d) < min and sqrt(q + d) <= max of the end speeds at once, q the mean square: no real
//       numbers do that.)
//   M6  a NaN position: every comparison fails down to the last return, infeasible
//  peak velocity for a given T
//   P1  (0, 0) -> (1, 0), T = 2.5: roots of the first quadratic 2 (beyond 1.001 vm) and 0.5; ramps cover 0.125 each, the
//       cruise 1.5 x 0.5: 1.  peak = 0.5
//   P2  the same with T = 2 - 1e-7: the discriminant is -4e-7, inside the 1e-5 band: the double root 0.5 (v0 + v1 + T)
//   P3  (0, 0) -> (0.25, 0.5), T = 1: two ramps up through 0.25: 0.03125 + 0.125 + 0.09375 = 0.25
//   P4  (0, 0.5) -> (0.25, 0), T = 1: two ramps down through 0.25
//   P5  (0, 0.8) -> (0.7, 0.8), T = 1.7: the peak below both: ramps to 0.2 cover 0.3 each in 0.6, the cruise 0.1 in 0.5
//   P6  (0, 0.74) -> (0.41, 0.95), T = 0.69505 (its minimum is 0.44505): no root passes, infeasible -- the gap of a
//       velocity-bounded double integrator that cannot stretch its time
//   P7  velocity beyond vm: infeasible, and the same-point shortcut first
//  point of a profile: P1's, ramp 0.5 / cruise 1.5 / ramp 0.5, at 0, 0.25, 1.25 (blend of 0.125 and 0.875), 2.25, 2.5, 3;
//   and a first ramp at vm = 2: the position moves half as far
//  bounds, box [-1, 1]: (0.9, 0.5) stops at 1.025: out; (0.8, 0.5): in; (-0.9, 0.5) would have started at -1.025: out;
//   (0.875, 0.5) stops at 1.0 exactly: in; (0, 1.5): velocity out; (1.5, 0): out; (1, 0): in
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../reak_amd/csrc/svp_device.h"

using namespace rkh;

static int g_fail = 0;
static void near(const char* what, double got, double want, double tol = 1e-15) {
  if (!(std::fabs(got - want) <= tol)) {
    std::printf("FAIL %s: got %.17g, want %.17g\n", what, got, want);
    ++g_fail;
  }
}
static void truth(const char* what, bool got, bool want) {
  if (got != want) {
    std::printf("FAIL %s: got %d, want %d\n", what, int(got), int(want));
    ++g_fail;
  }
}

static void hand_cases() {
  double t, vp, p, v;
  truth("M1 ok", svp_joint_min_time(0, 0, 0.3, 0.3, 1, &t, &vp), true);
  near("M1 t", t, 0), near("M1 peak", vp, 0.3);
  truth("M1b ok", svp_joint_min_time(0, 0, 2, 2, 1, &t, &vp), true);
  near("M1b t", t, 0), near("M1b peak", vp, 2);
  truth("M2", svp_joint_min_time(0, 1, 1.5, 0, 1, &t, &vp), false);
  truth("M3 ok", svp_joint_min_time(0, 3, 0, 0, 1, &t, &vp), true);
  near("M3 t", t, 4), near("M3 peak", vp, 1);
  truth("M3b ok", svp_joint_min_time(0, -3, 0, 0, 1, &t, &vp), true);
  near("M3b t", t, 4), near("M3b peak", vp, -1);
  truth("M4 ok", svp_joint_min_time(0, 0.25, 0, 0, 1, &t, &vp), true);
  near("M4 t", t, 1), near("M4 peak", vp, 0.5);
  truth("M5 ok", svp_joint_min_time(0, 0.01, 0.9, 0.1, 1, &t, &vp), true);
  near("M5 t", t, 2 * std::sqrt(0.4) + 1, 4e-15), near("M5 peak", vp, -std::sqrt(0.4), 4e-15);
  truth("M6", svp_joint_min_time(NAN, 1, 0, 0, 1, &t, &vp), false);

  truth("P1 ok", svp_joint_peak(0, 1, 0, 0, 1, 2.5, &vp), true);
  near("P1 peak", vp, 0.5);
  truth("P2 ok", svp_joint_peak(0, 1, 0, 0, 1, 2 - 1e-7, &vp), true);
  near("P2 peak", vp, 0.5 * (2 - 1e-7));
  truth("P3 ok", svp_joint_peak(0, 0.25, 0, 0.5, 1, 1, &vp), true);
  near("P3 peak", vp, 0.25);
  truth("P4 ok", svp_joint_peak(0, 0.25, 0.5, 0, 1, 1, &vp), true);
  near("P4 peak", vp, 0.25);
  truth("P5 ok", svp_joint_peak(0, 0.7, 0.8, 0.8, 1, 1.7, &vp), true);
  near("P5 peak", vp, 0.2, 1e-14);
  truth("P6 min", svp_joint_min_time(0, 0.41, 0.74, 0.95, 1, &t, &vp), true);
  near("P6 min t", t, 0.44505, 1e-14);
  truth("P6", svp_joint_peak(0, 0.41, 0.74, 0.95, 1, 0.69505, &vp), false);
  truth("P7", svp_joint_peak(0, 1, 0, 1.5, 1, 5, &vp), false);
  truth("P7b ok", svp_joint_peak(0, 0, 1.5, 1.5, 1, 5, &vp), true);
  near("P7b peak", vp, 1.5);

  const double at[6] = {0, 0.25, 1.25, 2.25, 2.5, 3}, wp[6] = {0, 0.03125, 0.5, 0.96875, 1, 1}, wv[6] = {0, 0.25, 0.5, 0.25, 0, 0};
  for (int k = 0; k < 6; ++k) {
    svp_joint_point(0, 1, 0, 0, 0.5, 1, at[k], 2.5, &p, &v);
    near("point p", p, wp[k]), near("point v", v, wv[k]);
  }
  svp_joint_point(0, 1, 0, 0, 0.5, 2, 0.5, 10, &p, &v);
  near("point vm 2 p", p, 0.0625), near("point vm 2 v", v, 0.5);

  SvpDev sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.n = 1, sp.lower[0] = -1, sp.upper[0] = 1, sp.vm[0] = sp.speed[0] = sp.accel[0] = 1;
  const double pts[7][2] = {{0.9, 0.5}, {0.8, 0.5}, {-0.9, 0.5}, {0.875, 0.5}, {0, 1.5}, {1.5, 0}, {1, 0}};
  const bool want[7] = {false, true, false, true, false, false, true};
  for (int k = 0; k < 7; ++k) truth("bounds", svp_in_bounds(sp, pts[k]), want[k]);

  // two joints: the slower one sets T, the other stretches (P1), peaks of both
  sp.n = 2, sp.vm[1] = sp.speed[1] = sp.accel[1] = 1, sp.lower[1] = -4, sp.upper[1] = 4;
  const double a[4] = {0, 0, 0, 0}, b[4] = {1, 0, 0.5625, 0};  // joint 1 alone: sqrt(0.5625) = 0.75, T = 1.5 < 2
  double peak[2];
  near("pair T", svp_reach(sp, a, b, peak), 2);
  near("pair peak 0", peak[0], 1);
  // joint 1 in T = 2: 0.5 (2 - sqrt(4 - 2.25)) = 0.5 (2 - sqrt(1.75))
  near("pair peak 1", peak[1], 0.5 * (2 - std::sqrt(1.75)), 2e-15);
  const double c[4] = {0, 0, 0, 1.5};
  truth("pair inf", std::isinf(svp_reach(sp, a, c, peak)), true);
  near("pair inf peak", peak[0] + peak[1], 0);
  bool over;
  truth("count 3", svp_count_points(0.25, 1.0, 100, &over) == 3 && !over, true);  // 0.25, 0.5, 0.75
  truth("count 0", svp_count_points(0.25, 0.25, 100, &over) == 0 && !over, true);
  truth("count cap", svp_count_points(0.25, 100.0, 8, &over) == 8 && over, true);
}

// the seeded list the twin repeats: a 64-bit LCG, 53 bits to a double in [0, 1)
static unsigned long long g_state = 20261020ull;
static double uni() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return double(g_state >> 11) / 9007199254740992.0;
}
static double range(double lo, double hi) { return lo + (hi - lo) * uni(); }

int main() {
  hand_cases();
  SvpDev sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.n = 3;
  const double speed[3] = {1.0, 0.5, 3.0}, accel[3] = {1.0, 1.0, 1.5};
  for (int i = 0; i < 3; ++i)
    sp.speed[i] = speed[i], sp.accel[i] = accel[i], sp.vm[i] = speed[i] / accel[i], sp.lower[i] = -2, sp.upper[i] = 2;
  for (int e = 0; e < 400; ++e) {
    double a[6], b[6], peak[3], x[6], xm[6];
    for (int i = 0; i < 3; ++i) {
      a[2 * i] = range(-2, 2), a[2 * i + 1] = range(-sp.vm[i], sp.vm[i]);
      b[2 * i] = (e % 5 == 0) ? a[2 * i] + range(-0.05, 0.05) : range(-2, 2);
      b[2 * i + 1] = range(-sp.vm[i], sp.vm[i]);
    }
    const double T = svp_reach(sp, a, b, peak);
    std::printf("pair %d %a %a %a %a", e, T, peak[0], peak[1], peak[2]);
    if (T < INFINITY) {
      svp_point(sp, a, b, peak, T, 0.37 * T, x, xm);
      for (int c = 0; c < 6; ++c) std::printf(" %a", x[c]);
      for (int c = 0; c < 6; ++c) std::printf(" %a", xm[c]);
    }
    std::printf(" %d %d\n", int(svp_in_bounds(sp, a)), int(svp_in_bounds(sp, b)));
  }
  if (g_fail) return 1;
  std::printf("svp host ok: hand-worked cases of the three closed forms and the bounds rule, 400 seeded pairs printed\n");
  return 0;
}
