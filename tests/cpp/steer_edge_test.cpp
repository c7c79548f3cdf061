// steer_edge_test.cpp -- the edge protocol of reak_amd/csrc/steer_edge.h at its edges, with hand-worked values.
// Host code only: built with the host compiler under AddressSanitizer + UBSan and run directly
// (tests/test_steer_edge_cpu.py).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "steer_edge.h"

using namespace rkh;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++g_checks;                                                      \
    if (!(cond)) {                                                   \
      ++g_failed;                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
    }                                                                \
  } while (0)

static const double kInf = std::numeric_limits<double>::infinity();
static const double kNaN = std::numeric_limits<double>::quiet_NaN();

static void test_gate() {
  KernelGate g;
  CHECK(!steer_gate_closed(&g));  // no counter: always open
  uint32_t count = 5;
  g.count = &count;
  g.lo = 5;
  g.hi = 6;
  CHECK(!steer_gate_closed(&g));  // lo <= count < hi
  g.lo = 6;
  g.hi = 9;
  CHECK(steer_gate_closed(&g));  // below lo
  g.lo = 0;
  g.hi = 5;
  CHECK(steer_gate_closed(&g));  // hi is exclusive
}

static void test_segment_of() {
  // segments of 0, 5, 0, 0, 4 entries: leading, inner and trailing empties around the two that hold something
  const uint32_t prefix[] = {0, 0, 5, 5, 5, 9};
  CHECK(segment_of(prefix, 5u, 0u) == 1u);
  CHECK(segment_of(prefix, 5u, 4u) == 1u);
  CHECK(segment_of(prefix, 5u, 5u) == 4u);
  CHECK(segment_of(prefix, 5u, 8u) == 4u);
  const uint32_t tail[] = {0, 3, 3, 3};  // trailing empties
  CHECK(segment_of(tail, 3u, 0u) == 0u);
  CHECK(segment_of(tail, 3u, 2u) == 0u);
  const uint32_t one[] = {0, 7};
  CHECK(segment_of(one, 1u, 6u) == 0u);
}

static void test_rows() {
  EdgeIO io;
  CHECK(edge_source_row(io, 3) == 3u && edge_target_row(io, 3) == 3ull);
  const uint32_t first = 10, off = 100;
  io.d_src_first = &first;
  io.d_tgt_off = &off;
  CHECK(edge_source_row(io, 3) == 13u && edge_target_row(io, 3) == 103ull);
  const uint32_t sidx[] = {7, 8, 9, 42}, tidx[] = {1, 2, 3, 77};
  io.src_idx = sidx;  // an index list wins over the offsets
  io.tgt_idx = tidx;
  CHECK(edge_source_row(io, 3) == 42u && edge_target_row(io, 3) == 77ull);
}

static void test_step_count() {
  const double dt = 0.1, full = 2.0;  // 20 steps of 0.1
  CHECK(edge_step_count(0.0, full, dt) == 0);  // 0 < 0 fails at once
  // fraction 1: current_time is the accumulated sum of 0.1, compared with 1.0 * 2.0; count it the same way here
  {
    double t = 0.0;
    int n = 0;
    while (t < 2.0) {
      t += 0.1;
      ++n;
    }
    CHECK(edge_step_count(1.0, full, dt) == n);
    CHECK(n == 20 || n == 21);  // (the accumulated sum decides, as in the reference)
  }
  // a fraction that ends between two steps: T_goal = 0.25 -> 0 < 0.25, 0.1 < 0.25, 0.2 < 0.25, then 0.3 (accumulated) stops
  CHECK(edge_step_count(0.125, full, dt) == 3);
  // exact in binary: dt = 0.25 -> fraction 1 takes 4 steps (1.0 < 1.0 fails), fraction 0.5 takes 2, 0.6 ends inside the third
  CHECK(edge_step_count(1.0, 1.0, 0.25) == 4);
  CHECK(edge_step_count(0.5, 1.0, 0.25) == 2);
  CHECK(edge_step_count(0.6, 1.0, 0.25) == 3);
  CHECK(edge_step_count(1e9, full, dt) == kMaxSteps);  // capped
}

static void test_pd_input() {
  CHECK(pd_input(2.0, 0.5, 10.0, 3.0, 1.0, 0.0, 4.0) == 2.0);    // 2 * 2 + 0.5 * (-4)
  CHECK(pd_input(2.0, 0.5, 1.5, 3.0, 1.0, 0.0, 4.0) == 1.5);     // saturates above
  CHECK(pd_input(2.0, 0.5, 1.5, -3.0, 1.0, 0.0, 4.0) == -1.5);   // 2 * (-4) - 2 = -10: saturates below
  CHECK(pd_input(2.0, 0.5, 2.0, 3.0, 1.0, 0.0, 4.0) == 2.0);     // exactly at the limit: unchanged
}

static void test_hyperbox() {
  CHECK(!hyperbox_out(-1.0, 1.0, 0.0));
  CHECK(!hyperbox_out(-1.0, 1.0, -1.0) && !hyperbox_out(-1.0, 1.0, 1.0));  // the bounds are inside
  CHECK(hyperbox_out(-1.0, 1.0, std::nextafter(1.0, 2.0)) && hyperbox_out(-1.0, 1.0, std::nextafter(-1.0, -2.0)));
  // reversed bounds (lower > upper), the reference's other branch: out when x > lower or x < upper
  CHECK(!hyperbox_out(1.0, -1.0, 0.0) && !hyperbox_out(1.0, -1.0, 1.0) && !hyperbox_out(1.0, -1.0, -1.0));
  CHECK(hyperbox_out(1.0, -1.0, std::nextafter(1.0, 2.0)));    // x > lower
  CHECK(hyperbox_out(1.0, -1.0, std::nextafter(-1.0, -2.0)));  // x < upper
  // equal bounds take that branch too: only the bound itself is inside
  CHECK(!hyperbox_out(0.5, 0.5, 0.5) && hyperbox_out(0.5, 0.5, 0.75) && hyperbox_out(0.5, 0.5, 0.25));
  CHECK(!hyperbox_out(-1.0, 1.0, std::numeric_limits<double>::quiet_NaN()));  // every comparison with NaN is false
}

static void test_rk4_stage() {
  // one inner step of x' = f, with the derivative values the four stages would see; against the unrolled expression
  const double h = 0.05, x0 = 0.7, dp[4] = {1.25, -0.5, 2.0, 0.375};
  double xe = x0, w = 0.0, k1 = 0.0, k2 = 0.0, k3 = 0.0;
  rk4_stage(0, h, dp[0], xe, w, k1, k2, k3);
  const double e_k1 = h * dp[0];
  CHECK(w == x0 && k1 == e_k1 && xe == x0 + 0.5 * e_k1);
  rk4_stage(1, h, dp[1], xe, w, k1, k2, k3);
  const double e_k2 = h * dp[1];
  CHECK(k2 == e_k2 && xe == x0 + 0.5 * e_k2);
  rk4_stage(2, h, dp[2], xe, w, k1, k2, k3);
  const double e_k3 = h * dp[2];
  CHECK(k3 == e_k3 && xe == x0 + e_k3);
  const double before = xe;
  rk4_stage(3, h, dp[3], xe, w, k1, k2, k3);
  CHECK(xe == before + ((((1.0 / 6.0) * e_k1 + (2.0 / 6.0) * e_k2) + (h / 6.0) * dp[3]) - (2.0 / 3.0) * e_k3));
  CHECK(w == x0);  // the start of the inner step is kept through the stages
}

static void test_accept() {
  const double bc[] = {0.0, 2.0};  // best_case[1] = 2
  const double tol = 0.25;
  // ---- steer: tol * best_case < traveled < 2 * best_case, both strict
  CHECK(edge_accept(EDGE_STEER_ACCEPT, 1.0, 9.0, 9.0, bc, 1, tol, kNoWalk) == 1);
  CHECK(edge_accept(EDGE_STEER_ACCEPT, 4.0, 9.0, 9.0, bc, 1, tol, kNoWalk) == 0);   // exactly 2 * best_case
  CHECK(edge_accept(EDGE_STEER_ACCEPT, std::nextafter(4.0, 0.0), 9.0, 9.0, bc, 1, tol, kNoWalk) == 1);
  CHECK(edge_accept(EDGE_STEER_ACCEPT, 0.5, 9.0, 9.0, bc, 1, tol, kNoWalk) == 0);   // exactly tol * best_case
  CHECK(edge_accept(EDGE_STEER_ACCEPT, std::nextafter(0.5, 1.0), 9.0, 9.0, bc, 1, tol, kNoWalk) == 1);
  CHECK(edge_accept(EDGE_STEER_ACCEPT, kInf, 9.0, 9.0, bc, 1, tol, kNoWalk) == 0);
  CHECK(edge_accept(EDGE_STEER_ACCEPT, kNaN, 9.0, 9.0, bc, 1, tol, kNoWalk) == 0);
  // no best_case: the distance to the target (n_ab = 8: accepted between 2 and 16)
  CHECK(edge_accept(EDGE_STEER_ACCEPT, 3.0, 8.0, 9.0, nullptr, 1, tol, kNoWalk) == 1);
  CHECK(edge_accept(EDGE_STEER_ACCEPT, 16.0, 8.0, 9.0, nullptr, 1, tol, kNoWalk) == 0);
  CHECK(edge_accept(EDGE_STEER_ACCEPT, 2.0, 8.0, 9.0, nullptr, 1, tol, kNoWalk) == 0);
  // ---- steer both: bit 1 only for a completed walk; a kernel without a walk does not know the mode
  CHECK(edge_accept(EDGE_STEER_BOTH, 1.0, 9.0, 9.0, bc, 1, tol, 0) == 1);
  CHECK(edge_accept(EDGE_STEER_BOTH, 1.0, 9.0, 9.0, bc, 1, tol, 1) == 3);
  CHECK(edge_accept(EDGE_STEER_BOTH, 4.0, 9.0, 9.0, bc, 1, tol, 1) == 2);
  CHECK(edge_accept(EDGE_STEER_BOTH, 4.0, 9.0, 9.0, bc, 1, tol, 0) == 0);
  CHECK(edge_accept(EDGE_STEER_ACCEPT, 1.0, 9.0, 9.0, bc, 1, tol, 1) == 1);  // bit 1 is EDGE_STEER_BOTH's alone
  CHECK(edge_accept(EDGE_STEER_BOTH, 1.0, 9.0, 9.0, bc, 1, tol, kNoWalk) == kNoAccept);
  // ---- connect: what is left to the target < tol * traveled (steer_tol carries the connection tolerance)
  CHECK(edge_accept(EDGE_CONNECT, 4.0, 9.0, 1.0, nullptr, 0, tol, kNoWalk) == 0);  // traveled at the tolerance: 1 < 0.25 * 4 fails
  CHECK(edge_accept(EDGE_CONNECT, std::nextafter(4.0, 5.0), 9.0, 1.0, nullptr, 0, tol, kNoWalk) == 1);
  CHECK(edge_accept(EDGE_CONNECT, kInf, 9.0, 1.0, nullptr, 0, tol, kNoWalk) == 0);
  CHECK(edge_accept(EDGE_CONNECT, kNaN, 9.0, 1.0, nullptr, 0, tol, kNoWalk) == 0);
  // ---- random walk: traveled > tol * best_case[e] (best_case carries the target distance)
  CHECK(edge_accept(EDGE_WALK_ACCEPT, 0.5, 9.0, 9.0, bc, 1, tol, kNoWalk) == 0);  // at the tolerance
  CHECK(edge_accept(EDGE_WALK_ACCEPT, std::nextafter(0.5, 1.0), 9.0, 9.0, bc, 1, tol, kNoWalk) == 1);
  CHECK(edge_accept(EDGE_WALK_ACCEPT, kInf, 9.0, 9.0, bc, 1, tol, kNoWalk) == 0);
  // ---- modes without an accept byte from the verdict
  CHECK(edge_accept(EDGE_PLAIN, 1.0, 9.0, 9.0, bc, 1, tol, 1) == kNoAccept);
  CHECK(edge_accept(EDGE_POINT, 1.0, 9.0, 9.0, bc, 1, tol, 1) == kNoAccept);
  CHECK(edge_accept(EDGE_GOAL_PROBE, 1.0, 9.0, 9.0, bc, 1, tol, 1) == kNoAccept);
  CHECK(edge_accept(7, 1.0, 9.0, 9.0, bc, 1, tol, 1) == kNoAccept);
  CHECK(edge_accept(-3, 1.0, 9.0, 9.0, bc, 1, tol, 1) == kNoAccept);
}

static void test_goal_probes() {
  // steerable space: reached when 5 % of the whole distance exceeds what is left, strictly
  const double n_ab = 8.0, edge = n_ab * 0.05;
  CHECK(goal_probe_steerable(n_ab, edge) == kInf);  // equality: not reached
  CHECK(goal_probe_steerable(n_ab, std::nextafter(edge, 0.0)) == n_ab);
  CHECK(goal_probe_steerable(n_ab, std::nextafter(edge, 1.0)) == kInf);
  CHECK(goal_probe_steerable(n_ab, kNaN) == kInf);
  // interpolated topology: reached when the walk ended on the target
  CHECK(goal_probe_interpolated(n_ab, DBL_EPSILON) == kInf);
  CHECK(goal_probe_interpolated(n_ab, std::nextafter(DBL_EPSILON, 0.0)) == n_ab);
  CHECK(goal_probe_interpolated(n_ab, 0.0) == n_ab);
  CHECK(goal_probe_interpolated(n_ab, 0.3) == kInf);  // the steerable rule would call this one reached
  CHECK(goal_probe_steerable(n_ab, 0.3) == n_ab);
}

int main() {
  test_gate();
  test_segment_of();
  test_rows();
  test_step_count();
  test_pd_input();
  test_hyperbox();
  test_rk4_stage();
  test_accept();
  test_goal_probes();
  if (g_failed) {
    std::printf("steer edge protocol: %d of %d checks FAILED\n", g_failed, g_checks);
    return 1;
  }
  std::printf("steer edge protocol ok: %d checks\n", g_checks);
  return 0;
}
