// probe_reach_test.cpp -- host-only check of the goal-probe certificate (reak_amd/csrc/probe_reach.h) and of the probe
// list's granule rule (reak_amd/csrc/round_plan.h).  Built with -fsanitize=address,undefined and run directly
// (tests/test_probe_reach_cpu.py).  Without arguments: hand-worked values of a one-joint chain, +inf for every refusal
// condition, the predicate one ulp either side of equality, the list through append / drop / leftover / probed_n.
// With `bound FILE`: the travel bound of the chain and space FILE describes (the Python test compares it with the
// oracle): n_dof, n_steps, dt, u_max, base_acc[3]; per joint axis[3] off_pos[3] joint_inertia mass inertia[6] v_lower
// v_upper; prints T, reach_q, W4 and A(W4).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "probe_reach.h"
#include "round_plan.h"

using namespace rkh;

static int g_checks = 0;

#define CHECK(cond)                                                       \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

static bool close_rel(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fmax(std::fabs(a), std::fabs(b)); }

// ---- a one-joint chain, worked by hand --------------------------------------------------------------------------------
// axis z (unit), link offset 0.5 along x, mass 2, tensor diag(0.1, 0.2, 0.3) (|I|_F = sqrt(0.14)), rotor inertia 0.5,
// gravity 9.81 as base acceleration, |qd| <= 2, u_max = 3.  At a rate bound w:
//   Lambda = 0, Omega = w, Gamma = 9.81 + 0.5 w^2, Phi = 2 Gamma, Theta = sqrt(0.14) w^2 + 0.5 Phi,
//   |f| <= Theta + 3, A(w) = |f| / 0.5
static ReachChain one_joint() {
  ReachChain c;
  c.n_dof = 1;
  c.serial = true;
  c.all_revolute = true;
  c.beam = false;
  c.base_acc[2] = 9.81;
  ReachJoint& J = c.joints[0];
  std::memset(&J, 0, sizeof(J));
  J.axis[2] = 1.0;
  J.off_pos[0] = 0.5;
  J.joint_inertia = 0.5;
  J.mass = 2.0;
  J.inertia[0] = 0.1;
  J.inertia[3] = 0.2;
  J.inertia[5] = 0.3;
  return c;
}
static ReachDyn one_joint_dyn() {
  ReachDyn d;
  d.n_dof = 1;
  d.n_steps = 20;
  d.dt = 1e-3;
  d.u_max = 3.0;
  for (int j = 0; j < kReachMaxDof; ++j) d.v_lower[j] = d.v_upper[j] = 0.0;
  d.v_lower[0] = -2.0;
  d.v_upper[0] = 1.5;  // V = the larger magnitude
  d.single_inner = true;
  return d;
}
static double hand_A(double w) {
  const double gamma = 9.81 + 0.5 * w * w;
  const double theta = std::sqrt(0.14) * w * w + 0.5 * (2.0 * gamma);
  return (theta + 3.0) / 0.5;
}

static void hand_worked() {
  const ReachChain c = one_joint();
  const ReachDyn d = one_joint_dyn();
  double W[kReachMaxDof] = {2.0};
  CHECK(close_rel(reach_accel_bound(c, W, 3.0), hand_A(2.0), 1e-14));
  CHECK(close_rel(hand_A(2.0), (4.0 * std::sqrt(0.14) + 11.81 + 3.0) / 0.5, 1e-14));
  // a non-unit axis scales the rate terms and the projection: axis (0, 0, 2) at w is Omega = 2 w, |f| <= 2 Theta + u_max
  {
    ReachChain c2 = c;
    c2.joints[0].axis[2] = 2.0;
    const double om = 4.0, gamma = 9.81 + 0.5 * om * om, theta = std::sqrt(0.14) * om * om + 0.5 * (2.0 * gamma);
    CHECK(close_rel(reach_accel_bound(c2, W, 3.0), (2.0 * theta + 3.0) / 0.5, 1e-14));
  }
  const double w2 = 2.0 + 0.5e-3 * hand_A(2.0), w3 = 2.0 + 0.5e-3 * hand_A(w2), w4 = 2.0 + 1e-3 * hand_A(w3);
  double W4[kReachMaxDof];
  reach_stage_rates(c, d, W4);
  CHECK(close_rel(W4[0], w4, 1e-14));
  double T[kReachMaxDof];
  CHECK(probe_travel(c, d, T));
  CHECK(close_rel(T[0], 20.0 * 1e-3 * w4 * 1.01, 1e-14));
  CHECK(T[0] > 20.0 * 1e-3 * 2.0 && T[0] < 0.05);  // a little more than n_steps dt V
  for (int j = 1; j < kReachMaxDof; ++j) CHECK(std::isinf(T[j]));
  CHECK(probe_reach_norm(T, 1) == T[0]);
  // two equal joints in a row: the second one's terms carry the first one's rate
  {
    ReachChain c2 = c;
    c2.n_dof = 2;
    c2.joints[1] = c2.joints[0];
    ReachDyn d2 = d;
    d2.n_dof = 2;
    d2.v_lower[1] = -2.0;
    d2.v_upper[1] = 2.0;
    double W2[kReachMaxDof] = {2.0, 2.0};
    // base -> tip: Lam = (0, 4), Om = (2, 4), Gam = (11.81, 11.81 + (16 + 4) 0.5 = 21.81)
    // tip -> base: Phi = (2 21.81 + 2 11.81, 2 21.81); Theta_1 = sqrt(.14) 20 + 0.5 43.62, f_1 = Theta_1 + 3,
    // Theta'_1 = 2 Theta_1 + 3; Theta_0 = Theta'_1 + sqrt(.14) 4 + 0.5 67.24, f_0 = Theta_0 + 3
    const double th1 = std::sqrt(0.14) * 20.0 + 0.5 * 43.62, f1 = th1 + 3.0;
    const double th0 = (2.0 * th1 + 3.0) + std::sqrt(0.14) * 4.0 + 0.5 * 67.24, f0 = th0 + 3.0;
    CHECK(close_rel(reach_accel_bound(c2, W2, 3.0), std::sqrt(f0 * f0 + f1 * f1) / 0.5, 1e-13));
    CHECK(probe_travel(c2, d2, T));
    CHECK(T[0] == T[1] && std::isinf(T[2]));
    CHECK(close_rel(probe_reach_norm(T, 2), T[0] * std::sqrt(2.0), 1e-14));
  }
}

// ---- every refusal condition gives +inf --------------------------------------------------------------------------------
static void refused(const ReachChain& c, const ReachDyn& d) {
  double T[kReachMaxDof];
  CHECK(!probe_travel(c, d, T));
  for (int j = 0; j < kReachMaxDof; ++j) CHECK(std::isinf(T[j]) && T[j] > 0.0);
  CHECK(std::isinf(probe_reach_norm(T, c.n_dof > 0 && c.n_dof <= kReachMaxDof ? c.n_dof : 1)));
}
static void refusals() {
  const ReachChain c0 = one_joint();
  const ReachDyn d0 = one_joint_dyn();
  double T[kReachMaxDof];
  CHECK(probe_travel(c0, d0, T));
  { ReachChain c = c0; c.serial = false; refused(c, d0); }
  { ReachChain c = c0; c.all_revolute = false; refused(c, d0); }
  { ReachChain c = c0; c.beam = true; refused(c, d0); }
  { ReachChain c = c0; c.joints[0].joint_inertia = 0.0; refused(c, d0); }
  { ReachChain c = c0; c.joints[0].joint_inertia = -1.0; refused(c, d0); }
  { ReachChain c = c0; c.joints[0].joint_inertia = NAN; refused(c, d0); }
  { ReachChain c = c0; c.joints[0].inertia[0] = -0.1; refused(c, d0); }                             // a negative diagonal entry
  { ReachChain c = c0; c.joints[0].inertia[1] = 0.2; refused(c, d0); }                              // a12^2 > a11 a22
  { ReachChain c = c0; c.joints[0].inertia[0] = c.joints[0].inertia[3] = c.joints[0].inertia[5] = 1.0;
    c.joints[0].inertia[1] = c.joints[0].inertia[2] = c.joints[0].inertia[4] = -0.9; refused(c, d0); }  // only the determinant is negative
  { ReachChain c = c0; c.joints[0].mass = -1.0; refused(c, d0); }
  { ReachDyn d = d0; d.v_lower[0] = 2.0; d.v_upper[0] = -2.0; refused(c0, d); }                      // a wrapped rate
  { ReachDyn d = d0; d.v_lower[0] = d.v_upper[0] = 1.0; refused(c0, d); }
  { ReachDyn d = d0; d.u_max = INFINITY; refused(c0, d); }
  { ReachDyn d = d0; d.u_max = NAN; refused(c0, d); }
  { ReachDyn d = d0; d.v_upper[0] = INFINITY; refused(c0, d); }                                      // the result is not finite
  { ReachDyn d = d0; d.v_upper[0] = 1e200; refused(c0, d); }                                         // ... overflows on the way
  { ReachDyn d = d0; d.single_inner = false; refused(c0, d); }
  { ReachDyn d = d0; d.n_steps = 0; refused(c0, d); }
  { ReachDyn d = d0; d.n_dof = 2; refused(c0, d); }
  { ReachChain c = c0; c.n_dof = 0; ReachDyn d = d0; d.n_dof = 0; refused(c, d); }
  { ReachChain c = c0; c.n_dof = kReachMaxDof + 1; ReachDyn d = d0; d.n_dof = kReachMaxDof + 1; refused(c, d); }
  // a positive semidefinite tensor with a zero eigenvalue and a zero mass are fine
  { ReachChain c = c0; c.joints[0].inertia[0] = c.joints[0].inertia[3] = c.joints[0].inertia[1] = 0.1; c.joints[0].mass = 0.0;
    CHECK(probe_travel(c, d0, T)); }
}

// ---- the predicate at its edge ------------------------------------------------------------------------------------------
static void predicate() {
  const double lo[1] = {-2.0}, hi[1] = {2.0};
  // equal rates: n_ab = |dq| = 2 exactly; certified iff 2 - reach_q >= 0.05 * 2 * (1 + 1e-9)
  const double a[2] = {2.5, 0.25}, b[2] = {0.5, 0.25};
  const double rhs = 0.05 * 2.0 * (1.0 + 1e-9);
  // 2 - r is exact for r in [1, 2]; the largest r with 2 - r >= rhs, found in extended precision (2 - rhs needs 58 bits)
  const long double r_eq = 2.0L - (long double)rhs;
  double r_lo = double(r_eq);
  if ((long double)r_lo > r_eq) r_lo = std::nextafter(r_lo, 0.0);
  const double r_hi = std::nextafter(r_lo, INFINITY);
  CHECK((long double)r_lo <= r_eq && (long double)r_hi > r_eq);
  CHECK(probe_certified(a, b, 2, r_lo, lo, hi));
  CHECK(!probe_certified(a, b, 2, r_hi, lo, hi));
  CHECK(probe_certified(a, b, 2, 0.0, lo, hi));
  CHECK(!probe_certified(a, b, 2, 2.0, lo, hi));
  // equality itself certifies: |dq| = 0.5, reach_q = 0.25, and n_ab grown through the rates until
  // 0.05 n_ab (1 + 1e-9) crosses 0.25 (n_ab near 5: dv near sqrt(24.75), outside no box since b's rate is the goal's)
  {
    const double lo5[1] = {-10.0}, hi5[1] = {10.0};
    const double a5[2] = {0.5, 0.0};
    auto cert = [&](double v) {
      const double b5[2] = {0.0, v};
      return probe_certified(a5, b5, 2, 0.25, lo5, hi5);
    };
    double in = 4.9, out = 5.0;
    CHECK(cert(in) && !cert(out));
    while (std::nextafter(in, out) < out) {  // bisect down to neighbouring doubles
      const double mid = in + 0.5 * (out - in);
      if (cert(mid)) in = mid;
      else out = mid;
    }
    // the last certified rate satisfies the inequality as probe_reach.h states it, the next double does not
    CHECK(0.5 - 0.25 >= 0.05 * std::sqrt(0.25 + in * in) * (1.0 + 1e-9));
    CHECK(!(0.5 - 0.25 >= 0.05 * std::sqrt(0.25 + out * out) * (1.0 + 1e-9)));
    CHECK(std::fabs(in - std::sqrt(24.75)) < 1e-6);
  }
  // a rate outside the box: never certified, however far away; on the bound itself it is inside
  {
    const double far_a[2] = {3.0, 2.0000000000000004}, far_b[2] = {-3.0, 0.0}, on_a[2] = {3.0, 2.0}, low_a[2] = {3.0, -2.0000000000000004};
    CHECK(!probe_certified(far_a, far_b, 2, 0.1, lo, hi));
    CHECK(!probe_certified(low_a, far_b, 2, 0.1, lo, hi));
    CHECK(probe_certified(on_a, far_b, 2, 0.1, lo, hi));
  }
  // no certificate, and values that are no numbers
  CHECK(!probe_certified(a, b, 2, INFINITY, lo, hi));
  CHECK(!probe_certified(a, b, 2, NAN, lo, hi));
  {
    const double nan_a[2] = {NAN, 0.0}, inf_a[2] = {INFINITY, 0.0};
    CHECK(!probe_certified(nan_a, b, 2, 0.1, lo, hi));
    CHECK(!probe_certified(inf_a, b, 2, 0.1, lo, hi));
  }
  // two joints: only the angles count on the left, all four components in n_ab
  {
    const double lo2[2] = {-2.0, -2.0}, hi2[2] = {2.0, 2.0};
    const double a2[4] = {3.0, 1.0, 4.0, -1.0}, b2[4] = {0.0, -1.0, 0.0, 1.0};  // |dq| = 5, n_ab = sqrt(33)
    const double r = 5.0 - 0.05 * std::sqrt(33.0) * (1.0 + 1e-9);
    CHECK(probe_certified(a2, b2, 4, r - 1e-12, lo2, hi2));
    CHECK(!probe_certified(a2, b2, 4, r + 1e-12, lo2, hi2));
  }
}

// ---- the list and the granule rule ----------------------------------------------------------------------------------------
// commit_kernel's steps on a problem's list (planner.hip), on the host
struct ListModel {
  std::vector<uint32_t> list;
  uint32_t n_new = 0;  // entries the next launch runs
  uint32_t n = 1;      // vertices (the root has no probe)
  uint32_t probed_n = 1;
  uint64_t run = 0, certified = 0;
  // a round commits `added` vertices, open[k] says whether vertex n + k's probe stays open
  void commit(const std::vector<bool>& open, uint32_t granule) {
    const uint32_t ran = n_new, waited = uint32_t(list.size()) - ran;
    list.erase(list.begin(), list.begin() + ran);  // drop what the launch ran, the leftover moves to the front
    for (size_t k = 0; k < open.size(); ++k) {
      if (open[k]) list.push_back(n + uint32_t(k));
      else ++certified;
    }
    n += uint32_t(open.size());
    run += ran;
    n_new = probe_ride_count(uint32_t(list.size()), waited, granule);
    probed_n = probe_probed_n(list.data(), uint32_t(list.size()), n);
  }
};

static void list_rule() {
  CHECK(probe_ride_count(0, 0, 32) == 0);
  CHECK(probe_ride_count(31, 0, 32) == 0);
  CHECK(probe_ride_count(32, 0, 32) == 32);
  CHECK(probe_ride_count(40, 0, 32) == 32);
  CHECK(probe_ride_count(13, 8, 32) == 8);    // the leftover rides after one round, the new ones wait
  CHECK(probe_ride_count(36, 6, 32) == 32);   // whole granules cover the leftover
  CHECK(probe_ride_count(64, 31, 32) == 64);
  CHECK(probe_ride_count(5, 5, 32) == 5);
  CHECK(probe_ride_count(7, 0, 1) == 7 && probe_ride_count(0, 0, 1) == 0);  // granule 1: every open probe rides
  const uint32_t some[3] = {17, 20, 21};
  CHECK(probe_probed_n(some, 3, 30) == 17 && probe_probed_n(some, 0, 30) == 30);

  ListModel m;
  m.commit(std::vector<bool>(40, true), 32);  // vertices 1 .. 40, all open
  CHECK(m.list.size() == 40 && m.n_new == 32 && m.probed_n == 1 && m.n == 41);
  std::vector<bool> five(5, true);
  m.commit(five, 32);  // 33 .. 40 are left over, 41 .. 45 join them
  CHECK(m.list.size() == 13 && m.list[0] == 33 && m.list[8] == 41 && m.n_new == 8 && m.probed_n == 33 && m.run == 32);
  m.commit({}, 32);  // the leftover rode; the five have now waited a round
  CHECK(m.list.size() == 5 && m.list[0] == 41 && m.n_new == 5 && m.probed_n == 41 && m.run == 40);
  m.commit({false, false, true}, 32);  // 46 and 47 are settled at commit, 48 stays open
  CHECK(m.list.size() == 1 && m.list[0] == 48 && m.n_new == 0 && m.probed_n == 48 && m.certified == 2 && m.run == 45);
  m.commit({false}, 32);
  CHECK(m.list.size() == 1 && m.n_new == 1 && m.probed_n == 48 && m.n == 50);
  m.commit({}, 32);
  CHECK(m.list.empty() && m.n_new == 0 && m.probed_n == 50 && m.run == 46 && m.certified == 3);
  CHECK(m.run + m.certified + m.list.size() == m.n - 1);

  // any sequence: fewer than the granule stay behind, nothing waits for more than one launch, the list stays within
  // b_max + granule - 1 entries and in vertex order, and probed_n never passes an open vertex
  for (uint32_t granule : {1u, 32u}) {
    for (uint32_t b_max : {8u, 384u}) {
      ListModel r;
      uint64_t s = 12345u + granule + b_max;
      std::vector<uint32_t> waiting;  // the vertices the last launch left behind
      for (int round = 0; round < 400; ++round) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t added = uint32_t((s >> 33) % (b_max + 1u));
        std::vector<bool> open(added);
        for (uint32_t k = 0; k < added; ++k) {
          s = s * 6364136223846793005ull + 1442695040888963407ull;
          open[k] = ((s >> 40) % 100u) < (round % 3 == 0 ? 90u : 3u);  // rounds near the goal, rounds far from it
        }
        r.commit(open, granule);
        CHECK(r.list.size() < size_t(b_max) + granule);
        CHECK(r.list.size() - r.n_new < granule);
        for (size_t k = 1; k < r.list.size(); ++k) CHECK(r.list[k - 1] < r.list[k]);
        for (uint32_t v : waiting) {  // what waited through the last launch rides in the next one
          size_t at = 0;
          while (at < r.list.size() && r.list[at] != v) ++at;
          CHECK(at < r.n_new);
        }
        waiting.assign(r.list.begin() + r.n_new, r.list.end());
        CHECK(r.probed_n == (r.list.empty() ? r.n : r.list[0]));
        CHECK(r.run + r.certified + r.list.size() == r.n - 1);
        if (granule == 1u) CHECK(r.n_new == r.list.size());
      }
    }
  }
}

// ---- `bound FILE` --------------------------------------------------------------------------------------------------------
static int print_bound(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return 2;
  ReachChain c;
  ReachDyn d;
  bool ok = std::fscanf(f, "%d %d %lf %lf %lf %lf %lf", &c.n_dof, &d.n_steps, &d.dt, &d.u_max, &c.base_acc[0], &c.base_acc[1],
                        &c.base_acc[2]) == 7;
  ok = ok && c.n_dof >= 1 && c.n_dof <= kReachMaxDof;
  d.n_dof = c.n_dof;
  c.serial = c.all_revolute = true;
  c.beam = false;
  d.single_inner = true;
  for (int j = 0; j < kReachMaxDof; ++j) d.v_lower[j] = d.v_upper[j] = 0.0;
  for (int j = 0; ok && j < c.n_dof; ++j) {
    ReachJoint& J = c.joints[j];
    int got = 0;
    for (int k = 0; k < 3; ++k) got += std::fscanf(f, "%lf", &J.axis[k]);
    for (int k = 0; k < 3; ++k) got += std::fscanf(f, "%lf", &J.off_pos[k]);
    got += std::fscanf(f, "%lf %lf", &J.joint_inertia, &J.mass);
    for (int k = 0; k < 6; ++k) got += std::fscanf(f, "%lf", &J.inertia[k]);
    got += std::fscanf(f, "%lf %lf", &d.v_lower[j], &d.v_upper[j]);
    ok = got == 16;
  }
  std::fclose(f);
  if (!ok) return 2;
  double T[kReachMaxDof], W[kReachMaxDof];
  if (!probe_travel(c, d, T)) {
    std::printf("refused\n");
    return 0;
  }
  reach_stage_rates(c, d, W);
  std::printf("T");
  for (int j = 0; j < c.n_dof; ++j) std::printf(" %.17g", T[j]);
  std::printf("\nreach_q %.17g\nW4", probe_reach_norm(T, c.n_dof));
  for (int j = 0; j < c.n_dof; ++j) std::printf(" %.17g", W[j]);
  std::printf("\nA4 %.17g\n", reach_accel_bound(c, W, d.u_max));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && std::strcmp(argv[1], "bound") == 0) return print_bound(argv[2]);
  hand_worked();
  refusals();
  predicate();
  list_rule();
  std::printf("probe reach ok: %d checks\n", g_checks);
  return 0;
}
