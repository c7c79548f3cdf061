// probe_reach.h -- goal probes that cannot reach the goal, settled without integrating them.
//
// A goal probe is a steered edge from a new vertex a towards the goal b whose only output is
// goal_probe_steerable(n_ab, n_rb) (steer_edge.h): n_ab if the edge's end state r lies within 5 % of n_ab of the goal,
// +inf otherwise.  An edge is n_steps RK4 steps of dt, and every state it passes at a step boundary lies in the state box,
// so its joint angles end within a travel bound T_j of the source's.  With reach_q = |T|_2:
//   n_rb >= |(r - b)_q| >= |(a - b)_q| - reach_q,
// and a vertex with |(a - b)_q| - reach_q >= 0.05 n_ab gets +inf whatever the integration does (probe_certified).
//
// probe_travel derives T from the chain, the box, u_max, dt and the step count alone, by the arithmetic of the f-eval
// (pair_state_derivative, propagate_pair.hip; oracle/reak_kte.hpp) with norms in place of vectors.  It is crude on purpose
// (six times what the edges of the 6-joint benchmark chain move) and refuses (+inf: nothing is ever certified) whatever
// it was not derived for.  No device builtin and no HIP header: a host compiler and a sanitizer read it on a machine
// without a GPU (tests/cpp/probe_reach_test.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#include "steer_edge.h"  // RKH_HD, hyperbox_out

namespace rkh {

constexpr int kReachMaxDof = 16;
constexpr double kReachMargin = 1.01;  // over the rounding of the kernels' own sums and of the Cholesky solve (a margin, not a measurement)
constexpr double kProbeReachShare = 0.05;  // goal_probe_steerable's share of n_ab
constexpr double kProbeReachSlack = 1.0 + 1e-9;  // over the rounding of n_ab and of the angle distance

struct ReachJoint {  // one {actuator, rotor inertia, revolute joint, rigid link, link inertia} group, base -> tip
  double axis[3];        // revolute_joint_3D::mAxis as given (not normalised by the f-eval's velocity and torque terms)
  double off_pos[3];     // the rigid link's offset
  double joint_inertia;  // rotor inertia (inertia_gen)
  double mass;
  double inertia[6];     // a11, a12, a13, a22, a23, a33 of the link's tensor
};

struct ReachChain {
  int n_dof = 0;
  bool serial = false;        // no branch, not planar
  bool all_revolute = false;  // no prismatic joint
  bool beam = false;          // the chain carries a flexible beam (its force grows with the deflection: no bound here)
  double base_acc[3] = {0.0, 0.0, 0.0};
  ReachJoint joints[kReachMaxDof];
};

struct ReachDyn {
  int n_dof = 0;
  int n_steps = 0;
  double dt = 0.0, u_max = 0.0;
  // the velocity bounds of the state box, per joint
  double v_lower[kReachMaxDof], v_upper[kReachMaxDof];
  bool single_inner = false;  // every step is one runge_kutta4_integrate_impl iteration (DynDev::inner[k] == 1, k < n_steps)
};

namespace reach_detail {
inline double norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
inline double frobenius_sym(const double* t) {  // a11, a12, a13, a22, a23, a33
  return std::sqrt(t[0] * t[0] + t[3] * t[3] + t[5] * t[5] + 2.0 * (t[1] * t[1] + t[2] * t[2] + t[4] * t[4]));
}
// positive semidefinite: every principal minor is >= 0
inline bool psd_sym(const double* t) {
  const double a = t[0], b = t[1], c = t[2], d = t[3], e = t[4], f = t[5];
  const double m12 = a * d - b * b, m13 = a * f - c * c, m23 = d * f - e * e;
  const double det = a * m23 - b * (b * f - c * e) + c * (b * e - c * d);
  return a >= 0.0 && d >= 0.0 && f >= 0.0 && m12 >= 0.0 && m13 >= 0.0 && m23 >= 0.0 && det >= 0.0;
}
}  // namespace reach_detail

// A(W): |qdd|_2 of the f-eval for any configuration, joint rates |qd_j| <= W[j] and inputs |u_j| <= u_max.
// The f-eval runs the chain with q_ddot = 0 (kte_nl_system.hpp:239-290); rotations keep norms.
//   base -> tip (revolute_doMotion, link_doMotion / frame_3D::addBefore):
//     Lambda_j = Lambda_{j-1} + Omega_{j-1} W_j |axis_j|       angular acceleration (the cross term; q_ddot = 0)
//     Omega_j  = Omega_{j-1} + W_j |axis_j|                    angular velocity
//     Gamma_j  = Gamma_{j-1} + (Omega_j^2 + Lambda_j) |off_j|  acceleration of the link's end frame, Gamma = |base_acc| at the base
//   inertia_3D::doForce:  |F| <= m_j Gamma_j,  |T| <= |I_j|_F (Lambda_j + Omega_j^2)
//   tip -> base (link_doForce, revolute_doForce, the actuator's reaction):
//     Phi_j   = Phi_{j+1} + m_j Gamma_j
//     Theta_j = Theta'_{j+1} + |I_j|_F (Lambda_j + Omega_j^2) + |off_j| Phi_j
//     |f_j|  <= Theta_j |axis_j| + u_max
//     Theta'_j = Theta_j (1 + |axis_j|^2) + u_max |axis_j|     what the joint passes on to its base
// The assembled matrix is sum T^t Mcm T + diag(joint_inertia) >= diag(joint_inertia) (mass_matrix_calc; link tensors
// positive semidefinite, masses >= 0), hence |qdd|_2 <= |f|_2 / min_j joint_inertia_j.
inline double reach_accel_bound(const ReachChain& c, const double* W, double u_max) {
  using namespace reach_detail;
  const int n = c.n_dof;
  double Lam[kReachMaxDof], Om[kReachMaxDof], Gam[kReachMaxDof];
  double lam = 0.0, om = 0.0, gam = norm3(c.base_acc);
  for (int j = 0; j < n; ++j) {
    const double ax = norm3(c.joints[j].axis);
    lam = lam + om * W[j] * ax;
    om = om + W[j] * ax;
    gam = gam + (om * om + lam) * norm3(c.joints[j].off_pos);
    Lam[j] = lam;
    Om[j] = om;
    Gam[j] = gam;
  }
  double phi = 0.0, theta_up = 0.0, f2 = 0.0, min_ji = INFINITY;
  for (int j = n - 1; j >= 0; --j) {
    const ReachJoint& J = c.joints[j];
    const double ax = norm3(J.axis);
    phi = phi + J.mass * Gam[j];
    const double theta = theta_up + frobenius_sym(J.inertia) * (Lam[j] + Om[j] * Om[j]) + norm3(J.off_pos) * phi;
    const double f = theta * ax + u_max;
    f2 += f * f;
    theta_up = theta * (1.0 + ax * ax) + u_max * ax;
    if (J.joint_inertia < min_ji) min_ji = J.joint_inertia;
  }
  return std::sqrt(f2) / min_ji;
}

// the conditions the bound was derived under
inline bool reach_applies(const ReachChain& c, const ReachDyn& d) {
  if (!c.serial || !c.all_revolute || c.beam) return false;
  if (c.n_dof < 1 || c.n_dof > kReachMaxDof || d.n_dof != c.n_dof || d.n_steps < 1) return false;
  if (!(d.dt > 0.0) || !std::isfinite(d.dt) || !std::isfinite(d.u_max) || !(d.u_max >= 0.0)) return false;
  // a sub-step's start state is not box-checked: one runge_kutta4_integrate_impl iteration per step only
  if (!d.single_inner) return false;
  for (int j = 0; j < c.n_dof; ++j) {
    const ReachJoint& J = c.joints[j];
    if (!(J.joint_inertia > 0.0) || !(J.mass >= 0.0) || !reach_detail::psd_sym(J.inertia)) return false;
    if (!(d.v_lower[j] < d.v_upper[j])) return false;  // (a wrapped coordinate is no bound)
  }
  return true;
}

// T[j] >= |q_j(end) - q_j(source)| of every steered edge (any target, any mapping): n_steps RK4 steps from states in the
// box.  Every mapping clamps |u_j| <= u_max (pd_input, steer_edge.h:128-133: the one-wave and planar kernels and the edge
// walks; propagate_pair.hip:1064-1069 and :1325-1330: the two-lanes kernels).  V_j = the larger magnitude of the velocity
// bounds; the stage velocities of one step (rk4_stage) are bounded by
//   W1 = V,  W2 = V + dt/2 A(W1),  W3 = V + dt/2 A(W2),  W4 = V + dt A(W3)
// and the angle update dt/6 (qd1 + 2 qd2 + 2 qd3 + qd4) by dt W4_j.  T_j = n_steps dt W4_j kReachMargin.
// Returns false, and +inf in every T[j], where reach_applies does not hold or the result is not finite.
// W4 of a chain and space reach_applies holds for
inline void reach_stage_rates(const ReachChain& c, const ReachDyn& d, double* W) {
  const int n = c.n_dof;
  double V[kReachMaxDof];
  for (int j = 0; j < n; ++j) V[j] = std::fmax(std::fabs(d.v_lower[j]), std::fabs(d.v_upper[j]));
  for (int j = 0; j < n; ++j) W[j] = V[j];
  const double h[3] = {0.5 * d.dt, 0.5 * d.dt, d.dt};
  for (int s = 0; s < 3; ++s) {
    const double A = reach_accel_bound(c, W, d.u_max);
    for (int j = 0; j < n; ++j) W[j] = V[j] + h[s] * A;
  }
}

inline bool probe_travel(const ReachChain& c, const ReachDyn& d, double* T) {
  for (int j = 0; j < kReachMaxDof; ++j) T[j] = INFINITY;
  if (!reach_applies(c, d)) return false;
  const int n = c.n_dof;
  double W[kReachMaxDof];
  reach_stage_rates(c, d, W);
  double out[kReachMaxDof];
  for (int j = 0; j < n; ++j) {
    out[j] = double(d.n_steps) * d.dt * W[j] * kReachMargin;
    if (!std::isfinite(out[j])) return false;
  }
  for (int j = 0; j < n; ++j) T[j] = out[j];
  return true;
}

// |T|_2 over the chain's joints; +inf: no certificate
inline double probe_reach_norm(const double* T, int n_dof) {
  double s = 0.0;
  for (int j = 0; j < n_dof; ++j) s += T[j] * T[j];
  return std::sqrt(s);
}

// The probe of vertex a (state (q0, qd0, q1, qd1, ...), D components) towards b gives +inf for certain: a's rates lie in
// the box (v_lower / v_upper per joint) and its angles are farther from b's than reach_q + 5 % of n_ab.  n_ab: the
// kernels' left-to-right sum over all D components.  False for reach_q = +inf and for anything not finite.
RKH_HD bool probe_certified(const double* a, const double* b, int D, double reach_q, const double* v_lower,
                            const double* v_upper) {
  double s_all = 0.0, s_q = 0.0;
  for (int d = 0; d < D; ++d) {
    const double df = a[d] - b[d];
    s_all += df * df;
    if ((d & 1) == 0) s_q += df * df;
    else if (hyperbox_out(v_lower[d >> 1], v_upper[d >> 1], a[d])) return false;
  }
  const double n_ab = std::sqrt(s_all);
  if (!(n_ab < INFINITY)) return false;
  return std::sqrt(s_q) - reach_q >= kProbeReachShare * n_ab * kProbeReachSlack;
}

}  // namespace rkh
