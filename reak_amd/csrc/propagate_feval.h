// propagate_feval.h -- HIP only: hipcc compiles it into the propagate*.hip units, no host compiler reads it (unlike the
// *_device.h headers).  x' = f(x,u) of a KTE chain: the phases, their one-wave form (state_derivative) and their
// two-waves form (state_derivative_duo).
#pragma once
#include "propagate_lds.h"

namespace rkh {

// axis_angle::getRotMat (rotations_3D.hpp:2160-2180) from cos/sin of the angle and the unit axis
RKH_DI m33 axis_angle_rotmat(double ca, double sa, d3 ax) {
  const double omc = 1.0 - ca;
  const double t11 = ca + omc * ax.x * ax.x, t22 = ca + omc * ax.y * ax.y, t33 = ca + omc * ax.z * ax.z;
  const double t12 = omc * ax.x * ax.y, t13 = omc * ax.x * ax.z, t23 = omc * ax.y * ax.z;
  const double t01 = sa * ax.x, t02 = sa * ax.y, t03 = sa * ax.z;
  return m33{t11, t12 - t03, t13 + t02, t12 + t03, t22, t23 - t01, t13 - t02, t23 + t01, t33};
}

// ---- the phases of x' = f(x,u) that its one-wave form (state_derivative) and its two-waves form (state_derivative_duo)
// share.  `sync` orders the LDS traffic of the lanes that run the phase: a block barrier where the whole block does, a
// wave-local fence where one wave of two does (wave_sync).

// Jacobian columns, one lane per (body b, coord c <= b): get_jac_relative_to (motion_jacobians.hpp:238-251) with
// f2 = (~F_c) * F_b (frame_3D.hpp:184-189,222-238,368-382)
template <int N, int GL, bool PRISM>
__device__ __forceinline__ void feval_jacobian_columns(const SceneDev* __restrict__ sc_beam, const JointLds* __restrict__ jl,
                                                       GroupWs<N>& ws, int gl) {
  for (int p = gl; p < N * (N + 1) / 2; p += GL) {
    int b = 0, c = p;  // unrank p -> (b, c), c <= b
    while (c > b) {
      c -= b + 1;
      ++b;
    }
    if (c < sc_beam->branch_first[b]) continue;  // joint c is not upstream of body b (another branch)
    const d3 cp = ld3(ws.Epos[c]);
    const d4 cq = ld4(ws.Equat[c]);
    const d3 bp = ld3(ws.Lpos[b]);
    const d4 bq = ld4(ws.Lquat[b]);
    const m33 R = rotmat(cq);
    const d4 iq = qinv(cq);
    const d3 ipos = mulT(-cp, R);
    const m33 Ri = rotmat(iq);
    const d3 f2pos = ipos + mul(Ri, bp);
    const d4 f2q = qmul(iq, bq);
    const m33 Rf = rotmat(f2q);
    const d3 axis = ld3(jl[c].axis);
    d3 wt = mulT(axis, Rf);
    d3 vt = mulT(cross(axis, f2pos), Rf);
    if (PRISM && ((sc_beam->prismatic_mask >> c) & 1u)) {  // prismatic_joint_3D: qd_vel = mAxis, qd_avel = 0
      vt = mulT(axis, Rf);
      wt = mk3(0, 0, 0);
    }
    st3(ws.Tcm[b][c], vt);
    st3(ws.Tcm[b][c] + 3, wt);
  }
}

// Mf = Tcm^T (Mcm Tcm), one lane per entry (i,j), summation order of mat_alg_symmetric.hpp:551-566 (Mcm*Tcm) and
// mat_operators.hpp:104-114 (dense product); then M = mat<symmetric>(Mf).
// (the loop is uniform -- lanes without an entry in the last pass recompute the last entry and do not store -- and the
// v_readlane reads of the chain parameters sit outside the per-lane condition: a readlane must not pick a lane that
// was masked off when a run-time-indexed copy of the parameter registers was made)
template <int N, int GL, class Sync>
__device__ __forceinline__ void feval_mass_matrix(const SceneDev* __restrict__ sc_beam, const CPack<N>& cp,
                                                  const JointLds* __restrict__ jl, GroupWs<N>& ws, int gl, Sync sync) {
  for (int e0 = 0; e0 < N * N; e0 += GL) {
    const bool e_valid = e0 + gl < N * N;
    const int e = e_valid ? e0 + gl : N * N - 1;
    const int i = e / N, jx = e % N;
    double s = 0.0;
    if (i == jx) s = s + jl[i].joint_inertia;  // inertia_gen rows: Tcm = 1, Mcm = rotor inertia
#pragma unroll
    for (int b = 0; b < N; ++b) {
      const int bb = b * 32;
      const double mass = cget(cp, bb + JC_MASS);
      const double inertia[6] = {cget(cp, bb + JC_INER), cget(cp, bb + JC_INER + 1), cget(cp, bb + JC_INER + 2),
                                 cget(cp, bb + JC_INER + 3), cget(cp, bb + JC_INER + 4), cget(cp, bb + JC_INER + 5)};
      const int first_b = sc_beam->branch_first[b];
      if (b >= i && b >= jx && i >= first_b && jx >= first_b) {
        const double* Ti = ws.Tcm[b][i];
        const double* Tj = ws.Tcm[b][jx];
        s = s + Ti[0] * (mass * Tj[0]);
        s = s + Ti[1] * (mass * Tj[1]);
        s = s + Ti[2] * (mass * Tj[2]);
        const d3 P = sym_mul(inertia, mk3(Tj[3], Tj[4], Tj[5]));
        s = s + Ti[3] * P.x;
        s = s + Ti[4] * P.y;
        s = s + Ti[5] * P.z;
      }
    }
    if (e_valid) ws.Mf[i][jx] = s;
  }
  sync();
  // mat<symmetric>(general): 0.5 * (M(j,i) + M(i,j)), j < i  (mat_alg_symmetric.hpp:183-187)
  for (int e = gl; e < N * N; e += GL) {
    const int i = e / N, jx = e % N;
    const int lo = i < jx ? i : jx, hi = i < jx ? jx : i;
    ws.M[i][jx] = (i == jx) ? ws.Mf[i][i] : 0.5 * (ws.Mf[lo][hi] + ws.Mf[hi][lo]);
  }
  sync();
}

// linsolve_Cholesky (mat_cholesky.hpp:546-554): lane i owns row i (Lrow); every L(i,j) is formed by the reference's
// operation sequence (A(i,j), minus L(i,k) L(j,k) for k ascending, divided by L(j,j)).  The factor overwrites ws.M.
// Returns whether a pivot was below 1e-8.
template <int N, class Sync>
__device__ __forceinline__ bool feval_cholesky_factor(GroupWs<N>& ws, int gl, double (&Lrow)[N], Sync sync) {
  const int row = gl < N ? gl : N - 1;
  bool sing = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    // pivot of column j, computed by every lane from row j (already final in LDS for k < j)
    double dgl = ws.M[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) {
      const double ljk = ws.M[j][k];
      dgl = dgl - ljk * ljk;
    }
    if (dgl < 1e-8) sing = true;
    const double ljj = sqrt(dgl);
    double v = ws.M[row][j];
#pragma unroll
    for (int k = 0; k < j; ++k) v = v - Lrow[k] * ws.M[j][k];
    v = v / ljj;
    Lrow[j] = (row == j) ? ljj : v;
    if (gl < N && row >= j) ws.M[row][j] = Lrow[j];
    sync();
  }
  return sing;
}

// backsub_Cholesky_impl (mat_cholesky.hpp:160-178): L y = f, then L^T x = y.  f: this lane's row of the right-hand side;
// returns its row of the solution (the rows of an edge sit in the lanes gb .. gb + N - 1 of the wave)
template <int N>
__device__ __forceinline__ double feval_backsub(const GroupWs<N>& ws, int gl, int gb, const double (&Lrow)[N], double f) {
  const int row = gl < N ? gl : N - 1;
  double diag = 1.0;
#pragma unroll
  for (int k = 0; k < N; ++k) diag = (row == k) ? Lrow[k] : diag;
  double accv = f;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double yk = __shfl(accv / diag, gb + k, 64);
    if (row == k) accv = yk;
    else if (row > k) accv = accv - Lrow[k] * yk;
  }
#pragma unroll
  for (int k = N - 1; k >= 0; --k) {
    const double xk = __shfl(accv / diag, gb + k, 64);
    if (row == k) accv = xk;
    else if (row < k) accv = accv - ws.M[k][row] * xk;
  }
  return accv;
}

// x' = f(x,u) for the lane group's edge.  ws.x / ws.u hold the state and the input (already staged).
// Returns dp for lane gl (< 2N); sets *singular if a Cholesky pivot is < 1e-8.
// PRISM: the scene may hold prismatic joints (SceneDev::prismatic_mask; serial chains without a beam); false compiles the
// revolute-only code unchanged.
template <int N, int GL, bool PRISM = false>
__device__ double state_derivative(const SceneDev* __restrict__ sc_beam, const CPack<N>& cp,
                                   const JointLds* __restrict__ jl, const double* __restrict__ base, GroupWs<N>& ws,
                                   double* __restrict__ sink, int gl, int gb, bool* singular,
                                   unsigned long long* stamps = nullptr) {
  constexpr int D = 2 * N;
  // diagnostic builds only (rkh_diag_feval_cycles): per-phase s_memtime deltas; null in the product path
#define RKH_STAMP(i)                                        \
  if (stamps) {                                             \
    const unsigned long long t_now = __builtin_readcyclecounter(); \
    stamps[i] += t_now - t_prev;                            \
    t_prev = t_now;                                         \
  }
  unsigned long long t_prev = stamps ? __builtin_readcyclecounter() : 0ull;
  const bool lead = (gl == 0);  // the group leader's stores land in ws, everyone else's in its private sink
  // ---- sin/cos, lane-parallel: lane 2j -> half angle, lane 2j+1 -> full angle
  if (gl < D) {
    const double q = ws.x[gl & ~1];
    double sn, cs;
    sincos((gl & 1) ? q : 0.5 * q, &sn, &cs);
    ws.cs[gl >> 1][(gl & 1) * 2 + 0] = cs;
    ws.cs[gl >> 1][(gl & 1) * 2 + 1] = sn;
  }
  __syncthreads();
  RKH_STAMP(0)

  // ---- base -> tip sweep (kte_map_chain::doMotion), group-uniform
  {
    d3 pos = ld3(base);
    d4 Q = ld4(base + 3);
    d3 w = mk3(0, 0, 0), alpha = mk3(0, 0, 0);
    d3 acc = ld3(base + 7);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int jb = j * 32;
      if (sc_beam->branch_start[j]) {  // a new branch: base frame * mount pose (rigid_link_3D::doMotion from frame 0)
        const d4 bq = ld4(base + 3);
        pos = ld3(base) + mul(rotmat(bq), ld3(sc_beam->mount_pos[j]));
        Q = qmul(bq, ld4(sc_beam->mount_quat[j]));
        w = mk3(0, 0, 0);
        alpha = mk3(0, 0, 0);
        acc = ld3(base + 7);
      }
      const d3 axis = cget3(cp, jb + JC_AXIS);
      const d3 axis_n = cget3(cp, jb + JC_AXISN);
      const double c2 = ws.cs[j][0], s2 = ws.cs[j][1];
      const double qd = ws.x[2 * j + 1];
      d4 EQ;
      d3 Ew, Ealpha;
      if (PRISM && ((sc_beam->prismatic_mask >> j) & 1u)) {
        // prismatic_joint_3D::doMotion (prismatic_joint.cpp:116-148), q_ddot = 0: the end frame keeps the base's
        // orientation and rates and moves by R(Q) (q a)
        const d3 tmp_pos = ws.x[2 * j] * axis;
        const d3 tmp_vel = qd * axis;
        const m33 Rb = rotmat(Q);
        acc = acc + mul(Rb, (cross(w, cross(w, tmp_pos)) + 2.0 * cross(w, tmp_vel)) + cross(alpha, tmp_pos));
        pos = pos + mul(Rb, tmp_pos);
        EQ = Q;
        Ew = w;
        Ealpha = alpha;
      } else {
        // revolute_joint_3D::doMotion (revolute_joint.cpp:121-148)
        const d4 tq = d4{c2, axis_n.x * s2, axis_n.y * s2, axis_n.z * s2};
        const m33 R2 = rotmat(tq);
        EQ = qmul(Q, tq);
        const d3 wb = mulT(w, R2);
        const d3 qa = qd * axis;
        Ew = wb + qa;
        Ealpha = mulT(alpha, R2) + cross(wb, qa);
      }
      st3(lead ? ws.Epos[j] : sink, pos);
      st4(lead ? ws.Equat[j] : sink, EQ);
      // rigid_link_3D::doMotion = frame * pose (frame_3D.hpp:240-255)
      const d3 op = cget3(cp, jb + JC_OFFP);
      const m33 R = rotmat(EQ);
      pos = pos + mul(R, op);
      acc = acc + mul(R, cross(Ew, cross(Ew, op)) + cross(Ealpha, op));
      const m33 Ro = m33{cget(cp, jb + JC_OFFR + 0), cget(cp, jb + JC_OFFR + 1), cget(cp, jb + JC_OFFR + 2),
                         cget(cp, jb + JC_OFFR + 3), cget(cp, jb + JC_OFFR + 4), cget(cp, jb + JC_OFFR + 5),
                         cget(cp, jb + JC_OFFR + 6), cget(cp, jb + JC_OFFR + 7), cget(cp, jb + JC_OFFR + 8)};
      Q = qmul(EQ, d4{cget(cp, jb + JC_OFFQ), cget(cp, jb + JC_OFFQ + 1), cget(cp, jb + JC_OFFQ + 2),
                      cget(cp, jb + JC_OFFQ + 3)});
      alpha = mulT(Ealpha, Ro);
      w = mulT(Ew, Ro);
      // inertia_3D::doForce terms (inertia.cpp:111-122), applied in the backward sweep
      const double inertia[6] = {cget(cp, jb + JC_INER), cget(cp, jb + JC_INER + 1), cget(cp, jb + JC_INER + 2),
                                 cget(cp, jb + JC_INER + 3), cget(cp, jb + JC_INER + 4), cget(cp, jb + JC_INER + 5)};
      const d3 Fi = cget(cp, jb + JC_MASS) * qrot(qinv(Q), acc);
      const d3 Ti = sym_mul(inertia, alpha) + cross(w, sym_mul(inertia, w));
      st3(lead ? ws.Lpos[j] : sink, pos);
      st4(lead ? ws.Lquat[j] : sink, Q);
      st3(lead ? ws.FT[j] : sink, Fi);
      st3(lead ? ws.FT[j] + 3 : sink, Ti);
    }
  }
  __syncthreads();
  {
    // flexible_beam_3D::doForce (listed last in the chain, so it runs first in the reverse pass and its force is the
    // first term of its anchor frames' accumulators); anchors are link end frames (or a world anchor for anchor 2)
    d3 BF1 = mk3(0, 0, 0), BT1 = mk3(0, 0, 0), BF2 = mk3(0, 0, 0), BT2 = mk3(0, 0, 0);
    if (sc_beam->beam_on) {
      const int j1 = sc_beam->beam_j1, j2 = sc_beam->beam_j2;
      const d3 p1 = ld3(ws.Lpos[j1]);
      const d4 q1 = ld4(ws.Lquat[j1]);
      const d3 p2 = j2 >= 0 ? ld3(ws.Lpos[j2]) : ld3(sc_beam->beam_pos);
      const d4 q2 = j2 >= 0 ? ld4(ws.Lquat[j2]) : ld4(sc_beam->beam_quat);
      beam_force(p1, q1, p2, q2, sc_beam->beam_rest, sc_beam->beam_k, sc_beam->beam_kt, &BF1, &BT1);
      if (j2 >= 0) beam_force_anchor2(p1, q1, p2, q2, sc_beam->beam_rest, sc_beam->beam_k, sc_beam->beam_kt, &BF2, &BT2);
    }
    __syncthreads();
    st3(lead ? ws.BFT[0] : sink, BF1);
    st3(lead ? ws.BFT[0] + 3 : sink, BT1);
    st3(lead ? ws.BFT[1] : sink, BF2);
    st3(lead ? ws.BFT[1] + 3 : sink, BT2);
  }
  __syncthreads();
  RKH_STAMP(1)

  // ---- jacobian columns
  feval_jacobian_columns<N, GL, PRISM>(sc_beam, jl, ws, gl);

  RKH_STAMP(2)
  // ---- tip -> base sweep (kte_map_chain::doForce in reverse op order), group-uniform
  double f_mine = 0.0;  // lane i < N keeps generalized force i
  {
    d3 LF = mk3(0, 0, 0), LT = mk3(0, 0, 0);
    const int bj1 = sc_beam->beam_on ? sc_beam->beam_j1 : -1, bj2 = sc_beam->beam_on ? sc_beam->beam_j2 : -1;
#pragma unroll
    for (int j = N - 1; j >= 0; --j) {
      const int jb = j * 32;
      const d3 axis = cget3(cp, jb + JC_AXIS);
      if (j + 1 < N && sc_beam->branch_start[j + 1]) {  // the joint above started another branch: this link is a tip
        LF = mk3(0, 0, 0);
        LT = mk3(0, 0, 0);
      }
      // the beam acted first on its anchor frames (reverse op order): (0 + beam) + what the child joint passes down
      if (j == bj1) {
        LF = LF + ld3(ws.BFT[0]);
        LT = LT + ld3(ws.BFT[0] + 3);
      }
      if (j == bj2) {
        LF = LF + ld3(ws.BFT[1]);
        LT = LT + ld3(ws.BFT[1] + 3);
      }
      // inertia_3D::doForce on the link end frame
      LF = LF - ld3(ws.FT[j]);
      LT = LT - ld3(ws.FT[j] + 3);
      // rigid_link_3D::doForce (rigid_link.cpp:170-178)
      const m33 Ro = m33{cget(cp, jb + JC_OFFR + 0), cget(cp, jb + JC_OFFR + 1), cget(cp, jb + JC_OFFR + 2),
                         cget(cp, jb + JC_OFFR + 3), cget(cp, jb + JC_OFFR + 4), cget(cp, jb + JC_OFFR + 5),
                         cget(cp, jb + JC_OFFR + 6), cget(cp, jb + JC_OFFR + 7), cget(cp, jb + JC_OFFR + 8)};
      const d3 op = cget3(cp, jb + JC_OFFP);
      const d3 tmp_force = mul(Ro, LF);
      const d3 ET = mul(Ro, LT) + cross(op, tmp_force);
      const double uj = ws.u[j];
      double fj;
      if (PRISM && ((sc_beam->prismatic_mask >> j) & 1u)) {
        // prismatic_joint_3D::doForce (prismatic_joint.cpp:150-170): the force along the axis goes to the coordinate
        const double tf = dot(tmp_force, axis);
        LF = tmp_force - tf * axis;
        LT = ET + cross(ws.x[2 * j] * axis, tmp_force);
        // inertia_gen::doForce (q_ddot = 0) ; driving_actuator_gen::doForce with prismatic_joint_3D::applyReactionForce
        // (prismatic_joint.cpp:219-222): a force on the base frame
        fj = tf + uj;
        LF = LF - uj * axis;
      } else {
        // revolute_joint_3D::doForce (revolute_joint.cpp:170-181)
        const m33 Ra = axis_angle_rotmat(ws.cs[j][2], ws.cs[j][3], cget3(cp, jb + JC_AXISN));
        const double ta = dot(ET, axis);
        LF = mul(Ra, tmp_force);
        LT = mul(Ra, ET - ta * axis);
        // inertia_gen::doForce: f -= q_ddot * mass with q_ddot = 0 ; driving_actuator_gen::doForce
        fj = ta + uj;
        LT = LT - uj * axis;
      }
      f_mine = (gl == j) ? fj : f_mine;
    }
  }
  if (gl < N) ws.tmp[gl] = f_mine;  // bias force, kept for the kernel-level parity export
  __syncthreads();
  RKH_STAMP(3)

  // ---- Mf = Tcm^T (Mcm Tcm), M
  feval_mass_matrix<N, GL>(sc_beam, cp, jl, ws, gl, [] { __syncthreads(); });

  RKH_STAMP(4)
  // ---- linsolve_Cholesky (mat_cholesky.hpp:546-554), then backsub_Cholesky_impl (mat_cholesky.hpp:160-178)
  double Lrow[N];
#pragma unroll
  for (int k = 0; k < N; ++k) Lrow[k] = 0.0;
  const bool sing = feval_cholesky_factor<N>(ws, gl, Lrow, [] { __syncthreads(); });
  const double accv = feval_backsub<N>(ws, gl, gb, Lrow, f_mine);
  if (sing) *singular = true;

  // pd[2j] = q_dot_j ; pd[2j+1] = qdd_j  (kte_nl_system.hpp:276-279)
  const double qdd = __shfl(accv, gb + (gl >> 1), 64);
  double out = 0.0;
  if (gl < D) out = (gl & 1) ? qdd : ws.x[gl + 1];
  RKH_STAMP(5)
#undef RKH_STAMP
  return out;
}

// x' = f(x,u) by TWO waves (the latency form of the latency mapping: rounds so small that half the chip's SIMDs would
// idle even at one wave per edge -- a single problem, a graph planner's step).  One f-eval of state_derivative is ~6.6 k
// fp64 instructions in one wave's stream, 26.5 k cycles, and its phases are not all dependent:
//   wave 0: joint / link end frames (the pose half of the base -> tip sweep) -> Jacobian columns -> Mf -> M -> Cholesky factor
//   wave 1: velocities, accelerations, d'Alembert terms (the other half of the sweep, one joint behind wave 0: it waits on
//           a counter in LDS, never on a barrier) -> beam -> tip -> base force sweep -> generalized forces
// then wave 0 solves and leaves x' in LDS for both.  Every value is formed by the same operation sequence as in
// state_derivative (the two halves of the sweep only share the rotation matrix of a joint's end frame, which each
// forms from the same quaternion), so the result is the same bits.  Critical path ~15 k cycles.
RKH_DI void wave_sync() {  // LDS traffic of this wave's lanes, ordered (no block barrier: the other wave is elsewhere)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}
template <int N>
__device__ double state_derivative_duo(const SceneDev* __restrict__ sc_beam, const CPack<N>& cp,
                                       const JointLds* __restrict__ jl, const double* __restrict__ base, GroupWs<N>& ws,
                                       double* __restrict__ sink, int gl, int wave, bool* singular,
                                       unsigned long long* stamps = nullptr) {
  constexpr int D = 2 * N, GL = 64;
  const bool lead = (gl == 0);
  // diagnostic builds only: cycles per phase of this wave (wave 0: sincos, frames, columns, Mf + M, factor, wait, solve;
  // wave 1: sincos, velocity half, beam, force sweep, wait)
#define RKH_STAMP(i)                                                \
  if (stamps) {                                                     \
    const unsigned long long t_now = __builtin_readcyclecounter(); \
    stamps[i] += t_now - t_prev;                                    \
    t_prev = t_now;                                                 \
  }
  unsigned long long t_prev = stamps ? __builtin_readcyclecounter() : 0ull;
  uint32_t branches = 0u;  // bit j: joint j starts a new branch at the chain base (read once, ahead of the serial loops)
#pragma unroll
  for (int j = 0; j < N; ++j) branches |= sc_beam->branch_start[j] ? (1u << j) : 0u;
  if (gl < D) {  // sin / cos (both waves: the same values)
    const double q = ws.x[gl & ~1];
    double sn, cs;
    sincos((gl & 1) ? q : 0.5 * q, &sn, &cs);
    ws.cs[gl >> 1][(gl & 1) * 2 + 0] = cs;
    ws.cs[gl >> 1][(gl & 1) * 2 + 1] = sn;
  }
  if (wave == 0 && lead) {
    ws.duo_ready = 0u;
    ws.duo_sing = 0u;
  }
  __syncthreads();
  RKH_STAMP(0)
  double Lrow[N];
#pragma unroll
  for (int k = 0; k < N; ++k) Lrow[k] = 0.0;
  bool sing = false;
  if (wave == 0) {
    {  // ---- pose half of the base -> tip sweep; every joint's end frames are published as soon as they are stored
      d3 pos = ld3(base);
      d4 Q = ld4(base + 3);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int jb = j * 32;
        if ((branches >> j) & 1u) {
          const d4 bq = ld4(base + 3);
          pos = ld3(base) + mul(rotmat(bq), ld3(sc_beam->mount_pos[j]));
          Q = qmul(bq, ld4(sc_beam->mount_quat[j]));
        }
        const d3 axis_n = cget3(cp, jb + JC_AXISN);
        const double c2 = ws.cs[j][0], s2 = ws.cs[j][1];
        const d4 tq = d4{c2, axis_n.x * s2, axis_n.y * s2, axis_n.z * s2};
        const d4 EQ = qmul(Q, tq);
        st3(lead ? ws.Epos[j] : sink, pos);
        st4(lead ? ws.Equat[j] : sink, EQ);
        const d3 op = cget3(cp, jb + JC_OFFP);
        const m33 R = rotmat(EQ);
        pos = pos + mul(R, op);
        Q = qmul(EQ, d4{cget(cp, jb + JC_OFFQ), cget(cp, jb + JC_OFFQ + 1), cget(cp, jb + JC_OFFQ + 2),
                        cget(cp, jb + JC_OFFQ + 3)});
        st3(lead ? ws.Lpos[j] : sink, pos);
        st4(lead ? ws.Lquat[j] : sink, Q);
        wave_sync();
        if (lead) __hip_atomic_store(&ws.duo_ready, uint32_t(j + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    RKH_STAMP(1)
    // ---- jacobian columns
    feval_jacobian_columns<N, GL, false>(sc_beam, jl, ws, gl);
    wave_sync();
    RKH_STAMP(2)
    // ---- Mf = Tcm^T (Mcm Tcm), M, Cholesky factor (wave-local ordering instead of barriers)
    feval_mass_matrix<N, GL>(sc_beam, cp, jl, ws, gl, [] { wave_sync(); });
    RKH_STAMP(3)
    sing = feval_cholesky_factor<N>(ws, gl, Lrow, [] { wave_sync(); });
    RKH_STAMP(4)
  } else {
    // ---- velocity / acceleration half of the base -> tip sweep.  Only the recurrences w, alpha, acc are serial: the
    // joint rotation matrices before them and the d'Alembert terms after them take one LANE per joint.
    if (gl < N) {
      const d3 axis_n = ld3(jl[gl].axis_n);
      const double c2 = ws.cs[gl][0], s2 = ws.cs[gl][1];
      const m33 R2 = rotmat(d4{c2, axis_n.x * s2, axis_n.y * s2, axis_n.z * s2});
      double* r2 = ws.R2[gl];
      r2[0] = R2.a11; r2[1] = R2.a12; r2[2] = R2.a13; r2[3] = R2.a21; r2[4] = R2.a22; r2[5] = R2.a23;
      r2[6] = R2.a31; r2[7] = R2.a32; r2[8] = R2.a33;
      const m33 Ra = axis_angle_rotmat(ws.cs[gl][2], ws.cs[gl][3], axis_n);  // revolute_joint_3D::doForce's rotation
      double* ra = ws.RA[gl];
      ra[0] = Ra.a11; ra[1] = Ra.a12; ra[2] = Ra.a13; ra[3] = Ra.a21; ra[4] = Ra.a22; ra[5] = Ra.a23;
      ra[6] = Ra.a31; ra[7] = Ra.a32; ra[8] = Ra.a33;
    }
    wave_sync();
    {
      d3 w = mk3(0, 0, 0), alpha = mk3(0, 0, 0);
      d3 acc = ld3(base + 7);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int jb = j * 32;
        // joint j's end frame from wave 0 (a counter in LDS: wave 0 does not stop for this)
        while (__hip_atomic_load(&ws.duo_ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < uint32_t(j + 1))
          __builtin_amdgcn_s_sleep(1);
        if ((branches >> j) & 1u) {
          w = mk3(0, 0, 0);
          alpha = mk3(0, 0, 0);
          acc = ld3(base + 7);
        }
        const d3 axis = cget3(cp, jb + JC_AXIS);
        const double qd = ws.x[2 * j + 1];
        const m33 R2 = ldm(ws.R2[j]);
        const d3 wb = mulT(w, R2);
        const d3 qa = qd * axis;
        const d3 Ew = wb + qa;
        const d3 Ealpha = mulT(alpha, R2) + cross(wb, qa);
        const d3 op = cget3(cp, jb + JC_OFFP);
        const m33 R = rotmat(ld4(ws.Equat[j]));
        acc = acc + mul(R, cross(Ew, cross(Ew, op)) + cross(Ealpha, op));
        const m33 Ro = m33{cget(cp, jb + JC_OFFR + 0), cget(cp, jb + JC_OFFR + 1), cget(cp, jb + JC_OFFR + 2),
                           cget(cp, jb + JC_OFFR + 3), cget(cp, jb + JC_OFFR + 4), cget(cp, jb + JC_OFFR + 5),
                           cget(cp, jb + JC_OFFR + 6), cget(cp, jb + JC_OFFR + 7), cget(cp, jb + JC_OFFR + 8)};
        alpha = mulT(Ealpha, Ro);
        w = mulT(Ew, Ro);
        st3(lead ? ws.Wj[j] : sink, w);
        st3(lead ? ws.ALj[j] : sink, alpha);
        st3(lead ? ws.ACCj[j] : sink, acc);
      }
    }
    wave_sync();
    if (gl < N) {  // inertia_3D::doForce terms (inertia.cpp:111-122) of joint gl's link, applied in the backward sweep
      const d4 Q = ld4(ws.Lquat[gl]);
      const d3 acc = ld3(ws.ACCj[gl]), alpha = ld3(ws.ALj[gl]), w = ld3(ws.Wj[gl]);
      const double* inertia = jl[gl].inertia;
      const d3 Fi = jl[gl].mass * qrot(qinv(Q), acc);
      const d3 Ti = sym_mul(inertia, alpha) + cross(w, sym_mul(inertia, w));
      st3(ws.FT[gl], Fi);
      st3(ws.FT[gl] + 3, Ti);
    }
    wave_sync();
    RKH_STAMP(1)
    {  // flexible_beam_3D::doForce (as in state_derivative)
      d3 BF1 = mk3(0, 0, 0), BT1 = mk3(0, 0, 0), BF2 = mk3(0, 0, 0), BT2 = mk3(0, 0, 0);
      if (sc_beam->beam_on) {
        const int j1 = sc_beam->beam_j1, j2 = sc_beam->beam_j2;
        const d3 p1 = ld3(ws.Lpos[j1]);
        const d4 q1 = ld4(ws.Lquat[j1]);
        const d3 p2 = j2 >= 0 ? ld3(ws.Lpos[j2]) : ld3(sc_beam->beam_pos);
        const d4 q2 = j2 >= 0 ? ld4(ws.Lquat[j2]) : ld4(sc_beam->beam_quat);
        beam_force(p1, q1, p2, q2, sc_beam->beam_rest, sc_beam->beam_k, sc_beam->beam_kt, &BF1, &BT1);
        if (j2 >= 0) beam_force_anchor2(p1, q1, p2, q2, sc_beam->beam_rest, sc_beam->beam_k, sc_beam->beam_kt, &BF2, &BT2);
      }
      st3(lead ? ws.BFT[0] : sink, BF1);
      st3(lead ? ws.BFT[0] + 3 : sink, BT1);
      st3(lead ? ws.BFT[1] : sink, BF2);
      st3(lead ? ws.BFT[1] + 3 : sink, BT2);
    }
    wave_sync();
    RKH_STAMP(2)
    double f_mine = 0.0;
    {  // ---- tip -> base sweep (as in state_derivative)
      d3 LF = mk3(0, 0, 0), LT = mk3(0, 0, 0);
      const int bj1 = sc_beam->beam_on ? sc_beam->beam_j1 : -1, bj2 = sc_beam->beam_on ? sc_beam->beam_j2 : -1;
#pragma unroll
      for (int j = N - 1; j >= 0; --j) {
        const int jb = j * 32;
        const d3 axis = cget3(cp, jb + JC_AXIS);
        if (j + 1 < N && ((branches >> (j + 1 < N ? j + 1 : 0)) & 1u)) {
          LF = mk3(0, 0, 0);
          LT = mk3(0, 0, 0);
        }
        if (j == bj1) {
          LF = LF + ld3(ws.BFT[0]);
          LT = LT + ld3(ws.BFT[0] + 3);
        }
        if (j == bj2) {
          LF = LF + ld3(ws.BFT[1]);
          LT = LT + ld3(ws.BFT[1] + 3);
        }
        LF = LF - ld3(ws.FT[j]);
        LT = LT - ld3(ws.FT[j] + 3);
        const m33 Ro = m33{cget(cp, jb + JC_OFFR + 0), cget(cp, jb + JC_OFFR + 1), cget(cp, jb + JC_OFFR + 2),
                           cget(cp, jb + JC_OFFR + 3), cget(cp, jb + JC_OFFR + 4), cget(cp, jb + JC_OFFR + 5),
                           cget(cp, jb + JC_OFFR + 6), cget(cp, jb + JC_OFFR + 7), cget(cp, jb + JC_OFFR + 8)};
        const d3 op = cget3(cp, jb + JC_OFFP);
        const d3 tmp_force = mul(Ro, LF);
        const d3 ET = mul(Ro, LT) + cross(op, tmp_force);
        const m33 Ra = ldm(ws.RA[j]);
        const double ta = dot(ET, axis);
        LF = mul(Ra, tmp_force);
        LT = mul(Ra, ET - ta * axis);
        const double uj = ws.u[j];
        const double fj = ta + uj;
        LT = LT - uj * axis;
        f_mine = (gl == j) ? fj : f_mine;
      }
    }
    if (gl < N) ws.tmp[gl] = f_mine;
    RKH_STAMP(3)
  }
  __syncthreads();
  RKH_STAMP(5)
  if (wave == 0) {  // backsub_Cholesky_impl (mat_cholesky.hpp:160-178): L y = f, then L^T x = y
    const double accv = feval_backsub<N>(ws, gl, 0, Lrow, (gl < N) ? ws.tmp[gl] : 0.0);
    const double qdd = __shfl(accv, gl >> 1, 64);
    if (gl < D) ws.dpx[gl] = (gl & 1) ? qdd : ws.x[gl + 1];
    if (sing && lead) ws.duo_sing = 1u;
  }
  __syncthreads();
  RKH_STAMP(6)
#undef RKH_STAMP
  if (ws.duo_sing) *singular = true;
  return gl < D ? ws.dpx[gl] : 0.0;
}

}  // namespace rkh
