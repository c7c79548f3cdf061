// propagate.hip -- RK4 forward-dynamics propagation of a KTE serial chain with a proximity
// (collision) test after every step, for batches of candidate edges (gfx950, wave64).
//
// What it replaces (paths relative to /root/reference/src/ReaK/):
//   steer loop        examples/misc/MEAQR_topology.hpp:503-565 (steer_with_constant_control pattern)
//   RK4               ctrl/sys_integrators/runge_kutta4_integrator_sys.hpp:53-97
//   x' = f(x,u)       ctrl/ctrl_sys/kte_nl_system.hpp:180-290 (apply_states_and_inputs, get_state_derivative)
//   KTE passes        ctrl/mbd_kte/kte_map_chain.hpp:71-89; revolute_joint.cpp:121-213; rigid_link.cpp:152-186;
//                     inertia.cpp:47-54,111-122; driving_actuator.cpp:31-39
//   mass matrix       ctrl/mbd_kte/mass_matrix_calculator.cpp:80-295 + core/kinetostatics/motion_jacobians.hpp:238-251
//   Cholesky solve    core/lin_alg/mat_cholesky.hpp:63-84,160-178,546-554
//   is_free           ctrl/topologies/manip_free_workspace.hpp:79-99 + geometry/proximity (proximity_device.h)
//
// Mapping onto the wave.  A block is one wave; a wave carries 64/GL candidate edges, GL lanes each
// (GL = 64: one wavefront per candidate, lowest latency; GL = 16: four candidates per wave, used when
// many planners oversubscribe the chip).  Within an edge's lane group:
//   * state x, RK4 temporaries, bounds: lane d < 2N owns component d (one register each)
//   * sin/cos of the N joint angles (half- and full-angle): lanes 0..2N-1 in parallel
//   * base->tip kinematic sweep and tip->base force sweep: serial by nature; every lane of the group runs
//     them on group-uniform values read by LDS broadcast (no cross-lane traffic), joints unrolled (template N)
//   * Jacobian columns Tcm(body b, coord c<=b): one lane per (b,c) pair; M(i,j): one lane per entry
//   * Cholesky: lane i owns row i (divisions of a column run in parallel), same per-element operation order
//   * proximity pairs: one lane per (robot shape, obstacle) pair, ballot for "any distance < 0"
// Chain parameters, obstacle table and all per-edge intermediates live in LDS.
// Compiled with -ffp-contract=off: products and sums round exactly as in the CPU reference; only
// sin/cos (OCML vs glibc) differ by ulps (stated tolerance: 1e-10 relative on propagated states).
//
// Scenes with prismatic joints (SceneDev::has_prismatic) run on forms of the one-wave steer, f-eval, distance and
// 3D edge-walk kernels compiled from this same text in a translation unit of their own (propagate_prismatic.hip
// defines RKH_PRISMATIC_FORMS and includes this file): there everything below lives in rkh::prismatic and kPrismatic
// is true.  Here kPrismatic is false and the prismatic branches compile away, so the revolute kernels keep their code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>

#include "device_math.h"
#include "proximity_device.h"
#include "proximity_planar_device.h"
#include "proximity_record_device.h"
#include "rkh_internal.h"

// Two more translation units take single forms out of this text and none of its other kernels or launchers:
// propagate_planar_qs_prismatic.hip (RKH_PLANAR_PRISMATIC_QS) and propagate_depth.hip (RKH_DEPTH_RECORDS).
#if defined(RKH_PLANAR_PRISMATIC_QS) || defined(RKH_DEPTH_RECORDS)
#define RKH_FORMS_ONLY 1
#endif

namespace rkh {
#ifdef RKH_PRISMATIC_FORMS
namespace prismatic {
constexpr bool kPrismatic = true;
#else
constexpr bool kPrismatic = false;
#endif

struct __attribute__((aligned(16))) JointLds {  // chain parameters of one joint group, staged in LDS
  double axis[3], joint_inertia;
  double axis_n[3], mass;
  double off_pos[3], pad0;
  double off_quat[4];
  double off_R[9], pad1;
  double inertia[6];
};

template <int N>
struct __attribute__((aligned(16))) GroupWs {  // per-edge LDS workspace
  double x[2 * N];                  // state being differentiated (q, qd interleaved)
  double b[2 * N];                  // steer target
  double u[N];                      // held input
  double tmp[2 * N];                // lane-parallel -> sequential-sum staging
  double cs[N][4];                  // c2, s2 (half angle), c1, s1 (full angle)
  double Epos[N][3], Equat[N][4];   // joint end frames (jacobian parents)
  double Lpos[N][3], Lquat[N][4];   // link end frames (inertia frames)
  double FT[N][6];                  // inertia_3D d'Alembert force / torque (to be subtracted)
  double BFT[2][6];                 // flexible beam force / torque on its two anchor frames (zero without a beam)
  double Tcm[N][N][6];              // [body][coord] jacobian column (v, w)
  double Mf[N][N];                  // Tcm^T (Mcm Tcm) before symmetrisation
  double M[N][N];                   // symmetric M, overwritten by its Cholesky factor
  double Rpos[2 * N][3], Rquat[2 * N][4];  // robot shapes, global pose
  // two waves per edge (state_derivative_duo): x' as the solving wave leaves it for the other one, the number of joints
  // whose end frames the first wave has published, the first wave's "pivot below 1e-8" verdict
  double dpx[2 * N];
  double R2[N][9], RA[N][9];               // rotation matrices of the joint rotations (half-angle quaternion / axis-angle form)
  double Wj[N][3], ALj[N][3], ACCj[N][3];  // link end frames: angular velocity, angular acceleration, acceleration
  uint32_t duo_ready, duo_sing;
};

template <int N, int GL>
struct BlockLds {
  JointLds joints[N];
  double base[10];  // pos3, quat4, acc3
  double sink[64][4];  // per-lane dummy store target: keeps the group-leader stores branch-free
  GroupWs<N> g[64 / GL];
};

// the quasi-static kernels (edge walk, distance query) only need what the proximity test touches
template <int N>
struct __attribute__((aligned(16))) GroupWsQs {
  double x[2 * N];
  double tmp[2 * N];
  double cs[N][4];
  double Epos[N][3], Equat[N][4];
  double Rpos[2 * N][3], Rquat[2 * N][4];
};
template <int N, int GL>
struct BlockLdsQs {
  JointLds joints[N];
  double base[10];
  double sink[64][4];
  GroupWsQs<N> g[64 / GL];
};

RKH_DI d3 ld3(const double* p) { return d3{p[0], p[1], p[2]}; }
RKH_DI d4 ld4(const double* p) { return d4{p[0], p[1], p[2], p[3]}; }
RKH_DI void st3(double* p, d3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
RKH_DI void st4(double* p, d4 v) { p[0] = v.w; p[1] = v.x; p[2] = v.y; p[3] = v.z; }
RKH_DI m33 ldm(const double* p) { return m33{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]}; }

// Chain parameters are wave-uniform.  They are packed into R vector registers (lane l of register r
// holds flat parameter r*64 + l, JointLds layout) and read back with v_readlane: no memory latency on
// the serial sweeps' critical path and no long-lived scalar registers.
template <int N>
struct CPack {
  static constexpr int R = (N * 32 + 63) / 64;
  double v[R];
};
RKH_DI double readlane_f64(double v, int src_lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}
template <int N>
RKH_DI double cget(const CPack<N>& cp, int idx) { return readlane_f64(cp.v[idx >> 6], idx & 63); }
template <int N>
RKH_DI d3 cget3(const CPack<N>& cp, int idx) { return d3{cget(cp, idx), cget(cp, idx + 1), cget(cp, idx + 2)}; }
template <int N>
RKH_DI CPack<N> load_cpack(const JointLds* jl, int lane) {
  CPack<N> cp;
#pragma unroll
  for (int r = 0; r < CPack<N>::R; ++r) {
    const int idx = r * 64 + lane;
    cp.v[r] = idx < N * 32 ? reinterpret_cast<const double*>(jl)[idx] : 0.0;
  }
  return cp;
}
// field offsets inside JointLds (in doubles)
enum : int { JC_AXIS = 0, JC_JIN = 3, JC_AXISN = 4, JC_MASS = 7, JC_OFFP = 8, JC_OFFQ = 12, JC_OFFR = 16, JC_INER = 26 };

// axis_angle::getRotMat (rotations_3D.hpp:2160-2180) from cos/sin of the angle and the unit axis
RKH_DI m33 axis_angle_rotmat(double ca, double sa, d3 ax) {
  const double omc = 1.0 - ca;
  const double t11 = ca + omc * ax.x * ax.x, t22 = ca + omc * ax.y * ax.y, t33 = ca + omc * ax.z * ax.z;
  const double t12 = omc * ax.x * ax.y, t13 = omc * ax.x * ax.z, t23 = omc * ax.y * ax.z;
  const double t01 = sa * ax.x, t02 = sa * ax.y, t03 = sa * ax.z;
  return m33{t11, t12 - t03, t13 + t02, t12 + t03, t22, t23 - t01, t13 - t02, t23 + t01, t33};
}

template <int N>
__device__ __forceinline__ void stage_chain(const SceneDev* __restrict__ sc, JointLds* jl, double* base, int lane) {
  for (int i = lane; i < N * 32; i += 64) {
    const int j = i >> 5, k = i & 31;
    const JointDev& J = sc->joints[j];
    double v = 0.0;
    if (k < 3) v = J.axis[k];
    else if (k == 3) v = J.joint_inertia;
    else if (k < 7) v = J.axis_n[k - 4];
    else if (k == 7) v = J.mass;
    else if (k < 11) v = J.off_pos[k - 8];
    else if (k == 11) v = 0.0;
    else if (k < 16) v = J.off_quat[k - 12];
    else if (k < 25) v = J.off_R[k - 16];
    else if (k == 25) v = 0.0;
    else v = J.inertia[k - 26];
    reinterpret_cast<double*>(&jl[j])[k] = v;
  }
  if (lane < 3) base[lane] = sc->base_pos[lane];
  else if (lane < 7) base[lane] = sc->base_quat[lane - 3];
  else if (lane < 10) base[lane] = sc->base_acc[lane - 7];
}

__device__ __forceinline__ void stage_env(const SceneDev* __restrict__ sc, ShapeDev* env_lds, int lane) {
  const int n_words = sc->n_env * int(sizeof(ShapeDev) / sizeof(double));
  const double* src = reinterpret_cast<const double*>(sc->env);
  double* dst = reinterpret_cast<double*>(env_lds);
  for (int i = lane; i < n_words; i += 64) dst[i] = src[i];
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

// Planar scenes (SceneDev::planar): revolute_joint_2D / rigid_link_2D kinematics (revolute_joint.cpp:30-47,
// rigid_link.cpp:87-99), pose_2D::getGlobalPose of the robot shapes, then proxy_query_pair_2D::findMinimumDistance
// (proxy_query_model.cpp:163-189) replayed in finder order: every lane computes one pair's cull value and distance,
// and the sequence "skip if cull > running minimum, else take the minimum" is resolved lane by lane.
// PRISM (the rkh::planar_prismatic kernels): joints whose bit is set in SceneDev::prismatic_mask are prismatic_joint_2D
// (prismatic_joint.cpp:44-46,60): the end frame is the base moved by R (q a), no sincos.  The mask is uniform over the
// launch, and the handovers through LDS keep the barriers of the revolute form.
template <int N, int GL, bool PRISM = false, typename WS>
__device__ double proximity_min_planar(const SceneDev* __restrict__ sc, const CPack<N>& cp, const double* __restrict__ base,
                                       const ShapeDev* __restrict__ env_lds, const PairDev* __restrict__ pairs, int n_pairs,
                                       WS& ws, int gl, int gb) {
  for (int jj = gl; jj < N; jj += GL) {
    if (PRISM && ((sc->prismatic_mask >> jj) & 1u)) continue;
    double sn, cs;
    sincos(ws.x[2 * jj], &sn, &cs);
    ws.cs[jj][0] = cs;
    ws.cs[jj][1] = sn;
  }
  __syncthreads();
  {
    d2 pos = mk2(base[0], base[1]);
    d2 R = mk2(base[3], base[4]);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int jb = j * 32;
      d2 ER;
      if (PRISM && ((sc->prismatic_mask >> j) & 1u)) {
        pos = pos + rrot(R, ws.x[2 * j] * mk2(cget(cp, jb + JC_AXIS), cget(cp, jb + JC_AXIS + 1)));
        ER = R;
      } else {
        ER = rmul(R, mk2(ws.cs[j][0], ws.cs[j][1]));
      }
      if (gl == 0) {
        ws.Epos[j][0] = pos.x;
        ws.Epos[j][1] = pos.y;
        ws.Equat[j][0] = ER.x;
        ws.Equat[j][1] = ER.y;
      }
      pos = pos + rrot(ER, mk2(cget(cp, jb + JC_OFFP), cget(cp, jb + JC_OFFP + 1)));
      R = rmul(ER, mk2(cget(cp, jb + JC_OFFQ), cget(cp, jb + JC_OFFQ + 1)));
    }
  }
  __syncthreads();
  for (int r = gl; r < sc->n_robot; r += GL) {
    const ShapeDev& sh = sc->robot[r];
    const int j = sh.link;
    const d2 pp = mk2(ws.Epos[j][0], ws.Epos[j][1]);
    const d2 pr = mk2(ws.Equat[j][0], ws.Equat[j][1]);
    const d2 gp = pp + rrot(pr, mk2(sh.pos[0], sh.pos[1]));
    const d2 gr = rmul(pr, mk2(sh.quat[0], sh.quat[1]));
    ws.Rpos[r][0] = gp.x;
    ws.Rpos[r][1] = gp.y;
    ws.Rquat[r][0] = gr.x;
    ws.Rquat[r][1] = gr.y;
  }
  __syncthreads();
  double min_dist = INFINITY;
  for (int p0 = 0; p0 < n_pairs; p0 += GL) {
    const int p = p0 + gl;
    double d = INFINITY, c = INFINITY;
    if (p < n_pairs) {
      const PairDev pr = pairs[p];
      const ShapeDev& rs = sc->robot[pr.robot];
      const ShapeDev& es = env_lds[pr.env];
      ShapeP A, Bv;
      A.kind = rs.kind;
      A.pos = mk2(ws.Rpos[pr.robot][0], ws.Rpos[pr.robot][1]);
      A.rot = mk2(ws.Rquat[pr.robot][0], ws.Rquat[pr.robot][1]);
      A.d0 = rs.dims[0]; A.d1 = rs.dims[1];
      Bv.kind = es.kind;
      Bv.pos = mk2(es.pos[0], es.pos[1]);
      Bv.rot = mk2(es.quat[0], es.quat[1]);
      Bv.d0 = es.dims[0]; Bv.d1 = es.dims[1];
      const ShapeP& s1 = pr.s1_is_robot ? A : Bv;
      const ShapeP& s2 = pr.s1_is_robot ? Bv : A;
      const double r1 = pr.s1_is_robot ? rs.brad : es.brad;
      const double r2 = pr.s1_is_robot ? es.brad : rs.brad;
      c = norm_2(to_parent(s2, mk2(0.0, 0.0)) - to_parent(s1, mk2(0.0, 0.0))) - r1 - r2;
      d = pair_distance_planar(pr.routine, s1, s2);
    }
    const int cnt = (n_pairs - p0 < GL) ? (n_pairs - p0) : GL;
    for (int l = 0; l < cnt; ++l) {
      const double cl = __shfl(c, gb + l, 64), dl = __shfl(d, gb + l, 64);
      if (p0 + l == 0) min_dist = dl;                       // the first finder is always computed
      else if (!(cl > min_dist) && dl < min_dist) min_dist = dl;
    }
  }
  return min_dist;
}

// Proximity of the configuration in ws.x (joint angles): minimum distance over computed pairs.
// With cull_positive, pairs whose bounding spheres are apart are skipped (they cannot make the verdict
// "colliding"; proxy_query_model.cpp:386-389 culls the same way against the running minimum) and the scan
// stops once every edge of the wave has met a negative distance.
// Global poses of the robot shapes at the configuration in ws.x (ws.Rpos / ws.Rquat), every lane group for its own
// point; ends on a block barrier.
template <int N, int GL, typename WS, bool PRISM = false>
__device__ __forceinline__ void proximity_frames(const SceneDev* __restrict__ sc, const ShapeDev* __restrict__ robot,
                                                 const CPack<N>& cp, const double* __restrict__ base, WS& ws,
                                                 double* __restrict__ sink, int gl) {
  const bool lead = (gl == 0);
  // half-angle sin/cos, one joint per lane (strided: a 16-lane group may carry more than 16 / 2 joints)
  for (int jj = gl; jj < N; jj += GL) {
    double sn, cs;
    sincos(0.5 * ws.x[2 * jj], &sn, &cs);
    ws.cs[jj][0] = cs;
    ws.cs[jj][1] = sn;
  }
  __syncthreads();
  {  // revolute_joint_3D / rigid_link_3D kinematics, position + orientation only
    d3 pos = ld3(base);
    d4 Q = ld4(base + 3);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int jb = j * 32;
      if (sc->branch_start[j]) {  // a new branch: base frame * mount pose (rigid_link_3D::doMotion from frame 0)
        const d4 bq = ld4(base + 3);
        pos = ld3(base) + mul(rotmat(bq), ld3(sc->mount_pos[j]));
        Q = qmul(bq, ld4(sc->mount_quat[j]));
      }
      const d3 axis_n = cget3(cp, jb + JC_AXISN);
      const double c2 = ws.cs[j][0], s2 = ws.cs[j][1];
      d4 EQ;
      if (PRISM && ((sc->prismatic_mask >> j) & 1u)) {  // prismatic_joint_3D: translate by R(Q) (q a), keep Q
        pos = pos + mul(rotmat(Q), ws.x[2 * j] * cget3(cp, jb + JC_AXIS));
        EQ = Q;
      } else {
        const d4 tq = d4{c2, axis_n.x * s2, axis_n.y * s2, axis_n.z * s2};
        EQ = qmul(Q, tq);
      }
      st3(lead ? ws.Epos[j] : sink, pos);
      st4(lead ? ws.Equat[j] : sink, EQ);
      const m33 R = rotmat(EQ);
      pos = pos + mul(R, cget3(cp, jb + JC_OFFP));
      Q = qmul(EQ, d4{cget(cp, jb + JC_OFFQ), cget(cp, jb + JC_OFFQ + 1), cget(cp, jb + JC_OFFQ + 2),
                      cget(cp, jb + JC_OFFQ + 3)});
    }
  }
  __syncthreads();
  // robot shapes -> global pose (pose_3D::getGlobalPose, pose_3D.hpp:102-110)
  for (int r = gl; r < sc->n_robot; r += GL) {
    const ShapeDev& sh = robot[r];
    const int j = sh.link;
    const d3 pp = ld3(ws.Epos[j]);
    const d4 pq = ld4(ws.Equat[j]);
    st3(ws.Rpos[r], pp + qrot(pq, ld3(sh.pos)));
    st4(ws.Rquat[r], qmul(pq, ld4(sh.quat)));
  }
  __syncthreads();
}

template <int N, int GL, typename WS, bool GJK = true, bool PRISM = false>
__device__ double proximity_min(const SceneDev* __restrict__ sc, const CPack<N>& cp,
                                const double* __restrict__ base, const ShapeDev* __restrict__ env_lds,
                                const PairDev* __restrict__ pairs, int n_pairs, WS& ws,
                                double* __restrict__ sink, int gl, int gb, bool cull_positive, bool group_done) {
  if (!PRISM && sc->planar) return proximity_min_planar<N, GL>(sc, cp, base, env_lds, pairs, n_pairs, ws, gl, gb);
  proximity_frames<N, GL, WS, PRISM>(sc, sc->robot, cp, base, ws, sink, gl);
  double dmin = INFINITY;
  bool hit = group_done;  // finished edges of the wave do not hold the scan open
  for (int p0 = 0; p0 < n_pairs; p0 += GL) {
    const int p = p0 + gl;
    double d = INFINITY;
    if (p < n_pairs && !hit) {
      const PairDev pr = pairs[p];
      const ShapeDev& rs = sc->robot[pr.robot];
      const ShapeDev& es = env_lds[pr.env];
      ShapeG A, Bv;
      A.kind = rs.kind;
      A.pos = ld3(ws.Rpos[pr.robot]);
      A.q = ld4(ws.Rquat[pr.robot]);
      A.d0 = rs.dims[0]; A.d1 = rs.dims[1]; A.d2 = rs.dims[2];
      Bv.kind = es.kind;
      Bv.pos = ld3(es.pos);
      Bv.q = ld4(es.quat);
      Bv.d0 = es.dims[0]; Bv.d1 = es.dims[1]; Bv.d2 = es.dims[2];
      bool skip = false;
      if (cull_positive) {
        // transformToGlobal(0) of both shapes, then |c2 - c1| - r1 - r2 (proxy_query_model.cpp:384-389)
        const d3 c1 = pr.s1_is_robot ? pose_to_parent(A.pos, A.q, mk3(0, 0, 0)) : pose_to_parent(Bv.pos, Bv.q, mk3(0, 0, 0));
        const d3 c2p = pr.s1_is_robot ? pose_to_parent(Bv.pos, Bv.q, mk3(0, 0, 0)) : pose_to_parent(A.pos, A.q, mk3(0, 0, 0));
        const double r1 = pr.s1_is_robot ? rs.brad : es.brad;
        const double r2 = pr.s1_is_robot ? es.brad : rs.brad;
        skip = (norm_2(c2p - c1) - r1 - r2 > 0.0);
      }
      if (!skip) d = pr.s1_is_robot ? pair_distance<GJK>(pr.routine, A, Bv, sc->mesh_verts) : pair_distance<GJK>(pr.routine, Bv, A, sc->mesh_verts);
    }
    if (d < dmin) dmin = d;
    if (cull_positive) {
      // per-edge "any lane found a negative distance", then stop when every edge of the wave has one
      const unsigned long long m = __ballot(d < 0.0);
      const unsigned long long gm = (GL == 64) ? m : ((m >> gb) & ((1ull << (GL & 63)) - 1ull));
      hit = hit || (gm != 0ull);
      if (__all(hit)) break;
    }
  }
  // group min
#pragma unroll
  for (int off = GL / 2; off > 0; off >>= 1) {
    const double o = __shfl_xor(dmin, off, 64);
    if (o < dmin) dmin = o;
  }
  return dmin;
}

// exact left-to-right euclidean metric of a lane-distributed difference vector
// (vect_distance_metrics.hpp:126-137): stage the squares in LDS, every lane sums them in order
template <int N>
RKH_DI double group_norm(GroupWs<N>& ws, double diff, int gl) {
  if (gl < 2 * N) ws.tmp[gl] = diff * diff;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < 2 * N; ++d) s = s + ws.tmp[d];
  __syncthreads();
  return sqrt(s);
}

template <int N, int GL>
struct SmemLayoutQs {
  static constexpr size_t block_bytes = (sizeof(BlockLdsQs<N, GL>) + 15) / 16 * 16;
  static size_t bytes(int n_env) { return block_bytes + size_t(n_env) * sizeof(ShapeDev); }
};
template <int N, int GL>
struct SmemLayout {
  static constexpr size_t block_bytes = (sizeof(BlockLds<N, GL>) + 15) / 16 * 16;
  static size_t bytes(int n_env) { return block_bytes + size_t(n_env) * sizeof(ShapeDev); }
};

struct WaveArgs {
  const SceneDev* sc;
  const PairDev* pairs;
  int n_pairs;
  DynDev dyn;
  EdgeIO io_a, io_b;
  const EdgeIO* tab_a;
  const EdgeIO* tab_b;
  uint32_t grid_a;
  KernelGate gate;
};
typedef const __attribute__((address_space(4))) WaveArgs* WaveArgP;
RKH_DI WaveArgP wave_args() {
  WaveArgP a = (WaveArgP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a));
  return a;
}

// ---------------------------------------------------------------------------------------------
// Kernel: steer edges.  Two edge groups per launch (planner: this round's steer candidates + the
// previous round's goal probes); 64/GL edges per wave.
// GL = 64 (one wave per edge, the latency mapping: rounds of fewer waves than the chip has SIMDs) may use the whole
// register file of its SIMD; four edges per wave (GL = 16) is the throughput form and keeps two waves per SIMD.
// DUO (GL = 64 only): two waves per edge.  Both run this body in step -- the same loads, the same RK4 glue, the same
// control flow, so every block barrier is met by both -- and differ inside state_derivative_duo; only the first wave
// writes results.
template <int N, int GL, bool GJK, bool DUO = false>
__global__ __launch_bounds__(DUO ? 128 : 64, GL == 64 ? 1 : 2) void propagate_kernel(WaveArgs) {
  static_assert(!DUO || GL == 64, "two waves per edge: one edge per block");
  // Every argument is read through the kernarg segment pointer at its point of use (by-value parameters are loaded in the
  // entry block and stay live in scalar registers; once those run out they are spilled into vector-register lanes, and
  // the EdgeIO / DynDev / KernelGate copies alone are ~170 dwords: the kernel then needed 256 registers + 185 spilled)
  const SceneDev* __restrict__ sc = wave_args()->sc;
  const PairDev* __restrict__ pairs = wave_args()->pairs;
  const int n_pairs = wave_args()->n_pairs;
  const uint32_t grid_a = wave_args()->grid_a;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  if (steer_gate_closed(&wave_args()->gate)) return;  // the planner's per-round choice between the kernel mappings
  constexpr int G = 64 / GL;
  BlockLds<N, GL>& lds = *reinterpret_cast<BlockLds<N, GL>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayout<N, GL>::block_bytes);
  // blockIdx.y selects the planning problem when per-problem EdgeIO tables are given
  bool group_b = blockIdx.x >= grid_a;
  uint32_t problem = blockIdx.y;
  uint32_t blk = group_b ? blockIdx.x - grid_a : blockIdx.x;
  if (wave_args()->gate.wave_base) {  // compact mapping (one edge per wave): block L of a 1-D grid takes working edge L
    const uint32_t L = blockIdx.x;
    if (L >= wave_args()->gate.wave_base[wave_args()->gate.n_segments]) return;
    const uint32_t seg = segment_of(wave_args()->gate.wave_base, wave_args()->gate.n_segments, L);
    problem = seg >> 1;
    group_b = (seg & 1u) != 0u;
    blk = L - wave_args()->gate.wave_base[seg];
  }
  auto edge_io = [&]() -> const EdgeIO* {
    WaveArgP A = wave_args();
    if (A->tab_a) return (group_b ? A->tab_b : A->tab_a) + problem;
    const char* ka = (const char*)(const void*)A;
    return (const EdgeIO*)(ka + (group_b ? offsetof(WaveArgs, io_b) : offsetof(WaveArgs, io_a)));
  };
  const uint32_t B = edge_io()->d_B ? *edge_io()->d_B : edge_io()->B;
  const int lane = DUO ? int(threadIdx.x & 63u) : int(threadIdx.x);
  const int wave = DUO ? int(threadIdx.x >> 6) : 0;
  const bool writer = !DUO || wave == 0;  // the wave whose results leave the block
  const int g = lane / GL, gl = lane % GL, gb = g * GL;
  const uint32_t e0 = blk * G;
  if (e0 >= B) return;
  const uint32_t e = e0 + g;
  const bool edge_valid = e < B;
  const uint32_t ec = edge_valid ? e : e0;  // idle groups shadow the wave's first edge, results discarded
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  stage_env(sc, env_lds, lane);
  GroupWs<N>& ws = lds.g[g];
  const uint32_t si = edge_source_row(*edge_io(), ec);
  const uint64_t trow = edge_target_row(*edge_io(), ec);
  const double a_d = (gl < D) ? edge_io()->src[uint64_t(si) * edge_io()->src_stride + gl] : 0.0;
  const double b_d = (gl < D) ? edge_io()->tgt[trow * edge_io()->tgt_stride + gl] : 0.0;
  const double lo = (gl < D) ? wave_args()->dyn.lower[gl] : 0.0;
  const double hi = (gl < D) ? wave_args()->dyn.upper[gl] : 0.0;
  if (gl < D) ws.b[gl] = b_d;
  double* __restrict__ record = (edge_valid && writer) ? edge_io()->record : nullptr;
  const int record_stride = edge_io()->record_stride;
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);

  double x = a_d;
  uint32_t n_free = 0;
  bool singular = false;   // a live edge met a singular mass matrix
  bool alive = true;       // this edge is still stepping
  uint32_t n_exec = 0;     // steps integrated for this edge (KernelGate::steps_exec)
  if (record && gl < D) record[(uint64_t(e) * record_stride + 0) * D + gl] = x;

  // steps of this edge: the launch's schedule, or (EdgeIO::frac) those of the edge's own travel fraction
  int n_steps = wave_args()->dyn.n_steps;
  if (edge_io()->frac) n_steps = edge_step_count(edge_io()->frac[ec], wave_args()->dyn.full_time, wave_args()->dyn.dt);
  if (edge_io()->mode == EDGE_POINT) {  // is_free(target): bounds, then proximity; no propagation
    n_steps = 0;
    x = b_d;
    const bool oob = (gl < D) && hyperbox_out(lo, hi, x);
    const unsigned long long m = __ballot(oob);
    const unsigned long long gm = (GL == 64) ? m : ((m >> gb) & ((1ull << (GL & 63)) - 1ull));
    bool free_pt = gm == 0ull;
    if (gl < D) ws.x[gl] = x;
    __syncthreads();
    const double dmin = proximity_min<N, GL, GroupWs<N>, GJK, kPrismatic>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, lds.sink[lane], gl, gb, true, !free_pt);
    if (dmin < 0.0) free_pt = false;
    if (edge_valid && gl == 0 && writer) edge_io()->accept[e] = free_pt ? 1 : 0;
  }

  for (int k = 0; k < n_steps; ++k) {
    // distance(x_current, x_goal) > goal_proximity_threshold
    const double dist = group_norm<N>(ws, x - b_d, gl);
    if (!(dist > wave_args()->dyn.goal_tol)) alive = false;
    if (!__any(alive)) break;
    if (alive) ++n_exec;
    // PD law, zero-order hold over the step
    if (gl < D) ws.x[gl] = x;
    __syncthreads();
    if (gl < N)
      ws.u[gl] = pd_input(wave_args()->dyn.kp, wave_args()->dyn.kd, wave_args()->dyn.u_max, ws.b[2 * gl], ws.x[2 * gl],
                          ws.b[2 * gl + 1], ws.x[2 * gl + 1]);
    // runge_kutta4_integrate_impl, time_step = dt: one call site for f(x,u), the stages of rk4_stage (steer_edge.h) in a
    // rolled loop.  The re-prime after the last iteration is dead in the reference and is not evaluated.
    const double h = wave_args()->dyn.dt;
    double xe = x;  // end_point
    {
      double w = xe, k1 = 0.0, k2 = 0.0, k3 = 0.0;
      bool sing_now = false;
      const int n_evals = 4 * wave_args()->dyn.inner[k];
#pragma unroll 1
      for (int ev = 0; ev < n_evals; ++ev) {
        if (gl < D) ws.x[gl] = xe;
        __syncthreads();
        const double dp = DUO ? state_derivative_duo<N>(sc, cp, lds.joints, lds.base, ws, lds.sink[lane], gl, wave, &sing_now)
                              : state_derivative<N, GL, kPrismatic>(sc, cp, lds.joints, lds.base, ws, lds.sink[lane], gl, gb, &sing_now);
        rk4_stage(ev & 3, h, dp, xe, w, k1, k2, k3);
      }
      if (sing_now && alive) {
        singular = true;
        alive = false;
      }
    }
    // is_free(x_next): hyperbox bounds, then proximity
    const bool oob = (gl < D) && hyperbox_out(lo, hi, xe);
    {
      const unsigned long long m = __ballot(oob);
      const unsigned long long gm = (GL == 64) ? m : ((m >> gb) & ((1ull << (GL & 63)) - 1ull));
      if (gm != 0ull) alive = false;
    }
    if (!__any(alive)) break;
    if (gl < D) ws.x[gl] = xe;
    __syncthreads();
    const double dmin = proximity_min<N, GL, GroupWs<N>, GJK, kPrismatic>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, lds.sink[lane], gl, gb, true, !alive);
    if (dmin < 0.0) alive = false;
    if (alive) {
      x = xe;
      ++n_free;
      if (record && gl < D) record[(uint64_t(e) * record_stride + n_free) * D + gl] = x;
    }
  }
  if (singular && gl == 0 && edge_valid && writer) atomicExch(edge_io()->err_flag, int(RKH_ERR_SINGULAR));
  if (edge_valid && gl < D && writer) edge_io()->x_out[uint64_t(e) * D + gl] = x;
  if (edge_valid && gl == 0 && writer) edge_io()->steps_free[e] = n_free;
  if (wave_args()->gate.steps_exec && edge_valid && gl == 0 && n_exec && writer)
    atomicAdd(wave_args()->gate.steps_exec, (unsigned long long)n_exec);
  if (edge_io()->mode != EDGE_PLAIN) {
    const double n_ar = group_norm<N>(ws, a_d - x, gl);
    const double n_ab = group_norm<N>(ws, a_d - b_d, gl);
    const double n_rb = group_norm<N>(ws, x - b_d, gl);
    const int acc = edge_accept(edge_io()->mode, n_ar, n_ab, n_rb, edge_io()->best_case, ec, edge_io()->steer_tol, kNoWalk);
    if (edge_valid && gl == 0 && writer) {
      if (acc != kNoAccept) edge_io()->accept[e] = uint8_t(acc);
      else if (edge_io()->mode == EDGE_GOAL_PROBE) edge_io()->goal_dist[si - 1] = goal_probe_steerable(n_ab, n_rb);
    }
  }
}

// Kernel: x' = f(x,u) for B states (one wave each); also exports M and the bias force.
template <int N>
__global__ __launch_bounds__(64) void state_derivative_kernel(const SceneDev* __restrict__ sc, const double* __restrict__ x,
                                                               const double* __restrict__ u, uint32_t B,
                                                               double* __restrict__ pd, double* __restrict__ M,
                                                               double* __restrict__ f, int* __restrict__ err_flag) {
  __shared__ BlockLds<N, 64> lds;
  const uint32_t e = blockIdx.x;
  if (e >= B) return;
  const int lane = threadIdx.x;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  GroupWs<N>& ws = lds.g[0];
  if (lane < D) ws.x[lane] = x[uint64_t(e) * D + lane];
  if (lane < N) ws.u[lane] = u[uint64_t(e) * N + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  bool singular = false;
  const double dp = state_derivative<N, 64, kPrismatic>(sc, cp, lds.joints, lds.base, ws, lds.sink[lane], lane, 0, &singular);
  if (lane < D) pd[uint64_t(e) * D + lane] = dp;
  if (singular && lane == 0) atomicExch(err_flag, int(RKH_ERR_SINGULAR));
  // exports for the kernel-level parity tests: the symmetric M is rebuilt from Mf (ws.M now holds its
  // Cholesky factor); the bias force was parked in ws.tmp by state_derivative.
  if (M)
    for (int t = lane; t < N * N; t += 64) {
      const int i = t / N, j = t % N;
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      M[uint64_t(e) * N * N + t] = (i == j) ? ws.Mf[i][i] : 0.5 * (ws.Mf[lo][hi] + ws.Mf[hi][lo]);
    }
  if (f && lane < N) f[uint64_t(e) * N + lane] = ws.tmp[lane];
}

// ---------------------------------------------------------------------------------------------
// Kernel: quasi-static edge walk interp_topo_move_position_toward_pred
// (ctrl/interpolation/interpolated_topologies.hpp:137-163) over joint positions (D = N), with
// manip_quasi_static_env::is_free (manip_free_workspace.hpp:154-156) as the predicate.
// Planar scenes (SceneDev::planar) only: 3D scenes walk in edge_points_kernel below, whose verdict may take the pairs
// in any order, while a planar verdict depends on the finder order (proximity_min_planar).
// One block of W waves per edge; its 4 * W 16-lane groups test that many consecutive interpolation points at a time
// (the points of a straight edge are independent), and the first colliding one is found from the groups' verdicts.
// dist_cur is accumulated by repeated addition exactly like the reference loop (":157 dist_cur += min_interval"),
// so the number of tested points is the same integer.  W (launch_edge_check) grows as the launch has fewer edges:
// 1 wave for thousands (the batch planner's rounds fill the machine with one wave per edge), up to 8 for a few hundred
// (a step of one or a few graph planners, which waits for its longest edge).
constexpr int kEdgeGL = 16;  // lanes per point
template <int N, int W>
struct BlockLdsQsW {
  static constexpr int G = (64 / kEdgeGL) * W;  // groups of the block = points per pass
  JointLds joints[N];
  double base[10];
  GroupWsQs<N> g[G];
  double pts[G][N];       // the groups' interpolation points (space coordinates)
  uint32_t masks[W];      // per wave: bit t = group t's point lies on the edge, bit 4 + t = it passed the predicate
};
template <int N, int W>
struct SmemLayoutQsW {
  static constexpr size_t block_bytes = (sizeof(BlockLdsQsW<N, W>) + 15) / 16 * 16;
  // env shapes, then (if it fits: edge_check_kernel's pairs_staged) the proxy pair list
  static size_t bytes(int n_env, int n_pairs_staged) {
    return block_bytes + size_t(n_env) * sizeof(ShapeDev) + size_t(n_pairs_staged) * sizeof(PairDev);
  }
};

// The arguments of both edge walk kernels (edge_check_kernel, edge_points_kernel), which read them through the kernarg
// segment pointer: a by-value record indexed at run time -- qs.speed[j], the choice between io_a and io_b -- would be
// copied to scratch.
struct EdgeWalkArgs {
  const SceneDev* sc;
  const PairDev* pairs;
  int n_pairs;
  QsDev qs;
  EdgeIO io_a, io_b;
  const EdgeIO* tab_a;
  const EdgeIO* tab_b;
  uint32_t grid_a;
  int pairs_staged;
};
typedef const __attribute__((address_space(4))) EdgeWalkArgs* EdgeWalkArgP;

// One edge walk of edge_check_kernel (the block's groups test G consecutive points per pass); PRISM: of
// planar_prismatic::edge_check_kernel, for chains with prismatic_joint_2D groups.
template <int N, int W, bool PRISM = false>
__device__ __forceinline__ void edge_walk(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs, int n_pairs,
                                          const QsDev& qs, const EdgeIO& io, BlockLdsQsW<N, W>& lds,
                                          const ShapeDev* __restrict__ env_lds, uint32_t e) {
  constexpr int GL = kEdgeGL, GPW = 64 / GL, G = GPW * W;  // lanes per group, groups per wave, groups of the block
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = tid / GL, gl = lane % GL, gb = (lane / GL) * GL;  // group of the block, lane of the group, its base lane in the wave
  GroupWsQs<N>& ws = lds.g[g];
  const uint32_t si = edge_source_row(io, e);
  const uint64_t trow = edge_target_row(io, e);
  const double a_d = (gl < N) ? io.src[uint64_t(si) * io.src_stride + gl] : 0.0;
  const double b_d = (gl < N) ? io.tgt[trow * io.tgt_stride + gl] : 0.0;
  const double lo = (gl < N) ? qs.lower[gl] : 0.0;
  const double hi = (gl < N) ? qs.upper[gl] : 0.0;
  const double speed = (gl < N) ? qs.speed[gl] : 1.0;  // rate-limited space: the model sees point * speed limit
  for (int t = gl; t < 2 * N; t += GL) ws.x[t] = 0.0;  // velocities stay zero (apply_to_model writes positions only)
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);

  // exact left-to-right euclidean norm of an N-vector held by lanes gl < N of every group
  auto norm_n = [&](double diff) {
    if (gl < N) ws.tmp[gl] = diff * diff;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < N; ++d) s = s + ws.tmp[d];
    __syncthreads();
    return sqrt(s);
  };
  if (io.mode == EDGE_POINT) {
    // is_free(target): hyperbox bounds, then proximity (manip_free_workspace.hpp:79-99,154-156); group 0 tests it
    if (gl < N) ws.x[2 * gl] = b_d * speed;
    const bool oob = (gl < N) && hyperbox_out(lo, hi, b_d);
    const unsigned long long mo = __ballot(oob);
    const bool group_oob = ((mo >> gb) & ((1ull << GL) - 1ull)) != 0ull;
    __syncthreads();
    const double dmin = proximity_min_planar<N, GL, PRISM>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, gl, gb);
    const bool is_free = !group_oob && !(dmin < 0.0);
    if (g == 0 && gl < N) io.x_out[uint64_t(e) * N + gl] = b_d;
    if (tid == 0) {
      io.steps_free[e] = 1;
      io.accept[e] = is_free ? 1 : 0;
    }
    return;
  }
  const double dist_tot = norm_n(a_d - b_d);
  const double fraction = io.frac ? io.frac[e] : qs.fraction;
  double result = a_d;       // component gl of the returned point
  uint32_t n_checked = 0;
  bool completed_walk = false;  // the predicate loop ran to dist_inter without a collision (EDGE_STEER_BOTH)
  if (dist_tot == INFINITY) {
    result = a_d;
  } else if (dist_tot < qs.min_interval) {
    result = a_d + (b_d - a_d) * fraction;  // vector_topology::move_position_toward, no predicate call
  } else {
    const double dist_inter = dist_tot * fraction;
    double cur = 0.0;          // dist_cur of the last tested point (0 + min_interval == min_interval exactly)
    double last_result = a_d;  // last point that passed the predicate
    bool collided = false;
    for (;;) {
      // dist_cur of this group's point and of the block's first and last ones: cur + min_interval, repeatedly
      double my = cur, last = cur;
#pragma unroll
      for (int t = 0; t < G; ++t) {
        if (t <= g) my = my + qs.min_interval;
        last = last + qs.min_interval;
      }
      if (!((cur + qs.min_interval) < dist_inter)) break;  // not even the first point is on the edge (block-uniform)
      const bool valid = my < dist_inter;
      const double pt = a_d + (b_d - a_d) * (my / dist_tot);
      if (gl < N) {
        ws.x[2 * gl] = pt * speed;
        lds.pts[g][gl] = pt;
      }
      const bool oob = (gl < N) && hyperbox_out(lo, hi, pt);
      const unsigned long long mo = __ballot(oob);
      const bool group_oob = ((mo >> gb) & ((1ull << GL) - 1ull)) != 0ull;
      __syncthreads();
      const double dmin = proximity_min_planar<N, GL, PRISM>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, gl, gb);
      const bool is_free = valid && !group_oob && !(dmin < 0.0);
      {  // the wave's verdicts -> LDS, then every thread scans the block's groups in edge order
        const unsigned long long mv = __ballot(valid && gl == 0), mf = __ballot(is_free && gl == 0);
        uint32_t m = 0;
#pragma unroll
        for (int t = 0; t < GPW; ++t)
          m |= (uint32_t((mv >> ((t * GL) & 63)) & 1ull) << t) | (uint32_t((mf >> ((t * GL) & 63)) & 1ull) << (4 + t));
        if (lane == 0) lds.masks[wave] = m;
      }
      __syncthreads();
      int first_bad = G;  // first valid group whose point fails the predicate
      int n_valid = 0;
#pragma unroll
      for (int t = G - 1; t >= 0; --t) {
        const uint32_t m = lds.masks[t / GPW];
        const bool v = (m >> (t % GPW)) & 1u, f = (m >> (4 + (t % GPW))) & 1u;
        if (v && !f) first_bad = t;
        if (v) n_valid = n_valid > t + 1 ? n_valid : t + 1;
      }
      if (first_bad < G) {
        n_checked += uint32_t(first_bad + 1);
        if (first_bad > 0 && gl < N) last_result = lds.pts[first_bad - 1][gl];
        collided = true;
        break;
      }
      n_checked += uint32_t(n_valid);
      if (gl < N) last_result = lds.pts[n_valid - 1][gl];
      if (n_valid < G) break;  // reached dist_inter without a collision
      cur = last;
      __syncthreads();         // the points and verdicts are rewritten by the next pass
    }
    completed_walk = !collided;
    if (collided) result = last_result;
    else if (fraction == 1.0) result = b_d;  // exact end fractions (:159-162)
    else if (fraction == 0.0) result = a_d;
    else result = a_d + (b_d - a_d) * fraction;
  }
  if (g == 0 && gl < N) io.x_out[uint64_t(e) * N + gl] = result;
  if (tid == 0) io.steps_free[e] = n_checked;
  if (io.mode != EDGE_PLAIN) {
    const double n_ar = norm_n(a_d - result);
    const double n_ab = dist_tot;
    const double n_rb = norm_n(result - b_d);
    const int acc = edge_accept(io.mode, n_ar, n_ab, n_rb, io.best_case, e, io.steer_tol, completed_walk ? 1 : 0);
    if (tid == 0) {
      if (acc != kNoAccept) io.accept[e] = uint8_t(acc);
      else if (io.mode == EDGE_GOAL_PROBE) io.goal_dist[si - 1] = goal_probe_interpolated(n_ab, n_rb);
    }
  }
}

template <int N, int W>
__device__ __forceinline__ const PairDev* edge_check_stage(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                           int n_pairs, int pairs_staged, BlockLdsQsW<N, W>& lds,
                                                           ShapeDev* env_lds) {
  const int tid = threadIdx.x, lane = tid & 63;
  stage_chain<N>(sc, lds.joints, lds.base, lane);  // (every wave writes the same values)
  stage_env(sc, env_lds, lane);
  // and, when the launch made room for it, the pair list, which every point scans
  if (!pairs_staged) return pairs;
  PairDev* pl = reinterpret_cast<PairDev*>(env_lds + sc->n_env);
  for (int i = tid; i < n_pairs; i += 64 * W) pl[i] = pairs[i];
  return pl;
}

template <int N, int W>
__global__ __launch_bounds__(64 * W) void edge_check_kernel(EdgeWalkArgs) {
  EdgeWalkArgP ka = (EdgeWalkArgP)__builtin_amdgcn_kernarg_segment_ptr();
  const SceneDev* __restrict__ sc = ka->sc;
  const int n_pairs = ka->n_pairs;
  const uint32_t grid_a = ka->grid_a;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BlockLdsQsW<N, W>& lds = *reinterpret_cast<BlockLdsQsW<N, W>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayoutQsW<N, W>::block_bytes);
  const bool group_b = blockIdx.x >= grid_a;
  const EdgeIO* iok = (const EdgeIO*)(group_b ? &ka->io_b : &ka->io_a);
  const EdgeIO io = ka->tab_a ? (group_b ? ka->tab_b[blockIdx.y] : ka->tab_a[blockIdx.y]) : *iok;
  const uint32_t B = io.d_B ? *io.d_B : io.B;
  const uint32_t e = group_b ? blockIdx.x - grid_a : blockIdx.x;
  if (e >= B) return;
  const PairDev* pairs = edge_check_stage<N, W>(sc, ka->pairs, n_pairs, ka->pairs_staged, lds, env_lds);
  edge_walk<N, W>(sc, pairs, n_pairs, *(const QsDev*)&ka->qs, io, lds, env_lds, e);
}

#ifdef RKH_PLANAR_PRISMATIC_QS
// The position-level forms for planar chains with prismatic_joint_2D groups (SceneDev::planar && has_prismatic): the
// edge walk here and the distance query below, over proximity_min_planar<.., PRISM = true>.  They are compiled in a
// translation unit of their own (propagate_planar_qs_prismatic.hip defines RKH_PLANAR_PRISMATIC_QS and includes this
// file), which instantiates these kernels and nothing else: a kernel added to this unit's module would shift the
// code of the ones it holds.  (rkh::prismatic holds the forms of 3D chains.)
namespace planar_prismatic {
template <int N, int W>
__global__ __launch_bounds__(64 * W) void edge_check_kernel(EdgeWalkArgs) {
  EdgeWalkArgP ka = (EdgeWalkArgP)__builtin_amdgcn_kernarg_segment_ptr();
  const SceneDev* __restrict__ sc = ka->sc;
  const int n_pairs = ka->n_pairs;
  const uint32_t grid_a = ka->grid_a;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BlockLdsQsW<N, W>& lds = *reinterpret_cast<BlockLdsQsW<N, W>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayoutQsW<N, W>::block_bytes);
  const bool group_b = blockIdx.x >= grid_a;
  const EdgeIO* iok = (const EdgeIO*)(group_b ? &ka->io_b : &ka->io_a);
  const EdgeIO io = ka->tab_a ? (group_b ? ka->tab_b[blockIdx.y] : ka->tab_a[blockIdx.y]) : *iok;
  const uint32_t B = io.d_B ? *io.d_B : io.B;
  const uint32_t e = group_b ? blockIdx.x - grid_a : blockIdx.x;
  if (e >= B) return;
  const PairDev* pairs = edge_check_stage<N, W>(sc, ka->pairs, n_pairs, ka->pairs_staged, lds, env_lds);
  edge_walk<N, W, true>(sc, pairs, n_pairs, *(const QsDev*)&ka->qs, io, lds, env_lds, e);
}
}  // namespace planar_prismatic
#endif

// ---------------------------------------------------------------------------------------------
// The same edge walk for 3D scenes, with ONE LANE PER POINT in the chain kinematics (edge_points_kernel).  A 16-lane
// group per point, as in edge_check_kernel, would run the serial base -> tip chain once per point: ~1.2 k fp64
// instructions per wave for 4 points.  Here a block of 4 waves takes G = 64 (32 for chains of more than 7 joints)
// consecutive points per pass and every phase is spread over what it is parallel in:
//   half-angle sin / cos   one (point, joint) per thread
//   joint end frames       one POINT per lane of the first wave: the serial chain, once per 64 points
//   robot shape poses      one (point, shape) per thread
//   bounding-sphere cull   one (point, pair) per thread -> survivors into the LDS queue
//   closed forms           one surviving (point, pair) per thread
// and the first colliding point comes out of two ballots.  is_free only asks whether SOME proxy pair is closer than 0
// (manip_free_workspace.hpp:154-156), so the pairs need no order: the cull is exactly findMinimumDistance's test
// against a running minimum of 0 (proxy_query_model.cpp:384-389), behind a cheaper test on squares that only ever skips
// what that one skips, and a pass nearly always needs ONE round of closed forms.  Should the survivors not fit the
// queue, the pair list is redone in slices that fit whatever survives.  Per-point data sit in LDS component-major
// ([..][G]: lanes of a wave = consecutive points = consecutive addresses).  Planar scenes, whose verdict depends on the
// finder order, walk in edge_check_kernel.
struct EdgePointsCfg {
  static constexpr int T = 256;                // threads per block
  static constexpr int QCAP = 1024;            // surviving (point, pair) combinations per round of closed forms
};
// G = points per pass: 64 for the launches of few edges (the step waits for its longest walk), 32 for the launches of
// thousands of edges (half the LDS, three blocks per CU) and for chains of more than 7 joints
template <int N, int G>
struct __attribute__((aligned(16))) EdgePointsLds {
  JointLds joints[N];
  double base[10];
  ShapeDev robot[2 * N];
  double a[N], b[N], res[N];      // the edge's end points; staging of an N-vector for the ordered sums
  double pts[N][G];               // the pass's interpolation points (space coordinates)
  double cs[N][2][G];             // cos, sin of the half joint angles
  double E[N][7][G];              // joint end frames: position, quaternion
  double R[2 * N][7][G];          // robot shapes, global pose
  uint32_t flags[G];              // bit 0: to be tested (on the edge, inside the bounds), bit 1: a pair closer than 0, bit 2: on the edge
  uint32_t q_cnt;
  uint32_t scan[2];               // first point that fails the predicate, points on the edge
  uint32_t queue[EdgePointsCfg::QCAP];
};
template <int N, int G>
struct EdgePointsSmem {
  static constexpr size_t block_bytes = (sizeof(EdgePointsLds<N, G>) + 15) / 16 * 16;
  static constexpr size_t bytes(int n_env, int n_pairs_staged) {
    return block_bytes + size_t(n_env) * sizeof(ShapeDev) + size_t(n_pairs_staged) * sizeof(PairDev);
  }
};

template <int N, bool GJK, int G>
__global__ __launch_bounds__(256) void edge_points_kernel(EdgeWalkArgs) {
  EdgeWalkArgP ka = (EdgeWalkArgP)__builtin_amdgcn_kernarg_segment_ptr();
  const SceneDev* __restrict__ sc = ka->sc;
  const PairDev* __restrict__ pairs = ka->pairs;
  const int n_pairs = ka->n_pairs, pairs_staged = ka->pairs_staged;
  const uint32_t grid_a = ka->grid_a;
  const EdgeIO* __restrict__ tab_a = ka->tab_a;
  const EdgeIO* __restrict__ tab_b = ka->tab_b;
  const auto& qs = ka->qs;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int T = EdgePointsCfg::T, QCAP = EdgePointsCfg::QCAP;
  EdgePointsLds<N, G>& lds = *reinterpret_cast<EdgePointsLds<N, G>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + EdgePointsSmem<N, G>::block_bytes);
  const bool group_b = blockIdx.x >= grid_a;
  const EdgeIO* iop = tab_a ? (group_b ? &tab_b[blockIdx.y] : &tab_a[blockIdx.y]) : nullptr;
  const __attribute__((address_space(4))) EdgeIO* iok = group_b ? &ka->io_b : &ka->io_a;
#define RKH_IO(f) (iop ? iop->f : iok->f)
  const uint32_t B = RKH_IO(d_B) ? *RKH_IO(d_B) : RKH_IO(B);
  const uint32_t e = group_b ? blockIdx.x - grid_a : blockIdx.x;
  if (e >= B) return;
  const int tid = threadIdx.x, lane = tid & 63;
  stage_chain<N>(sc, lds.joints, lds.base, lane);  // (every wave writes the same values)
  stage_env(sc, env_lds, lane);
  {
    const int n_words = sc->n_robot * int(sizeof(ShapeDev) / sizeof(double));
    for (int i = tid; i < n_words; i += T) reinterpret_cast<double*>(lds.robot)[i] = reinterpret_cast<const double*>(sc->robot)[i];
    if (pairs_staged) {
      PairDev* pl = reinterpret_cast<PairDev*>(env_lds + sc->n_env);
      for (int i = tid; i < n_pairs; i += T) pl[i] = pairs[i];
      pairs = pl;
    }
  }
  const int mode = RKH_IO(mode);
  if (tid < N) {
    const uint32_t si = edge_source_row(RKH_IO(src_idx), RKH_IO(d_src_first), e);
    const uint64_t trow = edge_target_row(RKH_IO(tgt_idx), RKH_IO(d_tgt_off), e);
    lds.a[tid] = RKH_IO(src)[uint64_t(si) * RKH_IO(src_stride) + tid];
    lds.b[tid] = RKH_IO(tgt)[trow * RKH_IO(tgt_stride) + tid];
  }
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  const int n_robot = sc->n_robot;

  // exact left-to-right euclidean norm of the N-vector whose component d thread d holds (vect_distance_metrics.hpp:126-137)
  auto norm_n = [&](double diff) {
    if (tid < N) lds.res[tid] = diff * diff;
    __syncthreads();
    double sacc = 0.0;
#pragma unroll
    for (int d = 0; d < N; ++d) sacc = sacc + lds.res[d];
    __syncthreads();
    return sqrt(sacc);
  };
  // is_free's proximity half for the points flagged 1 in lds.flags (their coordinates in lds.pts): sets bit 1 of the
  // flag of every point with a proxy pair closer than 0.  Block-uniform control flow throughout.
  auto test_points = [&](int n_pts) {
    for (int idx = tid; idx < G * N; idx += T) {   // half-angle sin / cos (revolute_joint_3D::doMotion)
      const int t = idx % G, j = idx / G;
      if (t >= n_pts) continue;
      double sn, cs;
      sincos(0.5 * (lds.pts[j][t] * qs.speed[j]), &sn, &cs);
      lds.cs[j][0][t] = cs;
      lds.cs[j][1][t] = sn;
    }
    __syncthreads();
    if (tid < G) {  // revolute_joint_3D / rigid_link_3D kinematics, position + orientation only: this lane's point
      const int t = tid;
      d3 pos = ld3(lds.base);
      d4 Q = ld4(lds.base + 3);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int jb = j * 32;
        if (sc->branch_start[j]) {  // a new branch: base frame * mount pose (rigid_link_3D::doMotion from frame 0)
          const d4 bq = ld4(lds.base + 3);
          pos = ld3(lds.base) + mul(rotmat(bq), ld3(sc->mount_pos[j]));
          Q = qmul(bq, ld4(sc->mount_quat[j]));
        }
        const d3 axis_n = cget3(cp, jb + JC_AXISN);
        const double c2 = lds.cs[j][0][t], s2 = lds.cs[j][1][t];
        d4 EQ;
        if (kPrismatic && ((sc->prismatic_mask >> j) & 1u)) {  // prismatic_joint_3D: translate by R(Q) (q a), keep Q
          pos = pos + mul(rotmat(Q), (lds.pts[j][t] * qs.speed[j]) * cget3(cp, jb + JC_AXIS));
          EQ = Q;
        } else {
          const d4 tq = d4{c2, axis_n.x * s2, axis_n.y * s2, axis_n.z * s2};
          EQ = qmul(Q, tq);
        }
        lds.E[j][0][t] = pos.x; lds.E[j][1][t] = pos.y; lds.E[j][2][t] = pos.z;
        lds.E[j][3][t] = EQ.w; lds.E[j][4][t] = EQ.x; lds.E[j][5][t] = EQ.y; lds.E[j][6][t] = EQ.z;
        const m33 Rm = rotmat(EQ);
        pos = pos + mul(Rm, cget3(cp, jb + JC_OFFP));
        Q = qmul(EQ, d4{cget(cp, jb + JC_OFFQ), cget(cp, jb + JC_OFFQ + 1), cget(cp, jb + JC_OFFQ + 2),
                        cget(cp, jb + JC_OFFQ + 3)});
      }
    }
    __syncthreads();
    for (int idx = tid; idx < G * n_robot; idx += T) {  // robot shapes -> global pose (pose_3D::getGlobalPose, pose_3D.hpp:102-110)
      const int t = idx % G, r = idx / G;
      const ShapeDev& sh = lds.robot[r];
      const int j = sh.link;
      const d3 pp = d3{lds.E[j][0][t], lds.E[j][1][t], lds.E[j][2][t]};
      const d4 pq = d4{lds.E[j][3][t], lds.E[j][4][t], lds.E[j][5][t], lds.E[j][6][t]};
      const d3 gp = pp + qrot(pq, ld3(sh.pos));
      const d4 gq = qmul(pq, ld4(sh.quat));
      lds.R[r][0][t] = gp.x; lds.R[r][1][t] = gp.y; lds.R[r][2][t] = gp.z;
      lds.R[r][3][t] = gq.w; lds.R[r][4][t] = gq.x; lds.R[r][5][t] = gq.y; lds.R[r][6][t] = gq.z;
    }
    __syncthreads();
    // bounding-sphere cull of every (pair, point), survivors -> queue -> closed forms (see above)
    int p_lo = 0, p_step = n_pairs;
    while (p_lo < n_pairs) {
      const int p_hi = (p_lo + p_step < n_pairs) ? p_lo + p_step : n_pairs;
      {  // a wave's lanes are consecutive points of ONE pair (two pairs when G = 32): the pair's constants are uniform
        constexpr int PPB = T / G;   // pairs per block iteration
        const int t = tid % G;
        const bool live = lds.flags[t] == 5u;
        auto cull = [&](int p) {
          const PairDev pr = pairs[p];
          const ShapeDev& rs = lds.robot[pr.robot];
          const ShapeDev& es = env_lds[pr.env];
          const d3 ca = d3{lds.R[pr.robot][0][t], lds.R[pr.robot][1][t], lds.R[pr.robot][2][t]}, cb = ld3(es.pos);
          const d3 dc = pr.s1_is_robot ? cb - ca : ca - cb;
          const double r1 = pr.s1_is_robot ? rs.brad : es.brad, r2 = pr.s1_is_robot ? es.brad : rs.brad;
          const double sq = ((0.0 + dc.x * dc.x) + dc.y * dc.y) + dc.z * dc.z, rr = r1 + r2;
          if (sq > (rr * rr) * (1.0 + 1e-9)) return false;   // clearly apart: the exact test below skips it too
          return !(sqrt(sq) - r1 - r2 > 0.0);                // |c2 - c1| - r1 - r2 > 0 (proxy_query_model.cpp:384-389, minimum 0)
        };
        int p = p_lo + tid / G;
        for (; p + 3 * PPB < p_hi; p += 4 * PPB) {  // four independent pairs in flight
          const bool k0 = cull(p), k1 = cull(p + PPB), k2 = cull(p + 2 * PPB), k3 = cull(p + 3 * PPB);
          if (live) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const bool k = u == 0 ? k0 : (u == 1 ? k1 : (u == 2 ? k2 : k3));
              if (k) {
                const uint32_t slot = atomicAdd(&lds.q_cnt, 1u);
                if (slot < uint32_t(QCAP)) lds.queue[slot] = uint32_t(t) | (uint32_t(p + u * PPB) << 8);
              }
            }
          }
        }
        for (; p < p_hi; p += PPB) {
          if (live && cull(p)) {
            const uint32_t slot = atomicAdd(&lds.q_cnt, 1u);
            if (slot < uint32_t(QCAP)) lds.queue[slot] = uint32_t(t) | (uint32_t(p) << 8);
          }
        }
      }
      __syncthreads();
      const uint32_t cnt = lds.q_cnt;
      __syncthreads();
      if (tid == 0) lds.q_cnt = 0u;
      if (cnt > uint32_t(QCAP)) {  // (block-uniform) does not fit: slices of QCAP / G pairs always do
        p_step = QCAP / G;
        __syncthreads();
        continue;
      }
      for (uint32_t i = tid; i < cnt; i += T) {
        const uint32_t ent = lds.queue[i];
        const int t = int(ent & 255u);
        if (lds.flags[t] != 5u) continue;              // this point already has a colliding pair
        const PairDev pr = pairs[ent >> 8];
        const ShapeDev& rs = lds.robot[pr.robot];
        const ShapeDev& es = env_lds[pr.env];
        ShapeG A, Bv;
        A.kind = rs.kind;
        A.pos = d3{lds.R[pr.robot][0][t], lds.R[pr.robot][1][t], lds.R[pr.robot][2][t]};
        A.q = d4{lds.R[pr.robot][3][t], lds.R[pr.robot][4][t], lds.R[pr.robot][5][t], lds.R[pr.robot][6][t]};
        A.d0 = rs.dims[0]; A.d1 = rs.dims[1]; A.d2 = rs.dims[2];
        Bv.kind = es.kind;
        Bv.pos = ld3(es.pos);
        Bv.q = ld4(es.quat);
        Bv.d0 = es.dims[0]; Bv.d1 = es.dims[1]; Bv.d2 = es.dims[2];
        const double d = pr.s1_is_robot ? pair_distance<GJK>(pr.routine, A, Bv, sc->mesh_verts)
                                        : pair_distance<GJK>(pr.routine, Bv, A, sc->mesh_verts);
        if (d < 0.0) atomicOr(&lds.flags[t], 2u);
      }
      __syncthreads();
      p_lo = p_hi;
    }
  };
  // hyperbox bounds of point t (manip_free_workspace.hpp:79-99; lower > upper: a wrapped coordinate)
  auto out_of_bounds = [&](int t) {
    bool oob = false;
#pragma unroll
    for (int d = 0; d < N; ++d) oob |= hyperbox_out(qs.lower[d], qs.upper[d], lds.pts[d][t]);
    return oob;
  };

  const double a_d = tid < N ? lds.a[tid] : 0.0, b_d = tid < N ? lds.b[tid] : 0.0;
  if (mode == EDGE_POINT) {
    // is_free(target): hyperbox bounds, then proximity (manip_free_workspace.hpp:79-99,154-156)
    if (tid < N) lds.pts[tid][0] = b_d;
    if (tid == 0) lds.q_cnt = 0u;
    __syncthreads();
    if (tid < G) lds.flags[tid] = (tid == 0 && !out_of_bounds(0)) ? 5u : 0u;
    __syncthreads();
    test_points(1);
    if (tid < N) RKH_IO(x_out)[uint64_t(e) * N + tid] = b_d;
    if (tid == 0) {
      RKH_IO(steps_free)[e] = 1;
      RKH_IO(accept)[e] = (lds.flags[0] == 5u) ? 1 : 0;
    }
    return;
  }
  const double dist_tot = norm_n(a_d - b_d);
  const double fraction = RKH_IO(frac) ? RKH_IO(frac)[e] : qs.fraction;
  double result = a_d;       // component tid of the returned point
  uint32_t n_checked = 0;
  bool completed_walk = false;  // the predicate loop ran to dist_inter without a collision (EDGE_STEER_BOTH)
  if (dist_tot == INFINITY) {
    result = a_d;
  } else if (dist_tot < qs.min_interval) {
    result = a_d + (b_d - a_d) * fraction;  // vector_topology::move_position_toward, no predicate call
  } else {
    const double dist_inter = dist_tot * fraction;
    double cur = 0.0;          // dist_cur of the last tested point (0 + min_interval == min_interval exactly)
    double last_result = a_d;  // last point that passed the predicate
    bool collided = false;
    for (;;) {
      // dist_cur of this thread's point and of the pass's last one: cur + min_interval, repeatedly (":157 dist_cur += min_interval")
      double my = cur, last = cur;
      const int t_mine = tid < G ? tid : 0;
#pragma unroll 8
      for (int t = 0; t < G; ++t) {
        if (t <= t_mine) my = my + qs.min_interval;
        last = last + qs.min_interval;
      }
      if (!((cur + qs.min_interval) < dist_inter)) break;  // not even the first point is on the edge (block-uniform)
      if (tid < G) {
        const bool valid = my < dist_inter;
        const double f = my / dist_tot;
#pragma unroll
        for (int d = 0; d < N; ++d) lds.pts[d][tid] = lds.a[d] + (lds.b[d] - lds.a[d]) * f;
        lds.flags[tid] = valid ? (out_of_bounds(tid) ? 4u : 5u) : 0u;
      }
      if (tid == 0) lds.q_cnt = 0u;
      __syncthreads();
      test_points(G);
      if (tid < 64) {  // the first point on the edge that fails the predicate, and how many points are on the edge
        const uint32_t fl = tid < G ? lds.flags[tid] : 0u;
        const unsigned long long mv = __ballot((fl & 4u) != 0u), mf = __ballot(fl == 5u);
        const unsigned long long bad = mv & ~mf;
        if (tid == 0) {
          lds.scan[0] = bad ? uint32_t(__builtin_ctzll(bad)) : uint32_t(G);
          lds.scan[1] = uint32_t(__builtin_popcountll(mv));
        }
      }
      __syncthreads();
      const int first_bad = int(lds.scan[0]), n_valid = int(lds.scan[1]);
      if (first_bad < G) {
        n_checked += uint32_t(first_bad + 1);
        if (first_bad > 0 && tid < N) last_result = lds.pts[tid][first_bad - 1];
        collided = true;
        break;
      }
      n_checked += uint32_t(n_valid);
      if (tid < N) last_result = lds.pts[tid][n_valid - 1];
      if (n_valid < G) break;  // reached dist_inter without a collision
      cur = last;
      __syncthreads();         // the points and verdicts are rewritten by the next pass
    }
    completed_walk = !collided;
    if (collided) result = last_result;
    else if (fraction == 1.0) result = b_d;  // exact end fractions (:159-162)
    else if (fraction == 0.0) result = a_d;
    else result = a_d + (b_d - a_d) * fraction;
  }
  if (tid < N) RKH_IO(x_out)[uint64_t(e) * N + tid] = result;
  if (tid == 0) RKH_IO(steps_free)[e] = n_checked;
  if (mode != EDGE_PLAIN) {
    const double n_ar = norm_n(a_d - result);
    const double n_ab = dist_tot;
    const double n_rb = norm_n(result - b_d);
    const int acc = edge_accept(mode, n_ar, n_ab, n_rb, RKH_IO(best_case), e, RKH_IO(steer_tol), completed_walk ? 1 : 0);
    if (tid == 0) {
      if (acc != kNoAccept) RKH_IO(accept)[e] = uint8_t(acc);
      else if (mode == EDGE_GOAL_PROBE)
        RKH_IO(goal_dist)[edge_source_row(RKH_IO(src_idx), RKH_IO(d_src_first), e) - 1] = goal_probe_interpolated(n_ab, n_rb);
    }
  }
#undef RKH_IO
}

// Diagnostic kernel (not on the product path): `iters` back-to-back f-evals + proximity tests of one edge per
// wave, with s_memtime deltas per phase: [sincos, forward sweep, jacobian columns, force sweep, mass matrix,
// cholesky, proximity, total].
template <int N>
__global__ __launch_bounds__(64) void feval_cycles_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                           int n_pairs, const double* __restrict__ x,
                                                           const double* __restrict__ u, int iters,
                                                           unsigned long long* __restrict__ out, double* __restrict__ sink_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BlockLds<N, 64>& lds = *reinterpret_cast<BlockLds<N, 64>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayout<N, 64>::block_bytes);
  const int lane = threadIdx.x;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  stage_env(sc, env_lds, lane);
  GroupWs<N>& ws = lds.g[0];
  double xv = (lane < D) ? x[uint64_t(blockIdx.x) * D + lane] : 0.0;
  if (lane < N) ws.u[lane] = u[uint64_t(blockIdx.x) * N + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool singular = false;
  double acc = 0.0;
  const unsigned long long t_begin = __builtin_readcyclecounter();
  for (int it = 0; it < iters; ++it) {
    if (lane < D) ws.x[lane] = xv;
    __syncthreads();
    const double dp = state_derivative<N, 64>(sc, cp, lds.joints, lds.base, ws, lds.sink[lane], lane, 0, &singular, st);
    xv = xv + 1e-4 * dp;
    if (lane < D) ws.x[lane] = xv;
    __syncthreads();
    const unsigned long long t0 = __builtin_readcyclecounter();
    acc += proximity_min<N, 64>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, lds.sink[lane], lane, 0, true, false);
    st[6] += __builtin_readcyclecounter() - t0;
  }
  st[7] = __builtin_readcyclecounter() - t_begin;
  if (lane == 0) {
    for (int i = 0; i < 8; ++i) out[blockIdx.x * 8 + i] = st[i];
    sink_out[blockIdx.x] = acc + xv + (singular ? 1.0 : 0.0);
  }
}

// Diagnostic kernel (not on the product path): state_derivative_duo, `iters` f-evals of one state per block of two
// waves; row 2 b of `out` = wave 0's stamps, row 2 b + 1 = wave 1's (8 counters each, see state_derivative_duo).
template <int N>
__global__ __launch_bounds__(128) void feval_cycles_duo_kernel(const SceneDev* __restrict__ sc, const double* __restrict__ x,
                                                                const double* __restrict__ u, int iters,
                                                                unsigned long long* __restrict__ out, double* __restrict__ sink_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BlockLds<N, 64>& lds = *reinterpret_cast<BlockLds<N, 64>*>(smem_raw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  GroupWs<N>& ws = lds.g[0];
  double xv = (lane < D) ? x[uint64_t(blockIdx.x) * D + lane] : 0.0;
  if (lane < N) ws.u[lane] = u[uint64_t(blockIdx.x) * N + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool singular = false;
  const unsigned long long t_begin = __builtin_readcyclecounter();
  for (int it = 0; it < iters; ++it) {
    if (lane < D) ws.x[lane] = xv;
    __syncthreads();
    const double dp = state_derivative_duo<N>(sc, cp, lds.joints, lds.base, ws, lds.sink[lane], lane, wave, &singular, st);
    xv = xv + 1e-4 * dp;
  }
  st[7] = __builtin_readcyclecounter() - t_begin;
  if (lane == 0) {
    for (int i = 0; i < 8; ++i) out[(uint64_t(blockIdx.x) * 2 + wave) * 8 + i] = st[i];
    if (wave == 0) sink_out[blockIdx.x] = xv + (singular ? 1.0 : 0.0);
  }
}

// Kernel: exact minimum proxy-pair distance for B states (no culling).
template <int N>
__global__ __launch_bounds__(64) void min_distance_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                           int n_pairs, const double* __restrict__ x, uint32_t B,
                                                           double* __restrict__ dist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BlockLdsQs<N, 64>& lds = *reinterpret_cast<BlockLdsQs<N, 64>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayoutQs<N, 64>::block_bytes);
  const uint32_t e = blockIdx.x;
  if (e >= B) return;
  const int lane = threadIdx.x;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  stage_env(sc, env_lds, lane);
  GroupWsQs<N>& ws = lds.g[0];
  if (lane < D) ws.x[lane] = x[uint64_t(e) * D + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  // (prismatic scenes hold no vertex sets: their form leaves the support-map query out)
  const double dmin = proximity_min<N, 64, GroupWsQs<N>, !kPrismatic, kPrismatic>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws,
                                                                                  lds.sink[lane], lane, 0, false, false);
  if (lane == 0) dist[e] = dmin;
}

#ifdef RKH_PLANAR_PRISMATIC_QS
namespace planar_prismatic {
// min_distance_kernel for planar chains with prismatic_joint_2D groups
template <int N>
__global__ __launch_bounds__(64) void min_distance_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                           int n_pairs, const double* __restrict__ x, uint32_t B,
                                                           double* __restrict__ dist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BlockLdsQs<N, 64>& lds = *reinterpret_cast<BlockLdsQs<N, 64>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayoutQs<N, 64>::block_bytes);
  const uint32_t e = blockIdx.x;
  if (e >= B) return;
  const int lane = threadIdx.x;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  stage_env(sc, env_lds, lane);
  GroupWsQs<N>& ws = lds.g[0];
  if (lane < D) ws.x[lane] = x[uint64_t(e) * D + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  const double dmin = proximity_min_planar<N, 64, true>(sc, cp, lds.base, env_lds, pairs, n_pairs, ws, lane, 0);
  if (lane == 0) dist[e] = dmin;
}
}  // namespace planar_prismatic
#endif

#ifndef RKH_PRISMATIC_FORMS
// ---- record queries (rkh_min_distance_records, rkh_collision_records) -----------------------------------------------
// One form serves revolute and prismatic chains: proximity_frames with PRISM = true reads SceneDev::prismatic_mask at
// run time and does exactly the revolute arithmetic where the bit is clear, so these kernels exist once, here, and
// rkh::prismatic gains none.  Planar scenes never reach them; scenes with vertex-set shapes reach the *_meshes_kernel forms
// (rkh_min_distance_records_meshes, rkh_collision_records_meshes), whose records of such pairs are gjk_record's.

// Pair pr at the frames proximity_frames left in ws: (shape1, shape2) in the finder's own order, and the gap of their
// bounding spheres (transformToGlobal(0) of both shapes, then |c2 - c1| - r1 - r2: proxy_query_model.cpp:384-389,407-411)
template <typename WS>
RKH_DI double record_pair_shapes(const SceneDev* __restrict__ sc, const ShapeDev* __restrict__ env_lds, const WS& ws,
                                 const PairDev pr, ShapeG* s1, ShapeG* s2) {
  const ShapeDev& rs = sc->robot[pr.robot];
  const ShapeDev& es = env_lds[pr.env];
  ShapeG A, Bv;
  A.kind = rs.kind;
  A.pos = ld3(ws.Rpos[pr.robot]);
  A.q = ld4(ws.Rquat[pr.robot]);
  A.d0 = rs.dims[0]; A.d1 = rs.dims[1]; A.d2 = rs.dims[2];
  Bv.kind = es.kind;
  Bv.pos = ld3(es.pos);
  Bv.q = ld4(es.quat);
  Bv.d0 = es.dims[0]; Bv.d1 = es.dims[1]; Bv.d2 = es.dims[2];
  *s1 = pr.s1_is_robot ? A : Bv;
  *s2 = pr.s1_is_robot ? Bv : A;
  const d3 c1 = pose_to_parent(s1->pos, s1->q, mk3(0, 0, 0));
  const d3 c2 = pose_to_parent(s2->pos, s2->q, mk3(0, 0, 0));
  const double r1 = pr.s1_is_robot ? rs.brad : es.brad;
  const double r2 = pr.s1_is_robot ? es.brad : rs.brad;
  return norm_2(c2 - c1) - r1 - r2;
}

// The three modes of the record kernels: closed forms only; vertex-set pairs through gjk_distance / gjk_record; the same
// pairs through gjk_depth_distance / gjk_depth_record (a penetration depth where the cores cross, and a normal with
// every record: pair_distance_depth / pair_record_depth).
constexpr int kRecClosed = 0, kRecGjk = 1, kRecDepth = 2;

template <int MODE>
RKH_DI double record_pair_distance(int routine, const ShapeG& s1, const ShapeG& s2, const double* __restrict__ mesh_pool) {
  if constexpr (MODE == kRecDepth) return pair_distance_depth(routine, s1, s2, mesh_pool);
  else return pair_distance<MODE == kRecGjk>(routine, s1, s2, mesh_pool);
}

// slot `at` of the record arrays: the record of pair p (p < 0: no record).  kRecGjk, kRecDepth: vertex-set pairs among
// them, answered from mesh_pool; kRecDepth: three doubles of normal as well (zeros without a record), and the dist of a
// vertex-set pair is its record's own -- gjk_depth_distance's value bit for bit, so a caller need not search twice
template <int MODE = kRecClosed, typename WS>
RKH_DI void write_pair_record(const SceneDev* __restrict__ sc, const ShapeDev* __restrict__ env_lds, const WS& ws,
                              const PairDev* __restrict__ pairs, const PairIdDev* __restrict__ ids, int p, const RecordOut& out,
                              uint64_t at, double dist, const double* __restrict__ mesh_pool = nullptr,
                              double* __restrict__ normal = nullptr) {
  ProxRecordG r;
  r.p1 = r.p2 = mk3(0.0, 0.0, 0.0);
  uint32_t id1 = 0xFFFFFFFFu, id2 = 0xFFFFFFFFu;
  if constexpr (MODE == kRecDepth) {
    d3 nrm = mk3(0.0, 0.0, 0.0);
    if (p >= 0) {
      const PairDev pr = pairs[p];
      ShapeG s1, s2;
      record_pair_shapes(sc, env_lds, ws, pr, &s1, &s2);
      const ProxRecordN rn = pair_record_depth(pr.routine, s1, s2, mesh_pool);
      r.p1 = rn.p1;
      r.p2 = rn.p2;
      nrm = rn.nrm;
      if (pr.routine == PR_GJK) dist = rn.dist;
      id1 = ids[p].shape1;
      id2 = ids[p].shape2;
    }
    st3(normal + 3 * at, nrm);
  } else if (p >= 0) {
    const PairDev pr = pairs[p];
    ShapeG s1, s2;
    record_pair_shapes(sc, env_lds, ws, pr, &s1, &s2);
    if constexpr (MODE == kRecGjk) r = pair_record<true>(pr.routine, s1, s2, mesh_pool);
    else r = pair_record(pr.routine, s1, s2);
    id1 = ids[p].shape1;
    id2 = ids[p].shape2;
  }
  out.dist[at] = dist;  // the distance the pair was found with (pair_distance), not the point form's own
  st3(out.point1 + 3 * at, r.p1);
  st3(out.point2 + 3 * at, r.p2);
  out.shape1[at] = id1;
  out.shape2[at] = id2;
}

// Kernel: proxy_query_pair_3D::findMinimumDistance()->getLastResult() for B states, one wave per state.  Every lane
// walks its pairs as min_distance_kernel does and keeps two things: the running minimum with that kernel's own
// comparison (so dist is its value bit for bit), and its best (distance, finder rank) in lexicographic order -- the
// reference's loop takes a new minimum only on a strictly smaller distance, so among equal distances the earliest
// finder stays.  A butterfly leaves the wave's winner in every lane; lane 0 evaluates that one pair's point form.
// GJK = true is the form for scenes with vertex-set shapes: it searches with the support-map query as min_distance_kernel
// does there, and lane 0 evaluates the winner's record with gjk_record where the winner is such a pair.  The two forms
// are kernels of their own names (the closed-form one keeps the name and the code it had).  MODE = kRecDepth is the
// third form (min_distance_depth_kernel, in propagate_depth.hip's module): the same search over pair_distance_depth, so
// among crossing vertex-set pairs the deepest wins, and lane 0 writes the winner's normal too.
template <int N, int MODE>
RKH_DI void min_distance_records_body(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                      const PairIdDev* __restrict__ ids, int n_pairs, const double* __restrict__ x, uint32_t B,
                                      const RecordOut& out, double* __restrict__ normal = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const double* mesh_pool = MODE != kRecClosed ? sc->mesh_verts : nullptr;
  BlockLdsQs<N, 64>& lds = *reinterpret_cast<BlockLdsQs<N, 64>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayoutQs<N, 64>::block_bytes);
  const uint32_t e = blockIdx.x;
  if (e >= B) return;
  const int lane = threadIdx.x;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  stage_env(sc, env_lds, lane);
  GroupWsQs<N>& ws = lds.g[0];
  if (lane < D) ws.x[lane] = x[uint64_t(e) * D + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  proximity_frames<N, 64, GroupWsQs<N>, true>(sc, sc->robot, cp, lds.base, ws, lds.sink[lane], lane);
  double dmin = INFINITY;
  double dbest = INFINITY;
  uint32_t rbest = 0xFFFFFFFFu;
  int pbest = -1;
  for (int p = lane; p < n_pairs; p += 64) {
    const PairDev pr = pairs[p];
    ShapeG s1, s2;
    record_pair_shapes(sc, env_lds, ws, pr, &s1, &s2);
    const double d = record_pair_distance<MODE>(pr.routine, s1, s2, mesh_pool);
    if (d < dmin) dmin = d;
    const uint32_t rank = ids[p].rank;
    if (d < dbest || (d == dbest && rank < rbest)) {
      dbest = d;
      rbest = rank;
      pbest = p;
    }
  }
  // all lanes are here: the cross-lane reads below run in uniform control flow
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(dmin, off, 64);
    if (o < dmin) dmin = o;
    const double od = __shfl_xor(dbest, off, 64);
    const uint32_t orank = uint32_t(__shfl_xor(int(rbest), off, 64));
    const int op = __shfl_xor(pbest, off, 64);
    if (od < dbest || (od == dbest && orank < rbest)) {
      dbest = od;
      rbest = orank;
      pbest = op;
    }
  }
  if (lane == 0) write_pair_record<MODE>(sc, env_lds, ws, pairs, ids, pbest, out, e, dmin, mesh_pool, normal);
}

template <int N>
__global__ __launch_bounds__(64) void min_distance_records_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                                   const PairIdDev* __restrict__ ids, int n_pairs,
                                                                   const double* __restrict__ x, uint32_t B, RecordOut out) {
  min_distance_records_body<N, kRecClosed>(sc, pairs, ids, n_pairs, x, B, out);
}

template <int N>
__global__ __launch_bounds__(64) void min_distance_records_meshes_kernel(const SceneDev* __restrict__ sc,
                                                                          const PairDev* __restrict__ pairs,
                                                                          const PairIdDev* __restrict__ ids, int n_pairs,
                                                                          const double* __restrict__ x, uint32_t B, RecordOut out) {
  min_distance_records_body<N, kRecGjk>(sc, pairs, ids, n_pairs, x, B, out);
}

// Kernel: proxy_query_pair_3D::gatherCollisionPoints for B states, one wave per state.  Every lane culls and measures
// its pairs (bounding spheres apart: skipped; distance < 0: a collision) and keeps one bit per collision -- pair
// p = 64 s + lane is bit s of (m0, m1), kMaxRecordPairs pairs at most.  The collisions leave in finder order: min(n_found,
// cap) rounds, each a butterfly over every lane's lowest remaining rank; lane 0 evaluates the round's point form and
// the owner drops its bit.  The round count is wave-uniform, so the butterflies run in uniform control flow.
// GJK = true: the form for scenes with vertex-set shapes, as for the minimum-distance records; only lane 0 runs
// gjk_record, between the rounds' butterflies and never around them.  MODE = kRecDepth (collision_depth_kernel): the
// same pairs in the same order (the depth mode keeps the collision mark), their records with depth and normal.
template <int N, int MODE>
RKH_DI void collision_records_body(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                   const PairIdDev* __restrict__ ids, int n_pairs, const double* __restrict__ x, uint32_t B,
                                   uint32_t cap, const RecordOut& out, double* __restrict__ normal = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const double* mesh_pool = MODE != kRecClosed ? sc->mesh_verts : nullptr;
  BlockLdsQs<N, 64>& lds = *reinterpret_cast<BlockLdsQs<N, 64>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayoutQs<N, 64>::block_bytes);
  const uint32_t e = blockIdx.x;
  if (e >= B) return;
  const int lane = threadIdx.x;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  stage_env(sc, env_lds, lane);
  GroupWsQs<N>& ws = lds.g[0];
  if (lane < D) ws.x[lane] = x[uint64_t(e) * D + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  proximity_frames<N, 64, GroupWsQs<N>, true>(sc, sc->robot, cp, lds.base, ws, lds.sink[lane], lane);
  unsigned long long m0 = 0ull, m1 = 0ull;
  for (int p = lane; p < n_pairs; p += 64) {
    const PairDev pr = pairs[p];
    ShapeG s1, s2;
    const double gap = record_pair_shapes(sc, env_lds, ws, pr, &s1, &s2);
    if (gap > 0.0) continue;
    // (kRecDepth: the depth mode keeps the collision mark, so gjk_distance gives its verdict without the expansion)
    constexpr int VMODE = MODE == kRecDepth ? kRecGjk : MODE;
    if (record_pair_distance<VMODE>(pr.routine, s1, s2, mesh_pool) < 0.0) {
      const int s = p >> 6;
      if (s < 64) m0 |= 1ull << s;
      else m1 |= 1ull << (s - 64);
    }
  }
  uint32_t total = uint32_t(__popcll(m0) + __popcll(m1));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) total += uint32_t(__shfl_xor(int(total), off, 64));
  if (lane == 0) out.n_found[e] = total;
  const uint32_t n_out = total < cap ? total : cap;
  const uint64_t row = uint64_t(e) * cap;
  for (uint32_t k = 0; k < n_out; ++k) {
    uint32_t rmin = 0xFFFFFFFFu;
    int pmin = -1;
    for (unsigned long long mm = m0; mm != 0ull; mm &= mm - 1ull) {
      const int p = ((__ffsll((long long)mm) - 1) << 6) + lane;
      const uint32_t r = ids[p].rank;
      if (r < rmin) rmin = r, pmin = p;
    }
    for (unsigned long long mm = m1; mm != 0ull; mm &= mm - 1ull) {
      const int p = ((__ffsll((long long)mm) - 1 + 64) << 6) + lane;
      const uint32_t r = ids[p].rank;
      if (r < rmin) rmin = r, pmin = p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t orank = uint32_t(__shfl_xor(int(rmin), off, 64));
      const int op = __shfl_xor(pmin, off, 64);
      if (orank < rmin) rmin = orank, pmin = op;
    }
    // (k < total: some lane held a bit, so pmin names a pair)
    if (lane == (pmin & 63)) {
      const int s = pmin >> 6;
      if (s < 64) m0 &= ~(1ull << s);
      else m1 &= ~(1ull << (s - 64));
    }
    if (lane == 0) {
      const PairDev pr = pairs[pmin];
      ShapeG s1, s2;
      record_pair_shapes(sc, env_lds, ws, pr, &s1, &s2);
      // (kRecDepth: a vertex-set pair's dist comes with its record, see write_pair_record)
      constexpr int DMODE = MODE == kRecDepth ? kRecClosed : MODE;
      write_pair_record<MODE>(sc, env_lds, ws, pairs, ids, pmin, out, row + k,
                              record_pair_distance<DMODE>(pr.routine, s1, s2, mesh_pool), mesh_pool, normal);
    }
  }
  for (uint32_t k = n_out + lane; k < cap; k += 64)
    write_pair_record<MODE>(sc, env_lds, ws, pairs, ids, -1, out, row + k, INFINITY, mesh_pool, normal);
}

template <int N>
__global__ __launch_bounds__(64) void collision_records_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                                const PairIdDev* __restrict__ ids, int n_pairs,
                                                                const double* __restrict__ x, uint32_t B, uint32_t cap,
                                                                RecordOut out) {
  collision_records_body<N, kRecClosed>(sc, pairs, ids, n_pairs, x, B, cap, out);
}

template <int N>
__global__ __launch_bounds__(64) void collision_records_meshes_kernel(const SceneDev* __restrict__ sc,
                                                                       const PairDev* __restrict__ pairs,
                                                                       const PairIdDev* __restrict__ ids, int n_pairs,
                                                                       const double* __restrict__ x, uint32_t B, uint32_t cap,
                                                                       RecordOut out) {
  collision_records_body<N, kRecGjk>(sc, pairs, ids, n_pairs, x, B, cap, out);
}

#ifdef RKH_DEPTH_RECORDS
// The depth forms of the two record kernels, and the pair-by-pair form of the diagnostic entry (rkh_diag_gjk_depth_records).
// propagate_depth.hip instantiates these three and nothing else of this text.
template <int N>
__global__ __launch_bounds__(64) void min_distance_depth_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                                 const PairIdDev* __restrict__ ids, int n_pairs,
                                                                 const double* __restrict__ x, uint32_t B, RecordOut out,
                                                                 double* __restrict__ normal) {
  min_distance_records_body<N, kRecDepth>(sc, pairs, ids, n_pairs, x, B, out, normal);
}

template <int N>
__global__ __launch_bounds__(64) void collision_depth_kernel(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                                              const PairIdDev* __restrict__ ids, int n_pairs,
                                                              const double* __restrict__ x, uint32_t B, uint32_t cap, RecordOut out,
                                                              double* __restrict__ normal) {
  collision_records_body<N, kRecDepth>(sc, pairs, ids, n_pairs, x, B, cap, out, normal);
}

__global__ __launch_bounds__(64) void gjk_pair_depth_kernel(const rkh_shape* __restrict__ a, const rkh_shape* __restrict__ b,
                                                             uint32_t n, const double* __restrict__ pool, double* __restrict__ dist,
                                                             double* __restrict__ point1, double* __restrict__ point2,
                                                             double* __restrict__ normal) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  auto conv = [](const rkh_shape& s) {
    ShapeG g;
    g.kind = s.kind;
    g.pos = mk3(s.pose.pos[0], s.pose.pos[1], s.pose.pos[2]);
    g.q = d4{s.pose.quat[0], s.pose.quat[1], s.pose.quat[2], s.pose.quat[3]};
    g.d0 = s.dims[0]; g.d1 = s.dims[1]; g.d2 = s.dims[2];
    return g;
  };
  const ProxRecordN r = pair_record_depth(PR_GJK, conv(a[i]), conv(b[i]), pool);
  dist[i] = r.dist;
  st3(point1 + 3 * size_t(i), r.p1);
  st3(point2 + 3 * size_t(i), r.p2);
  st3(normal + 3 * size_t(i), r.nrm);
}
#endif  // RKH_DEPTH_RECORDS
#endif  // !RKH_PRISMATIC_FORMS

// ---- host launchers ------------------------------------------------------------------------
// Written once for both joint kinds: the prismatic translation unit compiles them in rkh::prismatic for its chain sizes
// and without the duo, 16-lane, support-map and planar forms; the revolute launchers hand scenes with prismatic joints on.
template <class F>
static rkh_status with_chain_n(int n, F&& f) {
  if constexpr (kPrismatic) return with_n<1, 2, 3, 4, 6, 7>(n, f);
  else return with_n<1, 2, 3, 4, 6, 7, 12>(n, f);
}

template <int GL, bool GJK, bool DUO = false>
static rkh_status launch_propagate_t(hipStream_t s, const rkh_scene& scene, const DynDev& dyn, const EdgeIO& io,
                                     uint32_t edges_a, uint32_t edges_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                                     uint32_t n_problems, KernelGate gate) {
  constexpr uint32_t G = 64 / GL;
  const uint32_t ga = (edges_a + G - 1) / G, gbk = (edges_b + G - 1) / G;
  dim3 grid(ga + gbk, n_problems);
  if (gate.wave_base) {
    // compact mapping (G = 1): the kernel only runs while the round has fewer than gate.hi edges in total, so that many
    // blocks are enough -- instead of (bound per problem) x problems blocks that find nothing when the gate is closed
    const uint64_t all = uint64_t(ga + gbk) * n_problems;
    grid = dim3(uint32_t(std::min<uint64_t>(all, gate.hi)), 1);
  }
  WaveArgs args;
  args.sc = scene.d_scene.get();
  args.pairs = scene.d_pairs.get();
  args.n_pairs = scene.n_pairs_verdict;
  args.dyn = dyn;
  args.io_a = io;
  args.io_b = EdgeIO();
  args.tab_a = tab_a;
  args.tab_b = tab_b;
  args.grid_a = ga;
  args.gate = gate;
  return with_chain_n(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((propagate_kernel<N, GL, GJK, DUO>), grid, dim3(DUO ? 128 : 64),
                       (SmemLayout<N, GL>::bytes(scene.host.n_env)), s, args);
  });
}

#ifndef RKH_FORMS_ONLY
rkh_status launch_propagate(hipStream_t s, const rkh_scene& scene, SteerMapping m, const DynDev& dyn, const EdgeIO& io,
                            uint32_t grid_edges, uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                            uint32_t n_problems, double* d_lane_ws, KernelGate gate) {
  const uint32_t eb = tab_b ? grid_b : 0u;
  if (grid_edges + eb == 0 || n_problems == 0) return RKH_OK;
  rkh_status st;
  if constexpr (kPrismatic) {
    st = launch_propagate_t<64, false>(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, gate);
  } else {
    // a scene with prismatic joints never reaches a revolute form: whatever one-wave mapping was asked for is theirs
    // (planar chains with prismatic joints have forms of their own behind launch_propagate_planar)
    if (scene.host.has_prismatic && !scene.host.planar && m != SteerMapping::Pair) m = SteerMapping::Prismatic;
    switch (m) {
      case SteerMapping::Planar:
        return launch_propagate_planar(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, gate);
      case SteerMapping::Prismatic:
        return prismatic::launch_propagate(s, scene, m, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, d_lane_ws, gate);
      case SteerMapping::Pair:
        return rkh::launch_propagate_pairs(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, d_lane_ws, gate);
      case SteerMapping::Duo:
        st = launch_propagate_t<64, false, true>(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, gate);
        break;
      case SteerMapping::Wave16:
        st = launch_propagate_t<16, true>(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, gate);
        break;
      default:  // Wave; without vertex-set shapes the instantiation without the support-map query (no private segment)
        st = scene.host.has_meshes
                 ? launch_propagate_t<64, true>(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, gate)
                 : launch_propagate_t<64, false>(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, gate);
    }
  }
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

rkh_status launch_state_derivative(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                                   double* d_pd, double* d_M, double* d_f, int* d_err) {
  if (B == 0) return RKH_OK;
  if constexpr (!kPrismatic) {
    if (scene.host.planar) return launch_state_derivative_planar(s, scene, d_x, d_u, B, d_pd, d_M, d_f, d_err);
    if (scene.host.has_prismatic) return prismatic::launch_state_derivative(s, scene, d_x, d_u, B, d_pd, d_M, d_f, d_err);
  }
  const rkh_status st = with_chain_n(scene.host.n_dof, [&](auto c) {
    hipLaunchKernelGGL((state_derivative_kernel<decltype(c)::value>), dim3(B), dim3(64), 0, s, scene.d_scene.get(), d_x, d_u, B,
                       d_pd, d_M, d_f, d_err);
  });
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}
#endif  // !RKH_FORMS_ONLY

// The number of waves W of a planar edge_check_kernel launch, by the number of edges (1 for launches of 4096 edges and
// more, 4 below that, 8 below 512) and by what fits 64 KB of LDS (2 where 4 does not fit, 1 where neither does), and
// whether the pair list rides in LDS too.
template <int N>
static int edge_check_shape(int n_env, int n_pairs, uint64_t n_edges, int* staged) {
  auto fit = [&](size_t with_pairs, size_t without) { return with_pairs <= 65536 ? 2 : (without <= 65536 ? 1 : 0); };
  const int f1 = fit(SmemLayoutQsW<N, 1>::bytes(n_env, n_pairs), SmemLayoutQsW<N, 1>::bytes(n_env, 0));
  const int f2 = fit(SmemLayoutQsW<N, 2>::bytes(n_env, n_pairs), SmemLayoutQsW<N, 2>::bytes(n_env, 0));
  const int f4 = fit(SmemLayoutQsW<N, 4>::bytes(n_env, n_pairs), SmemLayoutQsW<N, 4>::bytes(n_env, 0));
  const int f8 = fit(SmemLayoutQsW<N, 8>::bytes(n_env, n_pairs), SmemLayoutQsW<N, 8>::bytes(n_env, 0));
  int w = 1;
  *staged = f1 == 2;
  if (n_edges < 4096) {
    if (f4) w = 4, *staged = f4 == 2;
    else if (f2) w = 2, *staged = f2 == 2;
  }
  if (n_edges < 512 && f8) w = 8, *staged = f8 == 2;
  return w;
}

template <int N, int W>
static void launch_edge_check_t(hipStream_t s, dim3 grid, int n_env, const EdgeWalkArgs& ka) {
  hipLaunchKernelGGL((edge_check_kernel<N, W>), grid, dim3(64 * W),
                     (SmemLayoutQsW<N, W>::bytes(n_env, ka.pairs_staged ? ka.n_pairs : 0)), s, ka);
}

template <int N, bool GJK, int G>
static rkh_status launch_edge_points_t(hipStream_t s, dim3 grid, int n_env, EdgeWalkArgs ka) {
  // a scene holds fewer than kMaxEnvShapes environment shapes: they always fit next to the block's data
  static_assert(EdgePointsSmem<N, G>::bytes(kMaxEnvShapes, 0) <= 160 * 1024, "edge_points_kernel: LDS over 160 KB");
  const size_t with_pairs = EdgePointsSmem<N, G>::bytes(n_env, ka.n_pairs);
  ka.pairs_staged = with_pairs <= 160 * 1024;
  const size_t smem = ka.pairs_staged ? with_pairs : EdgePointsSmem<N, G>::bytes(n_env, 0);
  auto kern = edge_points_kernel<N, GJK, G>;
  static bool big_lds = false;  // (per instantiation) more than the default 64 KB of dynamic LDS: ask once
  if (smem > 65536 && !big_lds) {
    RKH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    big_lds = true;
  }
  hipLaunchKernelGGL(kern, grid, dim3(256), smem, s, ka);
  return RKH_OK;
}

// The form of a quasi-static edge walk launch.  3D scenes: edge_points_kernel, 64 points per pass for launches of fewer
// than 2048 edges and chains of at most 7 joints, 32 otherwise, the support-map query only for scenes with vertex-set
// shapes.  Planar scenes: edge_check_kernel with edge_check_shape's W.  Both stage the pair list in LDS if it fits.
template <int N>
static rkh_status launch_edge_walk(hipStream_t s, dim3 grid, const rkh_scene& scene, const EdgeWalkArgs& ka) {
  const int n_env = scene.host.n_env;
  const uint64_t n_edges = uint64_t(grid.x) * grid.y;
  constexpr int GW = N <= 7 ? 64 : 32;
  const bool wide = n_edges < 2048;
  if constexpr (!kPrismatic) {
    if (scene.host.planar) {
      EdgeWalkArgs pa = ka;
      switch (edge_check_shape<N>(n_env, ka.n_pairs, n_edges, &pa.pairs_staged)) {
        case 8: launch_edge_check_t<N, 8>(s, grid, n_env, pa); break;
        case 4: launch_edge_check_t<N, 4>(s, grid, n_env, pa); break;
        case 2: launch_edge_check_t<N, 2>(s, grid, n_env, pa); break;
        default: launch_edge_check_t<N, 1>(s, grid, n_env, pa); break;
      }
      return RKH_OK;
    }
    if (scene.host.has_meshes)
      return wide ? launch_edge_points_t<N, true, GW>(s, grid, n_env, ka) : launch_edge_points_t<N, true, 32>(s, grid, n_env, ka);
  }
  return wide ? launch_edge_points_t<N, false, GW>(s, grid, n_env, ka) : launch_edge_points_t<N, false, 32>(s, grid, n_env, ka);
}

#ifndef RKH_PRISMATIC_FORMS
// the checks and the chain-size dispatch of every record launch (the depth forms' too)
template <class F>
static rkh_status launch_records(const rkh_scene& scene, bool meshes, F&& f) {
  if (scene.host.planar || (scene.host.has_meshes && !meshes) || !scene.d_pair_ids.get() || scene.n_pairs > kMaxRecordPairs) {
    set_error(meshes ? "record queries: 3D scenes only" : "record queries: 3D scenes without vertex-set shapes only");
    return RKH_ERR_UNSUPPORTED;
  }
  RKH_TRY((with_n<1, 2, 3, 4, 6, 7, 12>(scene.host.n_dof, f)));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}
#endif

#ifdef RKH_DEPTH_RECORDS
// The launchers of the depth forms (this translation unit holds nothing else).  A scene without vertex-set shapes has
// no pair for them to answer differently, but its records still gain their normals: the same kernels serve it.
rkh_status launch_min_distance_records_depth(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, RecordOut out,
                                             double* d_normal) {
  if (B == 0) return RKH_OK;
  return launch_records(scene, true, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((min_distance_depth_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, out, d_normal);
  });
}

rkh_status launch_collision_records_depth(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, uint32_t cap,
                                          RecordOut out, double* d_normal) {
  if (B == 0) return RKH_OK;
  return launch_records(scene, true, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((collision_depth_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, cap, out, d_normal);
  });
}

rkh_status launch_gjk_pair_depth(hipStream_t s, const rkh_shape* d_a, const rkh_shape* d_b, uint32_t n, const double* d_pool,
                                 double* d_dist, double* d_point1, double* d_point2, double* d_normal) {
  if (n == 0) return RKH_OK;
  hipLaunchKernelGGL(gjk_pair_depth_kernel, dim3((n + 63) / 64), dim3(64), 0, s, d_a, d_b, n, d_pool, d_dist, d_point1, d_point2,
                     d_normal);
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}
#elif defined(RKH_PLANAR_PRISMATIC_QS)
// The two launchers of the planar prismatic position-level forms (this translation unit holds nothing else).
namespace planar_prismatic {
template <int N, int W>
static void launch_edge_check_w(hipStream_t s, dim3 grid, int n_env, const EdgeWalkArgs& ka) {
  hipLaunchKernelGGL((edge_check_kernel<N, W>), grid, dim3(64 * W),
                     (SmemLayoutQsW<N, W>::bytes(n_env, ka.pairs_staged ? ka.n_pairs : 0)), s, ka);
}

rkh_status launch_edge_check(hipStream_t s, const rkh_scene& scene, const QsDev& qs, const EdgeIO& io, uint32_t grid_edges,
                             uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b, uint32_t n_problems) {
  const uint32_t eb = tab_b ? grid_b : 0u;
  if (grid_edges + eb == 0 || n_problems == 0) return RKH_OK;
  EdgeWalkArgs ka;
  ka.sc = scene.d_scene.get();
  ka.pairs = scene.d_pairs.get();
  ka.n_pairs = scene.n_pairs_verdict;
  ka.qs = qs;
  ka.io_a = io;
  ka.io_b = EdgeIO();
  ka.tab_a = tab_a;
  ka.tab_b = tab_b;
  ka.grid_a = grid_edges;
  ka.pairs_staged = 0;
  const dim3 grid(grid_edges + eb, n_problems);
  const int n_env = scene.host.n_env;
  RKH_TRY((with_n<1, 2, 3, 4, 6, 7>(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    switch (edge_check_shape<N>(n_env, ka.n_pairs, uint64_t(grid.x) * grid.y, &ka.pairs_staged)) {  // the revolute rule
      case 8: launch_edge_check_w<N, 8>(s, grid, n_env, ka); break;
      case 4: launch_edge_check_w<N, 4>(s, grid, n_env, ka); break;
      case 2: launch_edge_check_w<N, 2>(s, grid, n_env, ka); break;
      default: launch_edge_check_w<N, 1>(s, grid, n_env, ka); break;
    }
  })));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

rkh_status launch_min_distance(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, double* d_dist) {
  if (B == 0) return RKH_OK;
  RKH_TRY((with_n<1, 2, 3, 4, 6, 7>(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((min_distance_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.n_pairs, d_x, B, d_dist);
  })));
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}
}  // namespace planar_prismatic
#else  // the unit's own launchers
rkh_status launch_edge_check(hipStream_t s, const rkh_scene& scene, const QsDev& qs, const EdgeIO& io, uint32_t grid_edges,
                             uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b, uint32_t n_problems) {
  const uint32_t eb = tab_b ? grid_b : 0u;
  if (grid_edges + eb == 0 || n_problems == 0) return RKH_OK;
  if constexpr (!kPrismatic) {
    if (scene.host.has_prismatic && scene.host.planar)
      return planar_prismatic::launch_edge_check(s, scene, qs, io, grid_edges, eb, tab_a, tab_b, n_problems);
    if (scene.host.has_prismatic)
      return prismatic::launch_edge_check(s, scene, qs, io, grid_edges, eb, tab_a, tab_b, n_problems);
  }
  EdgeWalkArgs ka;
  ka.sc = scene.d_scene.get();
  ka.pairs = scene.d_pairs.get();
  ka.n_pairs = scene.n_pairs_verdict;
  ka.qs = qs;
  ka.io_a = io;
  ka.io_b = EdgeIO();
  ka.tab_a = tab_a;
  ka.tab_b = tab_b;
  ka.grid_a = grid_edges;
  ka.pairs_staged = 0;
  const dim3 grid(grid_edges + eb, n_problems);
  rkh_status st = RKH_OK;
  const rkh_status sn =
      with_chain_n(scene.host.n_dof, [&](auto c) { st = launch_edge_walk<decltype(c)::value>(s, grid, scene, ka); });
  if (sn != RKH_OK) return sn;
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

#ifndef RKH_PRISMATIC_FORMS  // the f-eval cycle probes instrument the revolute forms only
rkh_status launch_feval_cycles_duo(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                                   int iters, unsigned long long* d_out, double* d_sink) {
  if (scene.host.has_prismatic) {
    set_error("rkh_diag_feval_cycles: scenes with prismatic joints are not instrumented");
    return RKH_ERR_UNSUPPORTED;
  }
  const rkh_status st = with_chain_n(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((feval_cycles_duo_kernel<N>), dim3(B / 2), dim3(128), (SmemLayout<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), d_x, d_u, iters, d_out, d_sink);
  });
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

rkh_status launch_feval_cycles(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                               int iters, unsigned long long* d_out, double* d_sink) {
  if (scene.host.has_prismatic) {
    set_error("rkh_diag_feval_cycles: scenes with prismatic joints are not instrumented");
    return RKH_ERR_UNSUPPORTED;
  }
  const rkh_status st = with_chain_n(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((feval_cycles_kernel<N>), dim3(B), dim3(64), (SmemLayout<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.n_pairs, d_x, d_u, iters, d_out,
                       d_sink);
  });
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}
#endif

rkh_status launch_min_distance(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, double* d_dist) {
  if (B == 0) return RKH_OK;
  if constexpr (!kPrismatic) {
    if (scene.host.has_prismatic && scene.host.planar) return planar_prismatic::launch_min_distance(s, scene, d_x, B, d_dist);
    if (scene.host.has_prismatic) return prismatic::launch_min_distance(s, scene, d_x, B, d_dist);
  }
  const rkh_status st = with_chain_n(scene.host.n_dof, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((min_distance_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.n_pairs, d_x, B, d_dist);
  });
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

#ifndef RKH_PRISMATIC_FORMS  // the record kernels exist once and serve both joint kinds (see above)
rkh_status launch_min_distance_records(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, RecordOut out) {
  if (B == 0) return RKH_OK;
  return launch_records(scene, false, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((min_distance_records_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, out);
  });
}

rkh_status launch_collision_records(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, uint32_t cap,
                                    RecordOut out) {
  if (B == 0) return RKH_OK;
  return launch_records(scene, false, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((collision_records_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)), s,
                       scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, cap, out);
  });
}

// The same for every 3D scene: with vertex-set shapes the support-map forms, without them the kernels above
rkh_status launch_min_distance_records_meshes(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, RecordOut out) {
  if (!scene.host.has_meshes) return launch_min_distance_records(s, scene, d_x, B, out);
  if (B == 0) return RKH_OK;
  return launch_records(scene, true, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((min_distance_records_meshes_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)),
                       s, scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, out);
  });
}

rkh_status launch_collision_records_meshes(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B, uint32_t cap,
                                           RecordOut out) {
  if (!scene.host.has_meshes) return launch_collision_records(s, scene, d_x, B, cap, out);
  if (B == 0) return RKH_OK;
  return launch_records(scene, true, [&](auto c) {
    constexpr int N = decltype(c)::value;
    hipLaunchKernelGGL((collision_records_meshes_kernel<N>), dim3(B), dim3(64), (SmemLayoutQs<N, 64>::bytes(scene.host.n_env)),
                       s, scene.d_scene.get(), scene.d_pairs.get(), scene.d_pair_ids.get(), scene.n_pairs, d_x, B, cap, out);
  });
}
#endif

#endif  // RKH_DEPTH_RECORDS / RKH_PLANAR_PRISMATIC_QS / the unit's own launchers

#ifdef RKH_PRISMATIC_FORMS
}  // namespace prismatic
#endif
}  // namespace rkh
