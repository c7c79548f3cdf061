// propagate_pair.hip -- the throughput mapping of the steer kernel: TWO ADJACENT LANES PER CANDIDATE EDGE, 32 edges per
// wave, TWO WAVES PER SIMD (gfx950, wave64).
//
// Same function and same arithmetic as propagate_kernel (propagate.hip; reference citations there): RK4 forward
// dynamics of the KTE serial chain under the held PD input, proximity test after every step, accept test / goal probe
// at the end; every product and sum is formed in the reference's order (-ffp-contract=off), so the kernels return
// bit-identical states and verdicts (tests/test_gpu_parity.py::test_propagate_mappings_*).
//
// The mapping keeps the VALU busy with registers and DPP instead of LDS round trips:
//   * lane (el, h) = (lane >> 1, lane & 1): the edge's two lanes are neighbours, so they exchange values with a DPP
//     quad_perm move (one VALU instruction per 32 bits, no LDS, no select);
//   * the Jacobian columns of the current body live in REGISTERS: lane h computes the columns of the joints c = 2r + h
//     (r unrolled: static register indices), from the end frames of those joints, which it also keeps in registers
//     (a lane only ever needs the frames of its own columns): of a frame (p, q) it keeps q and (-p) * rotmat(q);
//   * the mass matrix is accumulated in REGISTERS: lane h owns the rows i = 2r + h; Mcm * T of its own columns is formed
//     once per body and handed to the neighbour by DPP, so each lane has all columns' products for its rows.  Every
//     M(i, jx) receives its terms in the same ascending-body order (mat_alg_symmetric.hpp:551-566) -- no LDS
//     read-modify-write chain;
//   * LDS per edge is 75 slots (state 2N, cos / sin 2N, input N, generalized forces N, and one region shared in time by
//     the link forces (6N), the joint frames of the proximity test (7N - 3) and the assembled mass matrix (N^2))
//     = 19.3 KB per wave: eight waves per CU;
//   * the RK4 stage vectors are split between the edge's lanes (lane h updates the joints 2r + h).
//
// Chains with prismatic joints (SceneDev::has_prismatic) run on forms compiled from this same text in a translation unit
// of their own (propagate_pair_prismatic.hip defines RKH_PRISMATIC_FORMS and includes this file): there the kernels and
// their launchers live in rkh::prismatic and kPrismatic is true.  Here kPrismatic is false and the prismatic branches
// compile away, so the revolute kernels keep their code; the launchers below hand prismatic scenes on.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "device_math.h"
#include "proximity_device.h"
#include "rkh_internal.h"
#include "round_carry.h"

namespace rkh {
#ifdef RKH_PRISMATIC_FORMS
namespace prismatic {
constexpr bool kPrismatic = true;
#else
constexpr bool kPrismatic = false;
#endif

namespace {

// The scene is read through a constant-address-space pointer: uniform addresses then always become scalar loads, also
// behind the laundering below (a laundered generic pointer would turn them into per-lane flat loads).
typedef const __attribute__((address_space(4))) SceneDev* ScenePtr;
typedef const __attribute__((address_space(4))) double* CDoubleP;
RKH_DI d3 ldg3(CDoubleP p) { return d3{p[0], p[1], p[2]}; }
RKH_DI d4 ldg4(CDoubleP p) { return d4{p[0], p[1], p[2], p[3]}; }
RKH_DI m33 ldgm(CDoubleP p) { return m33{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]}; }
struct Sym6 {
  double t[6];
};
RKH_DI Sym6 ldsym(CDoubleP p) { return Sym6{{p[0], p[1], p[2], p[3], p[4], p[5]}}; }

RKH_DI float readlane_f(float v, int src_lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}

// the value the edge's other lane holds (lane ^ 1): v_mov_b32_dpp quad_perm:[1,0,3,2]
RKH_DI int xchg_i(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true); }
RKH_DI double xchg(double v) {
  const int lo = xchg_i(__double2loint(v));
  const int hi = xchg_i(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
RKH_DI d3 xchg3(d3 v) { return d3{xchg(v.x), xchg(v.y), xchg(v.z)}; }

RKH_DI m33 pair_axis_angle_rotmat(double ca, double sa, d3 ax) {  // axis_angle::getRotMat (rotations_3D.hpp:2160-2180)
  const double omc = 1.0 - ca;
  const double t11 = ca + omc * ax.x * ax.x, t22 = ca + omc * ax.y * ax.y, t33 = ca + omc * ax.z * ax.z;
  const double t12 = omc * ax.x * ax.y, t13 = omc * ax.x * ax.z, t23 = omc * ax.y * ax.z;
  const double t01 = sa * ax.x, t02 = sa * ax.y, t03 = sa * ax.z;
  return m33{t11, t12 - t03, t13 + t02, t12 + t03, t22, t23 - t01, t13 - t02, t23 + t01, t33};
}

constexpr int kPairEdges = 32;  // edges per wave: every lane in use

// The two lanes of an edge hand values over through LDS without a barrier: one lane stores under a condition on h, then
// both read (one wave: the instructions execute in order).  The compiler models the lanes as independent threads, so it
// may read a slot BEFORE the neighbour's conditional store where it can prove that this thread does not store -- it did,
// in the one-joint prismatic form (the all-unrolled chain: the odd lane read the mass matrix slot early and found its
// edges singular).  The prismatic forms therefore close every such hand-over with a compiler-level memory barrier (no
// instruction); the revolute forms are left as they compile today.
RKH_DI void pair_lds_handover() {
  if (kPrismatic) asm volatile("" : : : "memory");
}

template <int N>
struct PairLayout {
  enum : int {
    R = (N + 1) / 2,  // joints (columns, rows) per lane
    XE = 0,           // state being differentiated / tested [2N]
    CS = 2 * N,       // cos, sin of the full joint angles [2N] (forward sweep -> backward sweep)
    U = 4 * N,        // held input of the step [N]
    F = 5 * N,        // generalized forces [N] (backward sweep -> Cholesky)
    REG = 6 * N,      // one region, three tenants in time:
    FT = REG,         //   inertia_3D d'Alembert force / torque per link [6N] (forward sweep -> backward sweep)
    MF = REG,         //   Tcm^T (Mcm Tcm) before symmetrisation [N*N] (after the backward sweep)
    ECP = REG,        //   proximity test: joint end frames, position of joints 1 .. N-1 [3N-3]
    ECQ = REG + 3 * N - 3,  //                                 quaternion [4N]
    REG_SLOTS = (6 * N > N * N ? (6 * N > 7 * N - 3 ? 6 * N : 7 * N - 3) : (N * N > 7 * N - 3 ? N * N : 7 * N - 3)),
    SLOTS = REG + REG_SLOTS
  };
};
template <int N>
struct PairLds {
  double v[PairLayout<N>::SLOTS][kPairEdges];
  double axis[N + 1][3];  // revolute_joint_3D::mAxis of every joint (indexed per lane: column 2r + h); one spare row
  // proximity test: queues of surviving (edge, robot shape, obstacle) pairs, their fill counts, one verdict per edge
  uint32_t q1[128], q2[64], qn[2], hit[kPairEdges];
};
#define RKH_LD(slot) lds.v[(slot)][el]

// global workspace of one wave, [slot][lane] (`ws` points at the lane's column): per-lane private values
template <int N>
struct PairWs {
  enum : int {
    R = (N + 1) / 2,
    W = 0,           // RK4: state at the start of the inner step (this lane's joints: 2 components each)
    KA = 2 * R,      // RK4: k1, then (1/6) k1 + (2/6) k2
    K3 = 4 * R,      // RK4: k3
    X = 6 * R,       // last free state [2N]
    B = 6 * R + 2 * N,  // steer target [2N]
    SLOTS = 6 * R + 4 * N
  };
};
// The workspace is addressed through a buffer resource: one descriptor (4 scalar registers) for the wave's region, the
// lane's byte offset in ONE vector register, the slot offset in the instruction's scalar offset.  (With flat pointers
// every slot beyond the 4 KB immediate range costs a 64-bit address pair held in vector registers across the kernel.)
typedef unsigned int rkh_u32x2 __attribute__((ext_vector_type(2)));
struct PairWsRef {
  __amdgpu_buffer_rsrc_t rsrc;
  int voff;  // lane * 8
};
RKH_DI double ws_ld(const PairWsRef& w, int slot) {
  const rkh_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(w.rsrc, w.voff, slot * 512, 0);
  return __hiloint2double(int(v.y), int(v.x));
}
RKH_DI void ws_st(const PairWsRef& w, int slot, double d) {
  rkh_u32x2 v;
  v.x = (unsigned)__double2loint(d);
  v.y = (unsigned)__double2hiint(d);
  __builtin_amdgcn_raw_buffer_store_b64(v, w.rsrc, w.voff, slot * 512, 0);
}

// The update after the f-eval of RK4 stage `stage` (runge_kutta4_integrator_sys.hpp:53-97).  Lane h advances the joints
// 2 jr + h: components 2j (q: derivative = qd of the differentiated state) and 2j + 1 (qd: derivative = qdd), in its
// private workspace slots sl = 2 jr + half (W_::W, KA, K3 + sl).  The slots are lane-private, so nothing aliases: a
// stage issues every workspace load it needs before its first store -- one memory round trip per stage, not one per
// slot (a load behind a buffer store is not moved over it).  Every slot's expression is the reference's.
template <int N, class W_>
RKH_DI void pair_rk4_stage_update(const PairWsRef& ws, PairLds<N>& lds, int el, int h, int stage, double h_dt,
                                  const double (&qdd)[N]) {
  typedef PairLayout<N> L_;
  constexpr int R = L_::R;
  double xv[2 * R], dp[2 * R], xn[2 * R];
#pragma unroll
  for (int jr = 0; jr < R; ++jr) {
    const int j = 2 * jr + h;
    const int jc = j < N ? j : 2 * jr;
    // (the odd joint's value goes through an opaque copy: a plain `h ? qdd[2jr+1] : qdd[2jr]` is turned into a
    // run-time-indexed read of the array, which puts the array into scratch)
    double qdd_odd = qdd[2 * jr + 1 < N ? 2 * jr + 1 : 2 * jr];
    asm volatile("" : "+v"(qdd_odd));
    const double qdd_j = h ? qdd_odd : qdd[2 * jr];
    const double xq = RKH_LD(L_::XE + 2 * jc), xqd = RKH_LD(L_::XE + 2 * jc + 1);
    xv[2 * jr] = xq;
    xv[2 * jr + 1] = xqd;
    dp[2 * jr] = xqd;
    dp[2 * jr + 1] = qdd_j;
  }
  if (stage == 0) {
#pragma unroll
    for (int sl = 0; sl < 2 * R; ++sl) {
      const double k1 = h_dt * dp[sl];
      ws_st(ws, W_::W + sl, xv[sl]);
      ws_st(ws, W_::KA + sl, k1);
      xn[sl] = xv[sl] + 0.5 * k1;
    }
  } else if (stage == 1) {
    double k1[2 * R], w[2 * R];
#pragma unroll
    for (int sl = 0; sl < 2 * R; ++sl) {
      k1[sl] = ws_ld(ws, W_::KA + sl);
      w[sl] = ws_ld(ws, W_::W + sl);
    }
#pragma unroll
    for (int sl = 0; sl < 2 * R; ++sl) {
      const double k2 = h_dt * dp[sl];
      ws_st(ws, W_::KA + sl, (1.0 / 6.0) * k1[sl] + (2.0 / 6.0) * k2);
      xn[sl] = w[sl] + 0.5 * k2;
    }
  } else if (stage == 2) {
    double w[2 * R];
#pragma unroll
    for (int sl = 0; sl < 2 * R; ++sl) w[sl] = ws_ld(ws, W_::W + sl);
#pragma unroll
    for (int sl = 0; sl < 2 * R; ++sl) {
      const double k3v = h_dt * dp[sl];
      ws_st(ws, W_::K3 + sl, k3v);
      xn[sl] = w[sl] + k3v;
    }
  } else {
    double ka[2 * R], k3[2 * R];
#pragma unroll
    for (int sl = 0; sl < 2 * R; ++sl) {
      ka[sl] = ws_ld(ws, W_::KA + sl);
      k3[sl] = ws_ld(ws, W_::K3 + sl);
    }
#pragma unroll
    for (int sl = 0; sl < 2 * R; ++sl) xn[sl] = xv[sl] + ((ka[sl] + (h_dt / 6.0) * dp[sl]) - (2.0 / 3.0) * k3[sl]);
  }
#pragma unroll
  for (int jr = 0; jr < R; ++jr) {
    const int j = 2 * jr + h;
    if (j < N) {
      RKH_LD(L_::XE + 2 * j) = xn[2 * jr];
      RKH_LD(L_::XE + 2 * j + 1) = xn[2 * jr + 1];
    }
  }
}

// Jacobian column of the body at (pos, Q) w.r.t. the coordinate of a joint whose end frame is (p, cq): get_jac_relative_to
// (motion_jacobians.hpp:238-251) with f2 = (~F_c) * F_b (frame_3D.hpp:184-189,222-238,368-382).  Rc = rotmat(cq) and
// ipos = (-p) * Rc are the joint's own, fixed from the iteration that captured its frame.  MASK: the slot can hold a lane
// whose column lies beyond the body (act false there); its column is an exact +0 vector.  (act is read only with MASK, pc
// only in the prismatic forms.)
template <bool MASK>
RKH_DI void pair_jac_column(d3 ipos, d4 cq, const m33& Rc, d3 pos, d4 Q, d3 ax_c, bool pc, bool act, d3& Tv, d3& Tw) {
  const d4 iq = qinv(cq);
  // rotmat(conj(q)) is rotmat(q) transposed bit for bit (negating x, y, z flips the sign of the w-products and
  // leaves the others unchanged), so Ri * pos is evaluated as pos * Rc: same products, same order
  const d3 f2pos = ipos + mulT(pos, Rc);
  const d4 f2q = qmul(iq, Q);
  const m33 Rf = rotmat(f2q);
  d3 wt = mulT(ax_c, Rf);
  d3 vt = mulT(cross(ax_c, f2pos), Rf);
  if (kPrismatic) {  // prismatic_joint_3D: qd_vel = mAxis, qd_avel = 0.  The column differs between the edge's
    // lanes: selects.  wt = +0 adds +-0 products to sums that are never -0, like a column beyond the body below.
    vt = mk3(pc ? wt.x : vt.x, pc ? wt.y : vt.y, pc ? wt.z : vt.z);
    wt = mk3(pc ? 0.0 : wt.x, pc ? 0.0 : wt.y, pc ? 0.0 : wt.z);
  }
  // A column beyond the body is an exact +0 vector: Mcm * 0 = +0 and s + (+-0) = s bit for bit (the sums start from +0
  // or from a joint inertia, so they are never -0), hence the accumulation needs no masks.
  if (MASK) {
    Tw = mk3(act ? wt.x : 0.0, act ? wt.y : 0.0, act ? wt.z : 0.0);
    Tv = mk3(act ? vt.x : 0.0, act ? vt.y : 0.0, act ? vt.z : 0.0);
  } else {
    Tw = wt;
    Tv = vt;
  }
}

// x' = f(x, u) of one edge.  In: the state in LD(XE..), the input in LD(U..).  Out: qdd[j] on both lanes (the q
// components of x' are the qd components of x).  el = the edge's LDS column, h = which of the edge's two lanes this is.
template <int N, bool DIAG = false>
__device__ __forceinline__ void pair_state_derivative(ScenePtr sc_in, PairLds<N>& lds, int el, int h,
                                                      double (&qdd)[N], bool& singular,
                                                      unsigned long long* stamps = nullptr) {
  typedef PairLayout<N> L_;
  constexpr int R = L_::R;
  // The scene pointer is laundered once per call: otherwise every scene constant this function reads (and every LDS
  // value that does not change between calls) is hoisted out of the caller's loops and held in registers across the
  // whole kernel -- the registers this kernel does not have (two waves per SIMD = 256 per lane).
  ScenePtr sc = sc_in;
  asm volatile("" : "+s"(sc), "+v"(h), "+v"(el) : : "memory");  // the lane's coordinates too: addresses derived from them
  unsigned long long t_prev = DIAG ? __builtin_readcyclecounter() : 0ull;
#define RKH_STAMP(i)                                                \
  if (DIAG) {                                                       \
    const unsigned long long t_now = __builtin_readcyclecounter(); \
    stamps[i] += t_now - t_prev;                                    \
    t_prev = t_now;                                                 \
  }
  // this lane's rows i = 2r + h of Tcm^T (Mcm Tcm): Mo[r][rr] = column 2rr + h (own parity), Mp[r][rr] = column
  // 2rr + 1 - h (the neighbour's parity).  inertia_gen rows: Tcm = 1 on the diagonal.
  const uint32_t pmask = kPrismatic ? sc->prismatic_mask : 0u;  // bit j: joint j translates (read in uniform control flow)
  double Mo[R][R], Mp[R][R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      Mo[r][rr] = 0.0;
      Mp[r][rr] = 0.0;
    }
    const double ji0 = sc->joints[2 * r].joint_inertia;
    const double ji1 = (2 * r + 1 < N) ? sc->joints[2 * r + 1 < N ? 2 * r + 1 : 0].joint_inertia : 0.0;
    Mo[r][r] = 0.0 + (h ? ji1 : ji0);
  }
  // end frames of this lane's joints c = 2r + h (parents of its Jacobian columns): the quaternion cq and, of the
  // position p, the one thing a column needs, ipos = (-p) * rotmat(cq) -- formed once, where the frame is captured.  A
  // slot whose joint has not been reached (or does not exist: an odd chain's last slot on lane 1) holds finite values
  // and its column is masked.
  d3 Eip[R];
  d4 Ecq[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    Eip[r] = mk3(0.0, 0.0, 0.0);
    Ecq[r] = d4{1.0, 0.0, 0.0, 0.0};
  }
  // rotmat(cq) of slot 0, the slot every body uses, kept where the registers are there for it (7 joints spill without
  // it).  It costs 16 registers at N = 6 (240 of 256 in the step kernel) for 1.4 % of the f-eval: the first thing to give
  // back if the register count tightens.
  constexpr bool kRc0 = N >= 2 && N <= 6;
  m33 Rc0 = m33{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

  // ---- base -> tip sweep (kte_map_chain::doMotion) with the Jacobian columns and M terms of each body
  d3 pos = ldg3(sc->base_pos);
  d4 Q = ldg4(sc->base_quat);
  d3 w = mk3(0, 0, 0), alpha = mk3(0, 0, 0);
  d3 acc = ldg3(sc->base_acc);
#pragma unroll 1
  for (int j = 0; j < N; ++j) {
    const auto& J = sc->joints[j];
    const d3 axis = ldg3(J.axis), axis_n = ldg3(J.axis_n);
    const double q = RKH_LD(L_::XE + 2 * j), qd = RKH_LD(L_::XE + 2 * j + 1);
    d4 EQ;
    d3 Ew, Ealpha;
    if (kPrismatic && ((pmask >> j) & 1u)) {  // (uniform: j is)
      // prismatic_joint_3D::doMotion (prismatic_joint.cpp:116-148), q_ddot = 0: the end frame keeps the base's
      // orientation and rates and moves by R(Q) (q a); no sincos, nothing in the cos / sin slots
      const d3 tmp_pos = q * axis;
      const d3 tmp_vel = qd * axis;
      const m33 Rb = rotmat(Q);
      acc = acc + mul(Rb, (cross(w, cross(w, tmp_pos)) + 2.0 * cross(w, tmp_vel)) + cross(alpha, tmp_pos));
      pos = pos + mul(Rb, tmp_pos);
      EQ = Q;
      Ew = w;
      Ealpha = alpha;
    } else {
      // one sincos per lane: half angle on lane h = 0, full angle on lane h = 1 (kept for the tip->base sweep)
      double sn, cs;
      sincos(h ? q : 0.5 * q, &sn, &cs);
      const double cs_o = xchg(cs), sn_o = xchg(sn);
      const double c2 = h ? cs_o : cs, s2 = h ? sn_o : sn;
      if (h) {
        RKH_LD(L_::CS + 2 * j) = cs;
        RKH_LD(L_::CS + 2 * j + 1) = sn;
      }
      // revolute_joint_3D::doMotion (revolute_joint.cpp:121-148)
      const d4 tq = d4{c2, axis_n.x * s2, axis_n.y * s2, axis_n.z * s2};
      const m33 R2 = rotmat(tq);
      EQ = qmul(Q, tq);
      const d3 wb = mulT(w, R2);
      const d3 qa = qd * axis;
      Ew = wb + qa;
      Ealpha = mulT(alpha, R2) + cross(wb, qa);
    }
    const m33 Rm = rotmat(EQ);
    {  // the joint's end frame, kept by the lane that owns column j, in slot j >> 1: a uniform branch, one select per value
      const bool mine = ((j & 1) == h);
      const int rj = j >> 1;
      const d3 ip = mulT(-pos, Rm);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (rj == r) {
          Eip[r] = mk3(mine ? ip.x : Eip[r].x, mine ? ip.y : Eip[r].y, mine ? ip.z : Eip[r].z);
          Ecq[r] = d4{mine ? EQ.w : Ecq[r].w, mine ? EQ.x : Ecq[r].x, mine ? EQ.y : Ecq[r].y, mine ? EQ.z : Ecq[r].z};
          if (kRc0 && r == 0)
            Rc0 = m33{mine ? Rm.a11 : Rc0.a11, mine ? Rm.a12 : Rc0.a12, mine ? Rm.a13 : Rc0.a13,
                      mine ? Rm.a21 : Rc0.a21, mine ? Rm.a22 : Rc0.a22, mine ? Rm.a23 : Rc0.a23,
                      mine ? Rm.a31 : Rc0.a31, mine ? Rm.a32 : Rc0.a32, mine ? Rm.a33 : Rc0.a33};
        }
      }
    }
    // rigid_link_3D::doMotion = frame * pose (frame_3D.hpp:240-255)
    const d3 op = ldg3(J.off_pos);
    pos = pos + mul(Rm, op);
    acc = acc + mul(Rm, cross(Ew, cross(Ew, op)) + cross(Ealpha, op));
    const m33 Ro = ldgm(J.off_R);
    Q = qmul(EQ, ldg4(J.off_quat));
    alpha = mulT(Ealpha, Ro);
    w = mulT(Ew, Ro);
    // inertia_3D::doForce terms (inertia.cpp:111-122), applied in the backward sweep
    const Sym6 In6 = ldsym(J.inertia);
    const d3 Fi = J.mass * qrot(qinv(Q), acc);
    const d3 Ti = sym_mul(In6.t, alpha) + cross(w, sym_mul(In6.t, w));
    if (h) {
      RKH_LD(L_::FT + 6 * j) = Fi.x; RKH_LD(L_::FT + 6 * j + 1) = Fi.y; RKH_LD(L_::FT + 6 * j + 2) = Fi.z;
      RKH_LD(L_::FT + 6 * j + 3) = Ti.x; RKH_LD(L_::FT + 6 * j + 4) = Ti.y; RKH_LD(L_::FT + 6 * j + 5) = Ti.z;
    }
    RKH_STAMP(0)
    // Jacobian columns of body j w.r.t. this lane's coords c = 2r + h <= j.  The newest slot (2r == j) is the one slot
    // that can hold a column beyond j (lane 1's), and its lane 0 column is joint j itself: rotmat(cq) is this
    // iteration's Rm.  Lane 1 computes on Rm too, and on its (identity) frame; its column is masked.
    d3 Tv[R], Tw[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      Tv[r] = mk3(0.0, 0.0, 0.0);
      Tw[r] = mk3(0.0, 0.0, 0.0);
      const int c = 2 * r + h;  // <= N: the spare row of lds.axis covers an odd chain's last slot
      const bool pc = kPrismatic && ((pmask >> c) & 1u) != 0u;
      const bool act = (c <= j);
      if (2 * r == j) {  // uniform
        const d3 ax_c = mk3(lds.axis[c][0], lds.axis[c][1], lds.axis[c][2]);
        pair_jac_column<true>(Eip[r], Ecq[r], Rm, pos, Q, ax_c, pc, act, Tv[r], Tw[r]);
      } else if (2 * r < j) {  // uniform: both lanes' columns exist, nothing to mask
        const d3 ax_c = mk3(lds.axis[c][0], lds.axis[c][1], lds.axis[c][2]);
        const m33 Rc = (kRc0 && r == 0) ? Rc0 : rotmat(Ecq[r]);
        pair_jac_column<false>(Eip[r], Ecq[r], Rc, pos, Q, ax_c, pc, act, Tv[r], Tw[r]);
      }
    }
    RKH_STAMP(1)
    // Mf += Tcm_b^T (Mcm_b Tcm_b): summation order of mat_alg_symmetric.hpp:551-566 and mat_operators.hpp:104-114.
    // Column block rr: Mcm * T of this lane's column 2rr + h, and the neighbour's (column 2rr + 1 - h) by DPP.
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      if (2 * rr <= j) {  // uniform
        const double m0 = J.mass * Tv[rr].x, m1 = J.mass * Tv[rr].y, m2 = J.mass * Tv[rr].z;
        const d3 P = sym_mul(In6.t, Tw[rr]);
        const double n0 = xchg(m0), n1 = xchg(m1), n2 = xchg(m2);
        const d3 Pn = xchg3(P);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (2 * r <= j) {  // uniform
            double s = Mo[r][rr];
            s = s + Tv[r].x * m0;
            s = s + Tv[r].y * m1;
            s = s + Tv[r].z * m2;
            s = s + Tw[r].x * P.x;
            s = s + Tw[r].y * P.y;
            s = s + Tw[r].z * P.z;
            Mo[r][rr] = s;
            double t = Mp[r][rr];
            t = t + Tv[r].x * n0;
            t = t + Tv[r].y * n1;
            t = t + Tv[r].z * n2;
            t = t + Tw[r].x * Pn.x;
            t = t + Tw[r].y * Pn.y;
            t = t + Tw[r].z * Pn.z;
            Mp[r][rr] = t;
          }
        }
      }
    }
    RKH_STAMP(2)
  }

  // ---- tip -> base sweep (kte_map_chain::doForce in reverse op order)
  pair_lds_handover();  // FT, CS
  {
    d3 LF = mk3(0, 0, 0), LT = mk3(0, 0, 0);
    if (sc->beam_on) {  // flexible_beam_3D::doForce: listed last, so first in the reverse pass (first term of the sums)
      d3 BF, BT;
      beam_force(pos, Q, ldg3(sc->beam_pos), ldg4(sc->beam_quat), sc->beam_rest, sc->beam_k, sc->beam_kt, &BF, &BT);
      LF = LF + BF;
      LT = LT + BT;
    }
#pragma unroll 1
    for (int j = N - 1; j >= 0; --j) {
      const auto& J = sc->joints[j];
      const d3 axis = ldg3(J.axis);
      LF = LF - mk3(RKH_LD(L_::FT + 6 * j), RKH_LD(L_::FT + 6 * j + 1), RKH_LD(L_::FT + 6 * j + 2));  // inertia_3D::doForce
      LT = LT - mk3(RKH_LD(L_::FT + 6 * j + 3), RKH_LD(L_::FT + 6 * j + 4), RKH_LD(L_::FT + 6 * j + 5));
      const m33 Ro = ldgm(J.off_R);                 // rigid_link_3D::doForce (rigid_link.cpp:170-178)
      const d3 op = ldg3(J.off_pos);
      const d3 tmp_force = mul(Ro, LF);
      const d3 ET = mul(Ro, LT) + cross(op, tmp_force);
      if (kPrismatic && ((pmask >> j) & 1u)) {  // (uniform)
        // prismatic_joint_3D::doForce (prismatic_joint.cpp:150-170): the force along the axis goes to the coordinate;
        // the actuator's reaction (prismatic_joint.cpp:219-222) is a force on the base frame
        const double tf = dot(tmp_force, axis);
        LF = tmp_force - tf * axis;
        LT = ET + cross(RKH_LD(L_::XE + 2 * j) * axis, tmp_force);
        const double uj = RKH_LD(L_::U + j);
        if (!h) RKH_LD(L_::F + j) = tf + uj;
        LF = LF - uj * axis;
        continue;
      }
      const m33 Ra = pair_axis_angle_rotmat(RKH_LD(L_::CS + 2 * j), RKH_LD(L_::CS + 2 * j + 1),
                                            ldg3(J.axis_n));  // revolute_joint_3D::doForce (revolute_joint.cpp:170-181)
      const double ta = dot(ET, axis);
      LF = mul(Ra, tmp_force);
      LT = mul(Ra, ET - ta * axis);
      const double uj = RKH_LD(L_::U + j);  // inertia_gen::doForce (q_ddot = 0), driving_actuator_gen::doForce
      if (!h) RKH_LD(L_::F + j) = ta + uj;
      LT = LT - uj * axis;
    }
  }
  RKH_STAMP(3)

  pair_lds_handover();  // F
  // ---- the two lanes' rows meet in LDS (the link forces are no longer needed)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = 2 * r + h;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      const int co = 2 * rr + h, cn = 2 * rr + 1 - h;
      if (i < N && co < N) RKH_LD(L_::MF + i * N + co) = Mo[r][rr];
      if (i < N && cn < N) RKH_LD(L_::MF + i * N + cn) = Mp[r][rr];
    }
  }
  pair_lds_handover();  // MF
  // ---- mat<symmetric>(general): 0.5 * (M(j,i) + M(i,j)), j < i (mat_alg_symmetric.hpp:183-187), lower triangle
  double L[N][N], f[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    f[i] = RKH_LD(L_::F + i);
#pragma unroll
    for (int j = 0; j <= i; ++j)
      L[i][j] = (i == j) ? RKH_LD(L_::MF + i * N + i) : 0.5 * (RKH_LD(L_::MF + j * N + i) + RKH_LD(L_::MF + i * N + j));
  }
  // ---- linsolve_Cholesky (mat_cholesky.hpp:63-84,546-554)
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double dgl = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) dgl = dgl - L[j][k] * L[j][k];
    if (dgl < 1e-8) singular = true;
    const double ljj = sqrt(dgl);
    L[j][j] = ljj;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double v = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
      L[i][j] = v / ljj;
    }
  }
  // backsub_Cholesky_impl (mat_cholesky.hpp:160-178): L y = f, then L^T x = y
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double yk = f[k] / L[k][k];
    f[k] = yk;
#pragma unroll
    for (int r = k + 1; r < N; ++r) f[r] = f[r] - L[r][k] * yk;
  }
#pragma unroll
  for (int k = N - 1; k >= 0; --k) {
    const double xk = f[k] / L[k][k];
    f[k] = xk;
#pragma unroll
    for (int r = 0; r < k; ++r) f[r] = f[r] - L[k][r] * xk;
  }
#pragma unroll
  for (int j = 0; j < N; ++j) qdd[j] = f[j];
  RKH_STAMP(4)
#undef RKH_STAMP
}

// ---- proximity test: work queues in LDS --------------------------------------------------------------------------
// The bounding cull runs per lane (lane h of an edge takes the robot shapes r0 + h); what survives it is NOT evaluated
// by the lane that found it but pushed, as (edge, robot shape, obstacle), into a queue in LDS and handed out one entry
// per lane: a wave spends one pass of the closed forms per 64 surviving pairs instead of one pass per pair of its
// unluckiest lane.  Pairs that need the golden-section search of findProximityBoxToLine (capped cylinder against box)
// go through a second queue, so the ~1.5 k instructions of a search are spent by full lanes only.
constexpr int kQ1Cap = 128, kQ2Cap = 64;
constexpr uint32_t kQEmpty = 0xFFFFFFFFu;
RKH_DI uint32_t q_pack(int el, int r, int o) { return (uint32_t(el) << 16) | (uint32_t(r) << 8) | uint32_t(o); }

// global pose of robot shape r of the edge in LDS column e (pose_3D::getGlobalPose, pose_3D.hpp:102-110)
template <int N>
RKH_DI ShapeG pair_robot_pose(ScenePtr sc, PairLds<N>& lds, int e, int r) {
  typedef PairLayout<N> L_;
  const auto& sh = sc->robot[r];
  const int j = sh.link;
  const int js3 = j > 0 ? 3 * j - 3 : 0;
  d3 Epos = mk3(lds.v[L_::ECP + js3][e], lds.v[L_::ECP + js3 + 1][e], lds.v[L_::ECP + js3 + 2][e]);
  if (j == 0) Epos = ldg3(sc->base_pos);
  if (kPrismatic) {
    // a prismatic root: joint 0's end position is the base moved by R(base_quat) (q0 a).  The layout has no slot for
    // it, so it is formed here, from the state in LDS and scene constants (uniform addresses: scalar loads).
    const d3 root = ldg3(sc->base_pos) + mul(rotmat(ldg4(sc->base_quat)), lds.v[L_::XE][e] * ldg3(sc->joints[0].axis));
    const bool moved = (j == 0) && (sc->prismatic_mask & 1u);
    Epos = mk3(moved ? root.x : Epos.x, moved ? root.y : Epos.y, moved ? root.z : Epos.z);
  }
  const d4 EQ = d4{lds.v[L_::ECQ + 4 * j][e], lds.v[L_::ECQ + 4 * j + 1][e], lds.v[L_::ECQ + 4 * j + 2][e],
                   lds.v[L_::ECQ + 4 * j + 3][e]};
  ShapeG A;
  A.kind = sh.kind;
  A.pos = Epos + qrot(EQ, ldg3(sh.pos));
  A.q = qmul(EQ, ldg4(sh.quat));
  A.d0 = sh.dims[0]; A.d1 = sh.dims[1]; A.d2 = sh.dims[2];
  return A;
}
template <class EnvRef>
RKH_DI ShapeG pair_env_shape(const EnvRef& es) {
  ShapeG Bv;
  Bv.kind = es.kind;
  Bv.pos = ldg3(es.pos);
  Bv.q = ldg4(es.quat);
  Bv.d0 = es.dims[0]; Bv.d1 = es.dims[1]; Bv.d2 = es.dims[2];
  return Bv;
}

// golden-section pairs of the second queue (all lanes of the wave call this together)
template <int N>
RKH_DI void pair_drain_q2(ScenePtr sc, PairLds<N>& lds) {
  const int lane = threadIdx.x & 63;
  const uint32_t n2 = lds.qn[1] < uint32_t(kQ2Cap) ? lds.qn[1] : uint32_t(kQ2Cap);
  if (n2 == 0) return;  // uniform
  const uint32_t ent = (uint32_t(lane) < n2) ? lds.q2[lane] : kQEmpty;
  if (ent != kQEmpty) {
    const int e = int(ent >> 16), r = int((ent >> 8) & 0xFFu), o = int(ent & 0xFFu);
    if (lds.hit[e] == 0u) {
      const ShapeG A = pair_robot_pose<N>(sc, lds, e, r);
      const ShapeG Bv = pair_env_shape(sc->env[o]);
      const double d = (A.kind == RKH_SHAPE_CCYLINDER) ? dist_ccyl_box(A, Bv) : dist_ccyl_box(Bv, A);  // PR_CCYL_BOX only
      if (d < 0.0) lds.hit[e] = 1u;
    }
  }
  if (lane == 0) lds.qn[1] = 0u;
}

// the first queue: closed forms, and the separating-axis screen in front of the golden-section pairs
// n_exact / n_gold (diagnostic instantiation only): closed forms this lane evaluated, golden-section pairs it queued
template <int N>
RKH_DI void pair_drain_q1(ScenePtr sc, PairLds<N>& lds, uint32_t* n_exact = nullptr, uint32_t* n_gold = nullptr) {
  const int lane = threadIdx.x & 63;
  const uint32_t n1 = lds.qn[0] < uint32_t(kQ1Cap) ? lds.qn[0] : uint32_t(kQ1Cap);
#pragma unroll 1
  for (uint32_t k0 = 0; k0 < n1; k0 += 64u) {
    const uint32_t idx = k0 + uint32_t(lane);
    const uint32_t ent = (idx < n1) ? lds.q1[idx] : kQEmpty;
    bool golden = false;
    if (ent != kQEmpty) {
      const int e = int(ent >> 16), r = int((ent >> 8) & 0xFFu), o = int(ent & 0xFFu);
      if (lds.hit[e] == 0u) {
        const ShapeG A = pair_robot_pose<N>(sc, lds, e, r);
        const ShapeG Bv = pair_env_shape(sc->env[o]);
        bool a_first = true;
        const int rt = pair_routine(A.kind, Bv.kind, &a_first);  // createProxFinderList's cascade of kinds
        if (rt == PR_CCYL_BOX) {
          // capped cylinder against a box = a golden-section search along the axis (prox_fundamentals_3D.cpp:108-115).
          // Every value that search can return is the distance of SOME point of the axis segment to the box, so a lower
          // bound over the segment that already exceeds the radius settles "no collision" without it: separation along the
          // box's own axes, |c_k| - hl |t_k| - half_k, in the box frame (fp64, margin 1e-9).
          const ShapeG& cc = a_first ? A : Bv;
          const ShapeG& bx = a_first ? Bv : A;
          const d3 cy_c = pose_to_parent(cc.pos, cc.q, mk3(0, 0, 0));
          const d3 cy_t = qrot(cc.q, mk3(0.0, 0.0, 1.0));
          const d4 bq = qinv(bx.q);
          const d3 crel = qrot(bq, cy_c - bx.pos);
          const d3 trel = qrot(bq, cy_t);
          const double hl = 0.5 * cc.d0;
          const double gx = fabs(crel.x) - fabs(trel.x) * hl - 0.5 * bx.d0;
          const double gy = fabs(crel.y) - fabs(trel.y) * hl - 0.5 * bx.d1;
          const double gz = fabs(crel.z) - fabs(trel.z) * hl - 0.5 * bx.d2;
          golden = !(fmax(gx, fmax(gy, gz)) > cc.d1 + 1e-9);
        } else if (rt != PR_NONE) {
          const double d = a_first ? pair_distance<false>(rt, A, Bv) : pair_distance<false>(rt, Bv, A);
          if (d < 0.0) lds.hit[e] = 1u;
          if (n_exact) ++*n_exact;
        }
      }
    }
    // golden-section pairs move on to the second queue; when it is full it is drained first (uniform decisions)
    while (__any(golden)) {
      uint32_t slot = kQ2Cap;
      if (golden) slot = atomicAdd(&lds.qn[1], 1u);
      if (golden && slot < uint32_t(kQ2Cap)) {
        lds.q2[slot] = ent;
        golden = false;
        if (n_gold) ++*n_gold;
      }
      if (__any(golden)) pair_drain_q2<N>(sc, lds);  // some did not fit: empty the queue, then they try again
    }
  }
  if (lane == 0) lds.qn[0] = 0u;
}

// Carried clearance (revolute forms; SceneDev::has_clearance scenes).  The cull below forms, for every pair it looks at,
// a lower bound lb = |w| - reach on the pair's distance.  The smallest lb over the pairs with a finder up to kClearHorizon
// beyond the static reach, and SceneDev::clear_static for all pairs further out, bound the clearance of the whole
// configuration from below (the minimum distance over every pair the reference evaluates); a pair that passes the cull
// has lb <= 0.  No point of the robot moves more than delta = sum_i clear_arm[i] |dq_i| between two
// configurations, so a state within delta < clearance of a tested one is free without a test: the steer kernels carry
// clearance - (the deltas of the steps since) per edge and run the test only when it is used up.  The test they skip
// would have returned "free", so states, step counts and verdicts are unchanged.
constexpr float kClearSlack = 1e-5f;   // for the rounding of the sqrt, the min and the carried subtractions
constexpr float kClearMax = 4.0f;      // the carried value stays below this, so one of its roundings is below 2.4e-7
constexpr float kClearStepPad = 2.4e-7f;  // added to every step's delta: the rounding of budget - delta

// is the configuration in LD(XE..) (joint angles) collision-free?  (manip_dk_proxy_env_impl::is_free, proximity only)
// clearance: a lower bound on the distance of the closest pair, <= 0 when some pair passed the cull (0 in the prismatic
// forms, which do not form it)
template <int N, bool DIAG = false>
__device__ __forceinline__ bool pair_proximity_free(ScenePtr sc_in, PairLds<N>& lds, int el, int h,
                                                    bool active, float& clearance, unsigned long long* stamps = nullptr) {
  typedef PairLayout<N> L_;
  constexpr int R = L_::R;
  ScenePtr sc = sc_in;  // laundered, see pair_state_derivative
  asm volatile("" : "+s"(sc), "+v"(h), "+v"(el) : : "memory");
  unsigned long long t_prev = DIAG ? __builtin_readcyclecounter() : 0ull;
#define RKH_STAMP(i)                                                \
  if (DIAG) {                                                       \
    const unsigned long long t_now = __builtin_readcyclecounter(); \
    stamps[i] += t_now - t_prev;                                    \
    t_prev = t_now;                                                 \
  }
  const int lane = threadIdx.x & 63;
  const int n_env = sc->n_env, n_robot = sc->n_robot;
  uint32_t c_q1 = 0, c_exact = 0, c_gold = 0;  // (diagnostic instantiation only)
  float lb_min = INFINITY;  // smallest lower bound over this lane's pairs
  if (lane < 2) lds.qn[lane] = 0u;
  if (lane < kPairEdges) lds.hit[lane] = 0u;
  // this lane's cull record of the first obstacle chunk, fetched ahead of the kinematics
  const int ol0 = (lane < n_env) ? lane : 0;
  const float e0x = float(sc->env_cull[ol0][0]), e0y = float(sc->env_cull[ol0][1]), e0z = float(sc->env_cull[ol0][2]),
              e0r = float(sc->env_cull[ol0][3]);
  {  // joint end frames: revolute_joint_3D / rigid_link_3D kinematics, position + orientation only.  The half-angle
     // sin / cos of the joints 2r + h are this lane's; both lanes read them back from the (idle) cos / sin slots.
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = 2 * r + h;
      const int jc = j < N ? j : N - 1;
      double s2, c2;
      sincos(0.5 * RKH_LD(L_::XE + 2 * jc), &s2, &c2);
      if (j < N) {
        RKH_LD(L_::CS + 2 * jc) = c2;
        RKH_LD(L_::CS + 2 * jc + 1) = s2;
      }
    }
    pair_lds_handover();  // CS
    d3 pos = ldg3(sc->base_pos);
    d4 Q = ldg4(sc->base_quat);
#pragma unroll 1
    for (int j = 0; j < N; ++j) {
      const auto& J = sc->joints[j];
      const d3 axis_n = ldg3(J.axis_n);
      const double c2 = RKH_LD(L_::CS + 2 * j), s2 = RKH_LD(L_::CS + 2 * j + 1);
      const d4 tq = d4{c2, axis_n.x * s2, axis_n.y * s2, axis_n.z * s2};
      d4 EQ = qmul(Q, tq);
      if (kPrismatic && ((sc->prismatic_mask >> j) & 1u)) {  // (uniform) prismatic_joint_3D: translate by R(Q) (q a), keep Q
        pos = pos + mul(rotmat(Q), RKH_LD(L_::XE + 2 * j) * ldg3(J.axis));
        EQ = Q;
      }
      if (!h) {
        if (j > 0) {
          RKH_LD(L_::ECP + 3 * j - 3) = pos.x; RKH_LD(L_::ECP + 3 * j - 2) = pos.y; RKH_LD(L_::ECP + 3 * j - 1) = pos.z;
        }
        RKH_LD(L_::ECQ + 4 * j) = EQ.w; RKH_LD(L_::ECQ + 4 * j + 1) = EQ.x;
        RKH_LD(L_::ECQ + 4 * j + 2) = EQ.y; RKH_LD(L_::ECQ + 4 * j + 3) = EQ.z;
      }
      const m33 Rm = rotmat(EQ);
      pos = pos + mul(Rm, ldg3(J.off_pos));
      Q = qmul(EQ, ldg4(J.off_quat));
    }
  }
  pair_lds_handover();  // ECP, ECQ
  RKH_STAMP(5)
#pragma unroll 1
  for (int r0 = 0; r0 < n_robot; r0 += 2) {
    const int r = r0 + h;
    const bool open = active && (lds.hit[el] == 0u);
    if (!__any(open)) break;  // every edge of the wave is settled
    const bool have = (r < n_robot) && open;
    const int rc = (r < n_robot) ? r : r0;
    const ShapeG A = pair_robot_pose<N>(sc, lds, el, rc);
    const d3 ca = pose_to_parent(A.pos, A.q, mk3(0, 0, 0));
    const d3 cull_org = ldg3(sc->base_pos);  // origin of the cull records (SceneDev::env_cull)
    const bool a_ccyl = (A.kind == RKH_SHAPE_CCYLINDER);
    // capped cylinder: its axis segment (for the cull below)
    const d3 a_ax = qrot(A.q, mk3(0.0, 0.0, 1.0));
    const double ra = sc->robot[rc].brad;
    const double seg_hl = a_ccyl ? 0.5 * A.d0 : 0.0, seg_rad_m = (a_ccyl ? A.d1 : ra) + 1e-9;
    // static reach (SceneDev::robot_n_reach): the obstacles this lane's shape can touch at all are a prefix of the table
    // (the revolute forms scan on to robot_n_clear: obstacles that only the clearance bound looks at)
    const int my_reach = sc->robot_n_reach[rc];
    const int my_clear = kPrismatic ? my_reach : sc->robot_n_clear[rc];
    const int reach0 = kPrismatic ? sc->robot_n_reach[r0] : sc->robot_n_clear[r0];
    const int reach1 = (r0 + 1 < n_robot) ? (kPrismatic ? sc->robot_n_reach[r0 + 1] : sc->robot_n_clear[r0 + 1]) : 0;
    const int n_scan = reach0 > reach1 ? reach0 : reach1;  // uniform
#pragma unroll 1
    for (int o0 = 0; o0 < n_scan; o0 += 64) {
      const int on = (n_scan - o0 < 64) ? n_scan - o0 : 64;
      const unsigned long long has_finder = sc->env_finder_mask[A.kind][o0 >> 6];  // per lane (its shape's kind)
      // Cull, one bit per surviving obstacle.  Lane l fetches the cull record of obstacle o0 + l once; the uniform loop
      // over the obstacles reads it back with v_readlane (no memory latency in the loop).  A pair is dropped only if a
      // lower bound on its distance is positive -- the bounding-sphere test of proxy_query_model.cpp:384-389 or, for
      // a capped-cylinder robot shape, the distance from the obstacle's bounding sphere to the cylinder's axis segment --
      // so the verdict "some pair is closer than 0" is unchanged.  The cull runs in fp32 with fused multiply-adds (a
      // conservative filter, not part of the reference's arithmetic) on coordinates RELATIVE TO THE CHAIN BASE: the
      // records hold centre - base, subtracted in fp64 on the host (scene.hip), and the shape's centre loses the base in
      // fp64 here, before anything is rounded to fp32.  What is rounded is then bounded by the chain's reach plus the
      // obstacle's distance from the base, wherever the world sits: a few metres for every pair that can touch, so the
      // 1 mm margin on the reach is three orders of magnitude above the rounding of the fp32 evaluation.  (Rounding
      // absolute coordinates made the margin depend on the world's offset: an fp32 ulp at 1e5 m is 8 mm.)  An obstacle
      // far from the base is rounded more coarsely -- relative to its own distance, 6e-8 of it.  Where its bounding
      // radius is of the order of the reach it is far outside every reach by the same measure; the margin does not
      // scale with the radius, so a very large obstacle centred far away (a slab of 100 m half-extent: centre and radius
      // rounded at 1e-5 m) is covered only to that rounding, at any world offset.
      float ecx = e0x, ecy = e0y, ecz = e0z, ecr = e0r;
      if (o0 != 0) {  // further chunks of 64 obstacles (uniform branch)
        const int ol = (o0 + lane < n_env) ? o0 + lane : o0;
        ecx = float(sc->env_cull[ol][0]); ecy = float(sc->env_cull[ol][1]); ecz = float(sc->env_cull[ol][2]);
        ecr = float(sc->env_cull[ol][3]);
      }
      const float cax = float(ca.x - cull_org.x), cay = float(ca.y - cull_org.y), caz = float(ca.z - cull_org.z);
      const float aax = float(a_ax.x), aay = float(a_ax.y), aaz = float(a_ax.z);
      const float shl = float(seg_hl), srm = float(seg_rad_m) + 1e-3f;
      unsigned long long mask = 0ull;
      // obstacles past this lane's own reach; pairs of kinds the reference has no finder for
      const int mine = my_reach - o0;
      unsigned long long mine_mask = (mine >= 64) ? ~0ull : (mine <= 0 ? 0ull : ((1ull << mine) - 1ull));
      mine_mask &= has_finder;
      if (!have) mine_mask = 0ull;
      // the pairs the clearance bound is taken over
      const int clr = my_clear - o0;
      unsigned long long clear_mask = (clr >= 64) ? ~0ull : (clr <= 0 ? 0ull : ((1ull << clr) - 1ull));
      clear_mask &= has_finder;
      if (!have) clear_mask = 0ull;
      unsigned mine_nib = 0u;  // bits i .. i + 3 of clear_mask
      auto cull_one = [&](int i) -> unsigned {  // 1 when the pair survives (branch-free: selects only)
        const float vx = readlane_f(ecx, i & 63) - cax, vy = readlane_f(ecy, i & 63) - cay, vz = readlane_f(ecz, i & 63) - caz;
        const float rb = readlane_f(ecr, i & 63);
        // a sphere / box robot shape is a segment of length 0 with its bounding radius
        float t = __builtin_fmaf(vz, aaz, __builtin_fmaf(vy, aay, vx * aax));
        t = __builtin_fminf(__builtin_fmaxf(t, -shl), shl);
        const float wx = __builtin_fmaf(-t, aax, vx), wy = __builtin_fmaf(-t, aay, vy), wz = __builtin_fmaf(-t, aaz, vz);
        const float w2 = __builtin_fmaf(wz, wz, __builtin_fmaf(wy, wy, wx * wx));
        const float reach = srm + rb;
        if (!kPrismatic) {  // (v_sqrt_f32: 1 ulp, covered by kClearSlack)
          const float lb = __builtin_amdgcn_sqrtf(w2) - reach;
          lb_min = __builtin_fminf(lb_min, ((mine_nib >> (i & 3)) & 1u) ? lb : INFINITY);
        }
        return (w2 > reach * reach) ? 0u : 1u;
      };
#pragma unroll 1
      for (int i = 0; i < on; i += 4) {
        if (!kPrismatic) mine_nib = unsigned(clear_mask >> i) & 0xFu;
        const unsigned nib = cull_one(i) | (cull_one(i + 1) << 1) | (cull_one(i + 2) << 2) | (cull_one(i + 3) << 3);
        mask |= (unsigned long long)nib << i;
      }
      mask &= mine_mask;
      // survivors -> first queue.  A lane whose entries do not all fit writes placeholders into the part of its range
      // that lies inside the queue and keeps its mask for the next turn.
      while (__any(mask != 0ull)) {
        const uint32_t cnt = uint32_t(__popcll(mask));
        uint32_t base = 0u;
        if (cnt) base = atomicAdd(&lds.qn[0], cnt);
        const bool fits = base + cnt <= uint32_t(kQ1Cap);
        if (DIAG && cnt && fits) c_q1 += cnt;
        if (cnt) {
          unsigned long long mm = mask;
          for (uint32_t k = 0; k < cnt; ++k) {
            const int i = __builtin_ctzll(mm);
            mm &= mm - 1ull;
            if (base + k < uint32_t(kQ1Cap)) lds.q1[base + k] = fits ? q_pack(el, rc, o0 + i) : kQEmpty;
          }
          if (fits) mask = 0ull;
        }
        if (__any(mask != 0ull) || lds.qn[0] >= 64u) pair_drain_q1<N>(sc, lds, DIAG ? &c_exact : nullptr, DIAG ? &c_gold : nullptr);
      }
    }
    RKH_STAMP(6)
  }
  pair_drain_q1<N>(sc, lds, DIAG ? &c_exact : nullptr, DIAG ? &c_gold : nullptr);
  pair_drain_q2<N>(sc, lds);
  RKH_STAMP(7)
  if (DIAG) {  // stamps[8..10]: (robot shape, obstacle) pairs past the cull, closed forms evaluated, golden-section searches
    uint32_t v0 = c_q1, v1 = c_exact, v2 = c_gold;
    for (int off = 32; off > 0; off >>= 1) {
      v0 += __shfl_xor(v0, off, 64);
      v1 += __shfl_xor(v1, off, 64);
      v2 += __shfl_xor(v2, off, 64);
    }
    stamps[8] += v0;
    stamps[9] += v1;
    stamps[10] += v2;
  }
  if (!kPrismatic) {  // the edge's two lanes took the robot shapes in turn
    const float other = __int_as_float(xchg_i(__float_as_int(lb_min)));
    clearance = __builtin_fminf(__builtin_fminf(lb_min, other), __builtin_fminf(float(sc->clear_static), kClearMax)) - kClearSlack;
  } else {
    clearance = 0.0f;
  }
  const bool hit = (lds.hit[el] != 0u);
  return !(hit && active);
#undef RKH_STAMP
}

}  // namespace

// All kernel arguments travel in ONE struct and are read through the kernarg segment pointer (scalar loads at the point
// of use, through a laundered pointer).  Referencing by-value parameters directly makes the compiler load every field in
// the entry block and keep it in registers for the whole kernel; a parameter array indexed at run time is even copied to
// scratch.  This kernel has neither registers nor scratch to spare.
struct PairArgs {
  const SceneDev* sc;
  DynDev dyn;
  EdgeIO io_a, io_b;
  const EdgeIO* tab_a;
  const EdgeIO* tab_b;
  uint32_t grid_a;
  double* ws_all;
  KernelGate gate;
};
typedef const __attribute__((address_space(4))) PairArgs* PairArgP;
RKH_DI PairArgP pair_args() {
  PairArgP a = (PairArgP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a));
  return a;
}

// The joint axes of the chain in LDS (PairLds::axis), for the Jacobian columns; ends on a block barrier
template <int N>
RKH_DI void pair_stage_axes(ScenePtr sc, PairLds<N>& lds) {
  if (threadIdx.x < 3 * (N + 1)) {
    const int jj = threadIdx.x / 3;
    lds.axis[jj][threadIdx.x % 3] = sc->joints[jj < N ? jj : N - 1].axis[threadIdx.x % 3];
  }
  __syncthreads();
}

// The rows of edge ec of an EdgeIO record, resolved in two levels of independent loads: every field at once, then the
// words the fields point at (the source row's index, the target offset).  A word the record does not ask for is read
// from the record itself, so that the second level has no branch to wait behind.  The values are meant to die before
// the next f-eval: a kernel resolves again (from the edge's (record, ec)) where it needs rows after one.
// Every caller gets every level, whatever it uses of it (a step launch at k > 0 reads neither si nor a): the record must
// keep src_idx[ec] (or *d_src_first) and *d_tgt_off readable for every edge ec < B in every launch, and x_out allocated
// for B rows before the first one; the step kernel's finishing edges also read best_case[ec] where best_case is set.
struct PairEdgeRows {
  uint32_t si;          // source row index
  const double* a;      // source row
  const double* b;      // target row
  double* x;            // the edge's x_out row
  double* record;       // the launch's record rows (null: none), record_stride states per edge
  int record_stride;
};
template <int D>
RKH_DI PairEdgeRows pair_edge_rows(const EdgeIO* io, uint32_t ec) {
  const double* src = io->src;
  const uint32_t* src_idx = io->src_idx;
  const uint32_t* d_src_first = io->d_src_first;
  const uint32_t src_stride = io->src_stride;
  const double* tgt = io->tgt;
  const uint32_t* d_tgt_off = io->d_tgt_off;
  const uint32_t tgt_stride = io->tgt_stride;
  PairEdgeRows r;
  r.x = io->x_out + uint64_t(ec) * D;
  r.record = io->record;
  r.record_stride = io->record_stride;
  const uint32_t w_src = *(src_idx ? src_idx + ec : (d_src_first ? d_src_first : &io->src_stride));
  const uint32_t w_tgt = *(d_tgt_off ? d_tgt_off : &io->tgt_stride);
  r.si = src_idx ? w_src : ((d_src_first ? w_src : 0u) + ec);
  r.a = src + uint64_t(r.si) * src_stride;
  r.b = tgt + ((d_tgt_off ? uint64_t(w_tgt) : 0ull) + ec) * tgt_stride;
  return r;
}
// D values of a row as independent loads (8 bytes each: neither the bases nor the strides are 16-byte aligned by contract)
template <int D>
RKH_DI void pair_load_row(const double* p, double (&v)[D]) {
#pragma unroll
  for (int d = 0; d < D; ++d) v[d] = p[d];
}

template <int N>
__global__ __launch_bounds__(64, 2) void propagate_pair_kernel(PairArgs) {
  __shared__ PairLds<N> lds;
  typedef PairLayout<N> L_;
  typedef PairWs<N> W_;
  constexpr int D = 2 * N;
  const int lane = threadIdx.x;
  const int h = lane & 1;
  const int el = lane >> 1;
  uint32_t problem, wave;
  bool group_b;
  {
    PairArgP A = pair_args();
    if (A->gate.count) {  // the planner's per-round choice between the kernel mappings
      const uint32_t c = *A->gate.count;
      if (c < A->gate.lo || c >= A->gate.hi) return;
    }
    const uint32_t grid_a = A->grid_a;
    group_b = blockIdx.x >= grid_a;
    problem = blockIdx.y;
    wave = group_b ? blockIdx.x - grid_a : blockIdx.x;
    const uint32_t* wave_base = A->gate.wave_base;
    if (wave_base) {  // compact mapping: block L of the grid (dispatch order) takes working wave L
      const uint32_t n_segments = A->gate.n_segments;
      const uint32_t L = blockIdx.y * gridDim.x + blockIdx.x;
      if (L >= wave_base[n_segments]) return;
      uint32_t lo = 0, hi = n_segments;  // wave_base[lo] <= L < wave_base[hi]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (wave_base[mid] <= L) lo = mid;
        else hi = mid;
      }
      problem = lo >> 1;
      group_b = (lo & 1u) != 0u;
      wave = L - wave_base[lo];
    }
  }
  const ScenePtr sc = (ScenePtr)pair_args()->sc;
  pair_stage_axes<N>((ScenePtr)sc, lds);
  // the launch's EdgeIO record: an entry of a device table, or one of the two by-value copies in the kernarg segment
  auto edge_io = [&]() -> const EdgeIO* {
    PairArgP A = pair_args();
    const EdgeIO* tab = group_b ? A->tab_b : A->tab_a;
    if (A->tab_a) return tab + problem;
    const char* ka = (const char*)(const void*)A;
    return (const EdgeIO*)(ka + (group_b ? offsetof(PairArgs, io_b) : offsetof(PairArgs, io_a)));
  };
  const uint32_t e0 = wave * uint32_t(kPairEdges);
  const uint32_t e = e0 + uint32_t(el);
  bool edge_valid;
  {
    const EdgeIO* io = edge_io();
    const uint32_t B = io->d_B ? *io->d_B : io->B;
    if (e0 >= B) return;
    edge_valid = e < B;
  }
  const bool writer = edge_valid && h == 0;  // the lane that exports the edge's results
  const uint32_t ec = edge_valid ? e : e0;  // idle slots shadow the wave's first edge, results discarded
  PairWsRef ws;
  ws.rsrc = __builtin_amdgcn_make_buffer_rsrc(
      pair_args()->ws_all + (uint64_t(blockIdx.y) * gridDim.x + blockIdx.x) * uint64_t(W_::SLOTS * 64), 0,
      W_::SLOTS * 512, 0x00020000);
  ws.voff = lane * 8;
  {  // the edge's rows -> the workspace: both rows as one batch of loads
    const PairEdgeRows rows = pair_edge_rows<D>(edge_io(), ec);
    double av[D], bv[D];
    pair_load_row<D>(rows.a, av);
    pair_load_row<D>(rows.b, bv);
    double* __restrict__ record = writer ? rows.record : nullptr;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      ws_st(ws, W_::X + d, av[d]);
      ws_st(ws, W_::B + d, bv[d]);
      if (record) record[(uint64_t(ec) * rows.record_stride + 0) * D + d] = av[d];
    }
  }

  uint32_t n_free = 0;
  bool singular = false;
  bool alive = edge_valid;
  uint32_t n_exec = 0;  // steps integrated for this edge (KernelGate::steps_exec)
  // carried clearance of the edge (see kClearSlack): what is left of the last test's bound; 0 = the first step tests
  float budget = 0.0f;
  uint32_t n_settled = 0, n_tested = 0;  // KernelGate::clear_stats: this edge's steps without a test, the wave's tests
  const int n_steps = pair_args()->dyn.n_steps;
#pragma unroll 1
  for (int k = 0; k < n_steps; ++k) {
    // distance(x_current, x_goal) > goal_proximity_threshold (exact left-to-right sum, vect_distance_metrics.hpp:126-137)
    // (the last free state and the target are read once per step, as one batch of workspace loads)
    double xs[D], bv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      xs[d] = ws_ld(ws, W_::X + d);
      bv[d] = ws_ld(ws, W_::B + d);
    }
    {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        RKH_LD(L_::XE + d) = xs[d];  // both lanes of the edge write the same value
        const double df = xs[d] - bv[d];
        s = s + df * df;
      }
      if (!(sqrt(s) > pair_args()->dyn.goal_tol)) alive = false;
    }
    if (!__any(alive)) break;
    if (alive) ++n_exec;
    // PD law, zero-order hold over the step
    {
      PairArgP A = pair_args();
      const double kp = A->dyn.kp, kd = A->dyn.kd, u_max = A->dyn.u_max;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        double v = kp * (bv[2 * j] - xs[2 * j]) + kd * (bv[2 * j + 1] - xs[2 * j + 1]);
        if (v > u_max) v = u_max;
        else if (v < -u_max) v = -u_max;
        RKH_LD(L_::U + j) = v;
      }
    }
    // runge_kutta4_integrate_impl (runge_kutta4_integrator_sys.hpp:53-97): the four useful f-evals per inner step as
    // the stages of a rolled loop (one copy of the dynamics in the instruction stream)
    bool sing_now = false;
    const int n_evals = 4 * int(pair_args()->dyn.inner[k]);
#pragma unroll 1
    for (int ev = 0; ev < n_evals; ++ev) {
      double qdd[N];
      pair_state_derivative<N>(sc, lds, el, h, qdd, sing_now);
      pair_rk4_stage_update<N, W_>(ws, lds, el, h, ev & 3, pair_args()->dyn.dt, qdd);
    }
    pair_lds_handover();  // XE
    if (sing_now && alive) {
      singular = true;
      alive = false;
    }
    // is_free(x_next): hyperbox bounds (hyperbox_topology.hpp:178-189), then proximity
    {
      PairArgP A = pair_args();
      bool oob = false;
#pragma unroll 1
      for (int d = 0; d < D; ++d) {
        const double lo = A->dyn.lower[d], hi = A->dyn.upper[d], xv = RKH_LD(L_::XE + d);
        if (lo < hi) oob = oob || (xv < lo) || (xv > hi);
        else oob = oob || (xv > lo) || (xv < hi);
      }
      if (oob) alive = false;
    }
    if (!__any(alive)) break;
    bool test = true;
    if (!kPrismatic) {
      if (pair_args()->gate.clearance && sc->has_clearance) {
        // delta of this step, from its start (the last free state) to the state to be tested, rounded up
        double q0[N];
#pragma unroll
        for (int j = 0; j < N; ++j) q0[j] = ws_ld(ws, W_::X + 2 * j);
        double dl = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) dl = dl + sc->clear_arm[j] * fabs(RKH_LD(L_::XE + 2 * j) - q0[j]);
        budget -= float(dl) * 1.000001f + kClearStepPad;
        test = __any(alive && !(budget > 0.0f));
      }
    }
    if (test) {  // (uniform) every live edge of the wave takes the fresh bound
      float fresh;
      if (!pair_proximity_free<N>(sc, lds, el, h, alive, fresh)) alive = false;
      budget = fresh;
      ++n_tested;
    } else if (alive) {
      ++n_settled;
    }
    if (alive) {
      ++n_free;
      const EdgeIO* io = edge_io();
      double* __restrict__ record = writer ? io->record : nullptr;
      const int record_stride = io->record_stride;
#pragma unroll 1
      for (int d = 0; d < D; ++d) {
        const double xv = RKH_LD(L_::XE + d);
        ws_st(ws, W_::X + d, xv);
        if (record) record[(uint64_t(ec) * record_stride + n_free) * D + d] = xv;
      }
    }
  }
  const EdgeIO* io = edge_io();
  // the three rows of the accept test / goal probe as one batch of loads
  const PairEdgeRows rows = pair_edge_rows<D>(io, ec);
  const uint32_t si = rows.si;
  double xs[D], av[D], bv[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    xs[d] = ws_ld(ws, W_::X + d);
    bv[d] = ws_ld(ws, W_::B + d);
  }
  pair_load_row<D>(rows.a, av);
  if (singular && writer) atomicExch(io->err_flag, int(RKH_ERR_SINGULAR));
  double s_ar = 0.0, s_ab = 0.0, s_rb = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (writer) rows.x[d] = xs[d];
    const double d_ar = av[d] - xs[d], d_ab = av[d] - bv[d], d_rb = xs[d] - bv[d];
    s_ar = s_ar + d_ar * d_ar;
    s_ab = s_ab + d_ab * d_ab;
    s_rb = s_rb + d_rb * d_rb;
  }
  if (writer) io->steps_free[ec] = n_free;
  if (pair_args()->gate.steps_exec) {
    uint32_t tot = writer ? n_exec : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off, 64);
    if (lane == 0 && tot) atomicAdd(pair_args()->gate.steps_exec, (unsigned long long)tot);
  }
  if (pair_args()->gate.clear_stats) {
    uint32_t tot = writer ? n_settled : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off, 64);
    if (lane == 0 && tot) atomicAdd(pair_args()->gate.clear_stats, (unsigned long long)tot);
    if (lane == 0 && n_tested) atomicAdd(pair_args()->gate.clear_stats + 1, (unsigned long long)n_tested);
  }
  if (io->mode != EDGE_PLAIN && writer) {
    const double n_ar = sqrt(s_ar), n_ab = sqrt(s_ab), n_rb = sqrt(s_rb);
    if (io->mode == EDGE_STEER_ACCEPT) {
      // planning_visitor_base::steer_towards_position (planning_visitors.hpp:349-360)
      io->accept[ec] = uint8_t(edge_accept(EDGE_STEER_ACCEPT, n_ar, n_ab, n_rb, io->best_case, ec, io->steer_tol, kNoWalk));
    } else {
      // C_free distance used by the goal probe (MEAQR_topology.hpp:995-1003)
      io->goal_dist[si - 1] = goal_probe_steerable(n_ab, n_rb);
    }
  }
}

// ---- live edges in full waves: one launch per step -------------------------------------------------------------------
// The same edge arithmetic as propagate_pair_kernel, cut at every step of the steer loop (MEAQR_topology.hpp:503-565:
// integrate one step, test is_free, stop at the first state that is not free).  The edges of a planner round are
// short-lived (tests/diag_edge_lifetimes.py: a candidate survives 9.7 of its 20 steps on average, 21 % end in the
// first), and a wave that carries 32 edges through all of their steps keeps the lanes of the edges that ended idle:
// about half of the lane-steps of propagate_pair_kernel do nothing.  So launch k advances every entry of its input list
// by step k, 32 per wave whatever (problem, candidates | probes) segment they belong to, and appends the survivors to
// the next list.  Launch 0 reads the implicit list of all the round's edges: entry i is found by bisection in the
// exclusive prefix of the segments' edge counts (round_begin_kernel's edge_base).
// Between two steps an edge lives in its x_out row (the state after its last free step).  The order of a list is
// irrelevant: edges are independent and their results are indexed by the edge.
struct PairStepArgs {
  const SceneDev* sc;
  DynDev dyn;
  const EdgeIO* tab_a;        // candidates of problem p
  const EdgeIO* tab_b;        // goal probes of problem p
  double* ws_all;             // RK4 stage vectors, PairStepWs slots x 64 lanes per block of the grid
  KernelGate gate;            // count / lo / hi: the planner's per-round choice between the mappings
  const uint32_t* edge_base;  // [n_segments + 1] exclusive prefix of the edges per segment (segment 2p + g)
  uint32_t n_segments;
  uint32_t step;              // the step this launch integrates
  // step > 0: (segment, edge, carried clearance as float bits, -) of the edges that are still alive, in two parts: the
  // entries expected to need no proximity test in this launch from the front ([0, cnt_in[0])), the others from the back
  // ([list_cap - cnt_in[kStepCntBack], list_cap)), so that whole waves can skip the test.  The sorting is a prediction
  // only: every wave checks the real budgets of its edges.
  const uint4* list_in;
  const uint32_t* cnt_in;
  uint4* list_out;            // survivors of this launch
  uint32_t* cnt_out;
  uint32_t list_cap;          // entries of each list
  unsigned long long* steps_exec;  // optional: + the number of edge-steps this launch integrated
  // A round that carries (carry_round of the gate's count, round_carry.h; kCarryOff: none does): launch 0 reads list_in
  // too -- the edges carry_restore_kernel left to steer, all with clearance 0 in the front part -- instead of the
  // implicit list of edge_base.  What launch 0 does because it integrates step 0 stays keyed on the step.
  uint32_t carry_min_edges;
};
constexpr uint32_t kStepCntBack = uint32_t(kMaxSteps) + 1u;  // d_cnt[kStepCntBack + k]: back entries of the list launch k reads
typedef const __attribute__((address_space(4))) PairStepArgs* PairStepArgP;
RKH_DI PairStepArgP pair_step_args() {
  PairStepArgP a = (PairStepArgP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a));
  return a;
}
template <int N>
struct PairStepWs {  // per-lane private RK4 values (this lane's joints: 2 components each)
  enum : int { R = (N + 1) / 2, W = 0, KA = 2 * R, K3 = 4 * R, SLOTS = 6 * R };
};

template <int N>
__global__ __launch_bounds__(64, 2) void propagate_pair_step_kernel(PairStepArgs) {
  __shared__ PairLds<N> lds;
  typedef PairLayout<N> L_;
  typedef PairStepWs<N> W_;
  constexpr int R = L_::R;
  constexpr int D = 2 * N;
  const int lane = threadIdx.x;
  const int h = lane & 1;
  const int el = lane >> 1;
  uint32_t n_front, n_back;
  bool listed;  // (uniform) this launch takes its edges from list_in
  {
    PairStepArgP A = pair_step_args();
    listed = A->step != 0u;
    if (A->gate.count) {
      const uint32_t c = *A->gate.count;
      if (c < A->gate.lo || c >= A->gate.hi) return;
      listed = listed || carry_round(c, A->gate.lo, A->gate.hi, A->carry_min_edges);
    }
    n_front = listed ? A->cnt_in[0] : A->edge_base[A->n_segments];
    n_back = listed ? A->cnt_in[kStepCntBack] : 0u;
  }
  const uint32_t chunks_front = (n_front + uint32_t(kPairEdges) - 1u) / uint32_t(kPairEdges);
  const uint32_t n_chunks = chunks_front + (n_back + uint32_t(kPairEdges) - 1u) / uint32_t(kPairEdges);
  if (blockIdx.x >= n_chunks) return;
  const ScenePtr sc = (ScenePtr)pair_step_args()->sc;
  pair_stage_axes<N>((ScenePtr)sc, lds);
  PairWsRef ws;
  ws.rsrc = __builtin_amdgcn_make_buffer_rsrc(pair_step_args()->ws_all + uint64_t(blockIdx.x) * uint64_t(W_::SLOTS * 64), 0,
                                              W_::SLOTS * 512, 0x00020000);
  ws.voff = lane * 8;
  const int n_steps = pair_step_args()->dyn.n_steps;
  const int k = int(pair_step_args()->step);
#pragma unroll 1
  for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const bool back = chunk >= chunks_front;  // (uniform)
    const uint32_t i0 = (back ? chunk - chunks_front : chunk) * uint32_t(kPairEdges);
    const bool edge_valid = i0 + uint32_t(el) < (back ? n_back : n_front);
    const uint32_t ic = edge_valid ? i0 + uint32_t(el) : i0;  // idle slots shadow the chunk's first edge
    // the lane pair's edge (both lanes of a pair hold the same values)
    uint32_t seg, ec;
    float budget = 0.0f;  // carried clearance (launch 0 has none: it tests)
    if (!listed) {  // entry ic of the round's implicit list: bisection in the prefix of the segments' edge counts
      const uint32_t* eb = pair_step_args()->edge_base;
      uint32_t lo = 0, hi = pair_step_args()->n_segments;  // eb[lo] <= ic < eb[hi]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (eb[mid] <= ic) lo = mid;
        else hi = mid;
      }
      seg = lo;
      ec = ic - eb[lo];
    } else {
      const uint4 ent = pair_step_args()->list_in[back ? pair_step_args()->list_cap - 1u - ic : ic];
      seg = ent.x;
      ec = ent.y;
      budget = __uint_as_float(ent.z);
    }
    const bool writer = edge_valid && h == 0;  // the lane that exports the edge's results
    // the edge's EdgeIO record: both tables' addresses are scalar kernarg loads, selected per lane (left to itself the
    // compiler selects the kernarg address and loads it per lane: a memory round trip)
    auto edge_io = [&]() -> const EdgeIO* {
      PairStepArgP A = pair_step_args();
      const EdgeIO* ta = A->tab_a;
      const EdgeIO* tb = A->tab_b;
      asm volatile("" : "+s"(ta), "+s"(tb));
      return ((seg & 1u) ? tb : ta) + (seg >> 1);
    };
    // the state the edge has reached (its source row, or what the step before left in x_out), the steer target, and
    // distance(x_current, x_goal) > goal_proximity_threshold (exact left-to-right sum, vect_distance_metrics.hpp:126-137).
    // Both rows are one batch of loads; what the step needs of them goes to LDS (XE, U) before the first f-eval.
    bool alive = edge_valid;
    bool singular = false;
    float step_delta = 0.0f;  // this step's bound on the motion of the robot's points
    {
      const PairEdgeRows rows = pair_edge_rows<D>(edge_io(), ec);
      double xs[D], bv[D];
      pair_load_row<D>(k ? rows.x : rows.a, xs);
      pair_load_row<D>(rows.b, bv);
      double* __restrict__ first = (k == 0 && writer) ? rows.x : nullptr;
      double* __restrict__ record = (k == 0 && writer) ? rows.record : nullptr;
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        RKH_LD(L_::XE + d) = xs[d];  // both lanes of the edge write the same value
        if (first) first[d] = xs[d];  // an edge that ends in its first step stays at its source
        if (record) record[(uint64_t(ec) * rows.record_stride + 0) * D + d] = xs[d];
        const double df = xs[d] - bv[d];
        s = s + df * df;
      }
      if (!(sqrt(s) > pair_step_args()->dyn.goal_tol)) alive = false;
      // PD law, zero-order hold over the step (read by the f-evals only: a wave without a live edge runs none)
      PairStepArgP A = pair_step_args();
      const double kp = A->dyn.kp, kd = A->dyn.kd, u_max = A->dyn.u_max;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        double v = kp * (bv[2 * j] - xs[2 * j]) + kd * (bv[2 * j + 1] - xs[2 * j + 1]);
        if (v > u_max) v = u_max;
        else if (v < -u_max) v = -u_max;
        RKH_LD(L_::U + j) = v;
      }
    }
    if (__any(alive)) {
      if (pair_step_args()->steps_exec) {
        const unsigned long long m = __ballot(alive && h == 0);
        if (lane == 0) atomicAdd(pair_step_args()->steps_exec, (unsigned long long)__popcll(m));
      }
      // runge_kutta4_integrate_impl (runge_kutta4_integrator_sys.hpp:53-97), see propagate_pair_kernel
      bool sing_now = false;
      const int n_evals = 4 * int(pair_step_args()->dyn.inner[k]);
#pragma unroll 1
      for (int ev = 0; ev < n_evals; ++ev) {
        double qdd[N];
        pair_state_derivative<N>(sc, lds, el, h, qdd, sing_now);
        pair_rk4_stage_update<N, W_>(ws, lds, el, h, ev & 3, pair_step_args()->dyn.dt, qdd);
      }
      pair_lds_handover();  // XE
      if (sing_now && alive) {
        singular = true;
        alive = false;
      }
      // is_free(x_next): hyperbox bounds (hyperbox_topology.hpp:178-189), then proximity
      {
        PairStepArgP A = pair_step_args();
        bool oob = false;
#pragma unroll 1
        for (int d = 0; d < D; ++d) {
          const double lo = A->dyn.lower[d], hi = A->dyn.upper[d], xv = RKH_LD(L_::XE + d);
          if (lo < hi) oob = oob || (xv < lo) || (xv > hi);
          else oob = oob || (xv > lo) || (xv < hi);
        }
        if (oob) alive = false;
      }
      if (__any(alive)) {
        bool test = true;
        if (!kPrismatic) {
          if (pair_step_args()->gate.clearance && sc->has_clearance) {
            // delta of this step: from the state the launch read to the state to be tested, rounded up.  The start's
            // angles are in the workspace's W slots (the lane's own joints; the neighbour's come by DPP) unless the
            // step had inner sub-steps: then W holds only the last one's start, and the edge's row is read again.
            double q0[N];
            if (n_evals == 4) {  // (uniform) one RK4 iteration: dyn.inner[k] == 1
              double own[R];
#pragma unroll
              for (int jr = 0; jr < R; ++jr) own[jr] = ws_ld(ws, W_::W + 2 * jr);
#pragma unroll
              for (int jr = 0; jr < R; ++jr) {
                const double oth = xchg(own[jr]);
                q0[2 * jr] = h ? oth : own[jr];
                if (2 * jr + 1 < N) q0[2 * jr + 1] = h ? own[jr] : oth;
              }
            } else {
              const PairEdgeRows rows = pair_edge_rows<D>(edge_io(), ec);
              const double* __restrict__ a_row = k ? rows.x : rows.a;
#pragma unroll
              for (int j = 0; j < N; ++j) q0[j] = a_row[2 * j];
            }
            double dl = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) dl = dl + sc->clear_arm[j] * fabs(RKH_LD(L_::XE + 2 * j) - q0[j]);
            step_delta = float(dl) * 1.000001f + kClearStepPad;
            budget -= step_delta;
            test = __any(alive && !(budget > 0.0f));
          }
        }
        unsigned long long* cs = pair_step_args()->gate.clear_stats;
        if (test) {  // (uniform) every live edge of the wave takes the fresh bound
          float fresh;
          if (!pair_proximity_free<N>(sc, lds, el, h, alive, fresh)) alive = false;
          budget = fresh;
          if (cs && lane == 0) atomicAdd(cs + 1, 1ull);
        } else if (cs) {
          const unsigned long long m = __ballot(alive && h == 0);
          if (lane == 0) atomicAdd(cs, (unsigned long long)__popcll(m));
        }
      }
    }
    // ---- the step's outcome: alive = step k was free (the edge stands at the new state), else it stays where it was
    const bool go_on = alive && (k + 1 < n_steps);
    const bool finished = edge_valid && !go_on;
    const uint32_t n_free = uint32_t(k) + (alive ? 1u : 0u);
    if (alive) {
      const EdgeIO* io = edge_io();
      double* const x_out = io->x_out;  // (the three fields as one batch of loads)
      double* const rec = io->record;
      const int record_stride = io->record_stride;
      double* __restrict__ xo = writer ? x_out + uint64_t(ec) * D : nullptr;
      double* __restrict__ record = writer ? rec : nullptr;
      if (xo) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const double xv = RKH_LD(L_::XE + d);
          xo[d] = xv;
          if (record) record[(uint64_t(ec) * record_stride + n_free) * D + d] = xv;
        }
      }
    }
    {  // survivors -> the next launch's list: from the front if the budget should last through the next step (it moves
       // about as far as this one), else from the back
      const bool quiet = budget > 2.0f * step_delta;  // (budgets are 0 where the clearance is off: all to the back)
      const unsigned long long mf = __ballot(go_on && h == 0 && quiet), mb = __ballot(go_on && h == 0 && !quiet);
      if (mf | mb) {
        PairStepArgP A = pair_step_args();
        uint32_t base_f = 0, base_b = 0;
        if (lane == 0 && mf) base_f = atomicAdd(A->cnt_out, uint32_t(__popcll(mf)));
        if (lane == 0 && mb) base_b = atomicAdd(A->cnt_out + kStepCntBack, uint32_t(__popcll(mb)));
        base_f = uint32_t(__builtin_amdgcn_readfirstlane(int(base_f)));
        base_b = uint32_t(__builtin_amdgcn_readfirstlane(int(base_b)));
        const unsigned long long below = (1ull << lane) - 1ull;
        if (go_on && h == 0) {
          const uint32_t at = quiet ? base_f + uint32_t(__popcll(mf & below))
                                    : A->list_cap - 1u - (base_b + uint32_t(__popcll(mb & below)));
          A->list_out[at] = make_uint4(seg, ec, __float_as_uint(budget), 0u);
        }
      }
    }
    if (__any(finished)) {  // accept test / goal probe of the edges that end here
      // Resolved again from (seg, ec): nothing of the prologue's batch lives through the f-evals.  Every field the
      // verdict can need comes with the first level, the best-case distance with the second, the three rows in a third.
      const EdgeIO* io = edge_io();
      const int mode = io->mode;
      uint32_t* const steps_free = io->steps_free;
      uint8_t* const accept = io->accept;
      double* const goal_dist = io->goal_dist;
      const double* const best_case = io->best_case;
      const double steer_tol = io->steer_tol;
      int* const err_flag = io->err_flag;
      const double bc = *(best_case ? best_case + ec : &io->steer_tol);
      const PairEdgeRows rows = pair_edge_rows<D>(io, ec);
      double av[D], bv[D], xr[D];
      pair_load_row<D>(rows.a, av);
      pair_load_row<D>(rows.b, bv);
      pair_load_row<D>(rows.x, xr);  // written above (alive: not used) or by an earlier step (k > 0)
      if (singular && writer) atomicExch(err_flag, int(RKH_ERR_SINGULAR));
      double s_ar = 0.0, s_ab = 0.0, s_rb = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double xv = alive ? RKH_LD(L_::XE + d) : (k ? xr[d] : av[d]);
        const double d_ar = av[d] - xv, d_ab = av[d] - bv[d], d_rb = xv - bv[d];
        s_ar = s_ar + d_ar * d_ar;
        s_ab = s_ab + d_ab * d_ab;
        s_rb = s_rb + d_rb * d_rb;
      }
      if (finished && writer) {
        steps_free[ec] = n_free;
        if (mode != EDGE_PLAIN) {
          const double n_ar = sqrt(s_ar), n_ab = sqrt(s_ab), n_rb = sqrt(s_rb);
          if (mode == EDGE_STEER_ACCEPT) {
            // planning_visitor_base::steer_towards_position (planning_visitors.hpp:349-360)
            accept[ec] = uint8_t(edge_accept(EDGE_STEER_ACCEPT, n_ar, n_ab, n_rb, best_case ? &bc : nullptr, 0u, steer_tol, kNoWalk));
          } else {
            // C_free distance used by the goal probe (MEAQR_topology.hpp:995-1003)
            goal_dist[rows.si - 1] = goal_probe_steerable(n_ab, n_rb);
          }
        }
      }
    }
  }
}

#ifndef RKH_PRISMATIC_FORMS  // (the workspace does not depend on the joint kinds)
size_t propagate_pair_step_workspace_bytes(int n_dof, uint32_t blocks) {
  return size_t(blocks) * size_t(6 * ((n_dof + 1) / 2)) * 64 * sizeof(double);
}
#endif

// The steer launches of a round, one per step, over two ping-pong lists of list_cap entries; d_cnt[k] and
// d_cnt[kStepCntBack + k] = front and back entries of the list launch k reads (d_cnt[0 .. 2 kMaxSteps + 1] must be zero
// when the first launch starts: round_begin_kernel clears them).  `blocks` bounds the
// grids; a launch with more chunks than blocks strides over them.
rkh_status launch_propagate_pair_steps(hipStream_t s, const rkh_scene& scene, const DynDev& dyn, const EdgeIO* tab_a,
                                       const EdgeIO* tab_b, uint32_t n_problems, const uint32_t* d_edge_base,
                                       uint4* d_list0, uint4* d_list1, uint32_t list_cap, uint32_t* d_cnt, double* d_ws,
                                       uint32_t blocks, KernelGate gate, unsigned long long* d_steps_exec,
                                       uint32_t carry_min_edges) {
  if (blocks == 0 || n_problems == 0) return RKH_OK;
  if constexpr (!kPrismatic)
    if (scene.host.has_prismatic)
      return prismatic::launch_propagate_pair_steps(s, scene, dyn, tab_a, tab_b, n_problems, d_edge_base, d_list0, d_list1,
                                                    list_cap, d_cnt, d_ws, blocks, gate, d_steps_exec, carry_min_edges);
  PairStepArgs args;
  args.sc = scene.d_scene.get();
  args.dyn = dyn;
  args.tab_a = tab_a;
  args.tab_b = tab_b;
  args.ws_all = d_ws;
  args.gate = gate;
  args.edge_base = d_edge_base;
  args.n_segments = 2 * n_problems;
  args.steps_exec = d_steps_exec;
  args.list_cap = list_cap;
  args.carry_min_edges = carry_min_edges;
  const rkh_status st = with_n<1, 2, 3, 4, 6, 7>(scene.host.n_dof, [&](auto c) {
    for (int k = 0; k < dyn.n_steps; ++k) {
      args.step = uint32_t(k);
      args.list_in = (k & 1) ? d_list1 : d_list0;
      args.list_out = (k & 1) ? d_list0 : d_list1;
      args.cnt_in = d_cnt + k;
      args.cnt_out = d_cnt + k + 1;
      hipLaunchKernelGGL((propagate_pair_step_kernel<decltype(c)::value>), dim3(blocks), dim3(64), 0, s, args);
    }
  });
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

#ifndef RKH_PRISMATIC_FORMS  // the cycle probe instruments the revolute form only
// Diagnostic kernel (not on the product path): `iters` back-to-back f-evals + proximity tests of kPairEdges states per
// wave with cycle counts per phase: [frames + sincos, jacobian columns, mass matrix, force sweep, assembly + cholesky,
// proximity: joint frames, cull, exact routines]
template <int N>
__global__ __launch_bounds__(64, 2) void pair_cycles_kernel(const SceneDev* __restrict__ sc, const double* __restrict__ x,
                                                             const double* __restrict__ u, uint32_t B, int iters,
                                                             unsigned long long* __restrict__ out,
                                                             double* __restrict__ sink_out) {
  __shared__ PairLds<N> lds;
  pair_stage_axes<N>((ScenePtr)sc, lds);
  typedef PairLayout<N> L_;
  const int lane = threadIdx.x, h = lane & 1, el = lane >> 1;
  uint32_t e = blockIdx.x * kPairEdges + el;
  if (e >= B) e = blockIdx.x * kPairEdges;
  for (int d = 0; d < 2 * N; ++d) RKH_LD(L_::XE + d) = x[uint64_t(e) * 2 * N + d];
  for (int j = 0; j < N; ++j) RKH_LD(L_::U + j) = u[uint64_t(e) * N + j];
  unsigned long long st[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool singular = false;
  double accv = 0.0;
  for (int it = 0; it < iters; ++it) {
    double qdd[N];
    pair_state_derivative<N, true>((ScenePtr)sc, lds, el, h, qdd, singular, st);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      accv += qdd[j];
      RKH_LD(L_::XE + 2 * j + 1) = RKH_LD(L_::XE + 2 * j + 1) + 1e-4 * qdd[j];
    }
    float clearance;
    accv += pair_proximity_free<N, true>((ScenePtr)sc, lds, el, h, true, clearance, st) ? 1.0 : 0.0;
  }
  if (lane == 0) {
    for (int i = 0; i < 8; ++i) out[blockIdx.x * 8 + i] = st[i];
    sink_out[blockIdx.x] = accv + (singular ? 1.0 : 0.0);
  }
}
#endif

// Diagnostic kernel (not on the product path): the proximity test of B states, 32 per wave, counting what survives each
// stage: out[0] += states tested, [1] += (robot shape, obstacle) pairs past the static reach + fp32 cull (the closed-form
// stage's input), [2] += closed forms evaluated, [3] += golden-section searches (capped cylinder / box), [4] += states
// found in collision.  clear_out (optional): the clearance bound of every state, as the steer kernels carry it.
template <int N>
__global__ __launch_bounds__(64, 2) void pair_counts_kernel(const SceneDev* __restrict__ sc, const double* __restrict__ x,
                                                             uint32_t B, unsigned long long* __restrict__ out,
                                                             float* __restrict__ clear_out) {
  __shared__ PairLds<N> lds;
  pair_stage_axes<N>((ScenePtr)sc, lds);
  typedef PairLayout<N> L_;
  const int lane = threadIdx.x, h = lane & 1, el = lane >> 1;
  const uint32_t e = blockIdx.x * kPairEdges + el;
  const bool valid = e < B;
  const uint32_t es = valid ? e : blockIdx.x * kPairEdges;
  for (int d = 0; d < 2 * N; ++d) RKH_LD(L_::XE + d) = x[uint64_t(es) * 2 * N + d];
  unsigned long long st[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  float clearance;
  const bool free_state = pair_proximity_free<N, true>((ScenePtr)sc, lds, el, h, true, clearance, st);
  if (clear_out && valid && h == 0) clear_out[e] = clearance;  // rkh_diag_proximity_clearance
  const unsigned long long hits = __ballot(!free_state && valid && h == 0);
  if (lane == 0) {
    const uint32_t n_here = (B - blockIdx.x * kPairEdges) < uint32_t(kPairEdges) ? (B - blockIdx.x * kPairEdges) : uint32_t(kPairEdges);
    atomicAdd(&out[0], (unsigned long long)n_here);
    atomicAdd(&out[1], st[8]);
    atomicAdd(&out[2], st[9]);
    atomicAdd(&out[3], st[10]);
    atomicAdd(&out[4], (unsigned long long)__popcll(hits));
  }
}

rkh_status launch_pair_counts(hipStream_t s, const rkh_scene& scene, const double* d_x, uint32_t B,
                              unsigned long long* d_out, float* d_clear_out) {
  if constexpr (!kPrismatic)
    if (scene.host.has_prismatic) return prismatic::launch_pair_counts(s, scene, d_x, B, d_out, d_clear_out);
  const uint32_t waves = (B + kPairEdges - 1) / kPairEdges;
  const rkh_status st = with_n<6, 3, 7>(scene.host.n_dof, [&](auto c) {
    hipLaunchKernelGGL((pair_counts_kernel<decltype(c)::value>), dim3(waves), dim3(64), 0, s, scene.d_scene.get(), d_x, B, d_out,
                       d_clear_out);
  });
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

#ifndef RKH_PRISMATIC_FORMS
rkh_status launch_pair_cycles(hipStream_t s, const rkh_scene& scene, const double* d_x, const double* d_u, uint32_t B,
                              int iters, unsigned long long* d_out, double* d_sink) {
  if (scene.host.has_prismatic) {
    set_error("rkh_diag_feval_cycles: scenes with prismatic joints are not instrumented");
    return RKH_ERR_UNSUPPORTED;
  }
  const uint32_t waves = (B + kPairEdges - 1) / kPairEdges;
  const rkh_status st = with_n<6, 3>(scene.host.n_dof, [&](auto c) {
    hipLaunchKernelGGL((pair_cycles_kernel<decltype(c)::value>), dim3(waves), dim3(64), 0, s, scene.d_scene.get(), d_x, d_u, B,
                       iters, d_out, d_sink);
  });
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  RKH_HIP(hipStreamSynchronize(s));
  return RKH_OK;
}

// bytes of workspace a launch of (edges_a + edges_b) edges per problem needs
size_t propagate_pairs_workspace_bytes(int n_dof, uint32_t edges_a, uint32_t edges_b, uint32_t n_problems) {
  const size_t waves = size_t((edges_a + kPairEdges - 1) / kPairEdges + (edges_b + kPairEdges - 1) / kPairEdges) * n_problems;
  const size_t slots = size_t(6 * ((n_dof + 1) / 2) + 4 * n_dof);
  return waves * slots * 64 * sizeof(double);
}
#endif

rkh_status launch_propagate_pairs(hipStream_t s, const rkh_scene& scene, const DynDev& dyn, const EdgeIO& io,
                                  uint32_t grid_edges, uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                                  uint32_t n_problems, double* d_ws, KernelGate gate) {
  const uint32_t eb = tab_b ? grid_b : 0u;
  if (grid_edges + eb == 0 || n_problems == 0) return RKH_OK;
  if (!d_ws) {
    set_error("propagate (two lanes per edge): no workspace");
    return RKH_ERR_BAD_ARG;
  }
  if constexpr (!kPrismatic)
    if (scene.host.has_prismatic)
      return prismatic::launch_propagate_pairs(s, scene, dyn, io, grid_edges, eb, tab_a, tab_b, n_problems, d_ws, gate);
  const uint32_t ga = (grid_edges + kPairEdges - 1) / kPairEdges, gbk = (eb + kPairEdges - 1) / kPairEdges;
  PairArgs args;
  args.sc = scene.d_scene.get();
  args.dyn = dyn;
  args.io_a = io;
  args.io_b = EdgeIO();
  args.tab_a = tab_a;
  args.tab_b = tab_b;
  args.grid_a = ga;
  args.ws_all = d_ws;
  args.gate = gate;
  const rkh_status st = with_n<1, 2, 3, 4, 6, 7>(scene.host.n_dof, [&](auto c) {
    hipLaunchKernelGGL((propagate_pair_kernel<decltype(c)::value>), dim3(ga + gbk, n_problems), dim3(64), 0, s, args);
  });
  if (st != RKH_OK) return st;
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

#ifndef RKH_PRISMATIC_FORMS
uint32_t pair_kernel_edges_per_wave() { return uint32_t(kPairEdges); }
#endif

// resident waves per CU of the kernel for this chain size (and joint kinds: has_prismatic = the scene's)
uint32_t pair_kernel_waves_per_cu(int n_dof, bool has_prismatic) {
  if constexpr (!kPrismatic)
    if (has_prismatic) return prismatic::pair_kernel_waves_per_cu(n_dof, true);
  int blocks = 0;
  hipError_t e = hipErrorInvalidValue;
  with_n<1, 2, 3, 4, 6, 7>(n_dof, [&](auto c) {
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, propagate_pair_kernel<decltype(c)::value>, 64, 0);
  });
  return (e == hipSuccess && blocks > 0) ? uint32_t(blocks) : 8u;
}

#undef RKH_LD
#ifdef RKH_PRISMATIC_FORMS
}  // namespace prismatic
#endif
}  // namespace rkh
