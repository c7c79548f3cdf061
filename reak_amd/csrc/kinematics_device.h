// kinematics_device.h -- direct kinematics, Jacobians and the damped least-squares pose step of a KTE chain, per lane.
//
// What it restates (reference paths relative to src/ReaK/):
//   kte_map_chain::doMotion with q'' = 0, pose and rates of one frame: revolute_joint.cpp:121-148 (2D :30-56),
//   prismatic_joint.cpp:116-148 (2D :44-62), rigid_link.cpp:152-156 (2D :87-99), frame_3D::addBefore(pose).
//   jacobian_gen_3D::get_jac_relative_to (core/kinetostatics/motion_jacobians.hpp:238-251) and jacobian_gen_2D's
//   (:138-146) for the generators the joints register: revolute qd_avel = mAxis, prismatic qd_vel = mAxis, the rest 0.
//
// A frame is carried as the reference carries a parentless frame_3D: Position and Velocity in world coordinates, Quat,
// AngVelocity in the frame's OWN coordinates.  The pose part runs in the operation order of proximity_frames
// (propagate.hip), so a pose from here is bit for bit the pose the distance query gives its shapes.
//
// Jacobian columns are evaluated in their world form.  With joint i's end frame (p_i, R_i, v_i, W_i = R_i w_i), the asked
// frame (p, R, v, W = R w), d = p - p_i and A = R_i mAxis, the reference's f2 = frame relative to the joint's end frame is
//   f2.Position = R_i^T d,  rotmat(f2.Quat) = R_i^T R,  f2.Velocity = R_i^T (v - v_i - W_i x d),  f2.AngVelocity = R^T (W - W_i)
// and get_jac_relative_to's four lines become
//   v    = R^T (A x d)  (prismatic: R^T A)            w    = R^T A  (prismatic: 0)
//   vdot = R^T (A x (v - v_i - W_i x d)) - f2.AngVelocity x v      (prismatic: the second term alone)
//   wdot = - f2.AngVelocity x w
// the same numbers up to rounding, without inverting a frame per column.
//
// Nothing here uses a device builtin: with the stand-in for <hip/hip_runtime.h> a host compiler reads this header and
// device_math.h / proximity_planar_device.h as they are (tests/cpp/kinematics_host.cpp).
#pragma once
#include <stdint.h>

#include "device_math.h"
#include "proximity_planar_device.h"

namespace rkh {

constexpr int kKinMaxDof = 12;  // = kMaxDof (rkh_internal.h)

// One joint group of the chain as the scene builder flattened it: [mount link from the base] joint, link.
struct KinJoint {
  double axis[3];        // mAxis as given (the generator, and a prismatic joint's travel direction)
  double axis_n[3];      // axis_angle's normalised copy (the revolute rotation)
  double off_pos[3];     // the link's pose offset (planar: [0..1], and off_quat[0..1] = (cos, sin))
  double off_quat[4];
  double mount_pos[3];   // branch_start: rigid link from the chain base that carries this joint (identity if none)
  double mount_quat[4];
  int32_t prismatic;
  int32_t branch_start;
};
struct KinChain {
  int32_t n_dof;
  int32_t planar;
  double base_pos[3];
  double base_quat[4];
  KinJoint joints[kKinMaxDof];
};

// Where a frame of the caller's numbering sits in the flattened chain.
enum KinFrameKind : int32_t { KIN_INVALID = 0, KIN_BASE = 1, KIN_MOUNT = 2, KIN_JOINT_END = 3, KIN_LINK_END = 4 };
struct KinFrameRef {
  int32_t kind;    // KinFrameKind
  int32_t first;   // first joint of the branch the frame hangs on
  int32_t last;    // the frame's own joint group (KIN_MOUNT: the group the mount carries)
  uint32_t up;     // upstream joints: up[end] = up[base] | bit(coord) over the op program
};

struct KinFrame {  // frame_3D without a parent
  d3 p;  // Position, world
  d4 Q;  // Quat
  d3 v;  // Velocity, world
  d3 w;  // AngVelocity, the frame's own coordinates
};
struct KinFrame2 {  // frame_2D without a parent
  d2 p, R, v;  // Position, Rotation (cos, sin), Velocity
  double w;    // AngVelocity
};

RKH_DI d3 kin_ld3(const double* a) { return d3{a[0], a[1], a[2]}; }
RKH_DI d4 kin_ld4(const double* a) { return d4{a[0], a[1], a[2], a[3]}; }
RKH_DI d2 kin_ld2(const double* a) { return d2{a[0], a[1]}; }

// doMotion from the chain base to frame `fr`.  q / qd are read at [j * stride]; qd may be null (zero rates).  at(j, E)
// is called with the END frame of every joint on the way (joint `last` included unless the walk ends before it).
template <bool VEL, class AtJoint>
RKH_DI KinFrame kin_walk(const KinChain& C, const KinFrameRef& fr, const double* q, const double* qd, int stride,
                         AtJoint&& at) {
  KinFrame f;
  f.p = kin_ld3(C.base_pos);
  f.Q = kin_ld4(C.base_quat);
  f.v = mk3(0.0, 0.0, 0.0);
  f.w = mk3(0.0, 0.0, 0.0);
  if (fr.kind == KIN_BASE) return f;
  for (int j = fr.first; j <= fr.last; ++j) {
    const KinJoint& J = C.joints[j];
    if (J.branch_start) {  // rigid_link_3D::doMotion from frame 0 (the base is at rest)
      const d4 bq = kin_ld4(C.base_quat);
      f.p = kin_ld3(C.base_pos) + mul(rotmat(bq), kin_ld3(J.mount_pos));
      f.Q = qmul(bq, kin_ld4(J.mount_quat));
      f.v = mk3(0.0, 0.0, 0.0);
      f.w = mk3(0.0, 0.0, 0.0);
    }
    if (fr.kind == KIN_MOUNT) return f;
    const double qj = q[j * stride];
    const double qdj = (VEL && qd) ? qd[j * stride] : 0.0;
    const d3 axis = kin_ld3(J.axis);
    if (J.prismatic) {  // prismatic_joint.cpp:116-148
      const m33 R = rotmat(f.Q);
      const d3 tp = qj * axis;
      if (VEL) f.v = f.v + mul(R, cross(f.w, tp) + qdj * axis);
      f.p = f.p + mul(R, tp);
    } else {  // revolute_joint.cpp:121-148
      double s2, c2;
      sincos(0.5 * qj, &s2, &c2);
      const d3 an = kin_ld3(J.axis_n);
      const d4 tq = d4{c2, an.x * s2, an.y * s2, an.z * s2};
      if (VEL) f.w = mulT(f.w, rotmat(tq)) + qdj * axis;
      f.Q = qmul(f.Q, tq);
    }
    at(j, f);
    if (j == fr.last && fr.kind == KIN_JOINT_END) return f;
    {  // rigid_link.cpp:152-156 = frame_3D::addBefore(pose)
      const m33 R = rotmat(f.Q);
      const d3 P = kin_ld3(J.off_pos);
      const d4 PQ = kin_ld4(J.off_quat);
      if (VEL) f.v = f.v + mul(R, cross(f.w, P));
      f.p = f.p + mul(R, P);
      if (VEL) f.w = mulT(f.w, rotmat(PQ));
      f.Q = qmul(f.Q, PQ);
    }
  }
  return f;
}

struct KinCol {  // one column of Jac / JacDot: rows (velocity, angular velocity), the asked frame's coordinates
  d3 v, w, vd, wd;
};
// Column of the joint with end frame E (its generator along `axis`) for the asked frame T; RT = rotmat(T.Q), WT = RT T.w.
template <bool DOT>
RKH_DI KinCol kin_column(bool prismatic, d3 axis, const KinFrame& E, const KinFrame& T, const m33& RT, d3 WT) {
  const m33 RE = rotmat(E.Q);
  const d3 A = mul(RE, axis);
  const d3 d = T.p - E.p;
  KinCol c;
  c.v = mulT(prismatic ? A : cross(A, d), RT);
  c.w = prismatic ? mk3(0.0, 0.0, 0.0) : mulT(A, RT);
  c.vd = c.wd = mk3(0.0, 0.0, 0.0);
  if (DOT) {
    const d3 WE = mul(RE, E.w);
    const d3 rel_w = mulT(WT - WE, RT);  // f2.AngVelocity
    const d3 lin = prismatic ? mk3(0.0, 0.0, 0.0) : mulT(cross(A, (T.v - E.v) - cross(WE, d)), RT);
    c.vd = lin - cross(rel_w, c.v);
    c.wd = mk3(0.0, 0.0, 0.0) - cross(rel_w, c.w);
  }
  return c;
}

// ---- planar chains ---------------------------------------------------------------------------------------------------
RKH_DI d2 kin_perp(d2 v, double s) { return d2{-v.y * s, v.x * s}; }  // scalar % vect (vect_alg.hpp:1171-1176)

template <bool VEL, class AtJoint>
RKH_DI KinFrame2 kin_walk2(const KinChain& C, const KinFrameRef& fr, const double* q, const double* qd, int stride,
                           AtJoint&& at) {
  KinFrame2 f;
  f.p = kin_ld2(C.base_pos);
  f.R = kin_ld2(C.base_quat);
  f.v = mk2(0.0, 0.0);
  f.w = 0.0;
  if (fr.kind == KIN_BASE) return f;
  for (int j = fr.first; j <= fr.last; ++j) {
    const KinJoint& J = C.joints[j];
    const double qj = q[j * stride];
    const double qdj = (VEL && qd) ? qd[j * stride] : 0.0;
    if (J.prismatic) {  // prismatic_joint.cpp:44-62
      const d2 axis = kin_ld2(J.axis);
      const d2 tp = qj * axis;
      if (VEL) f.v = f.v + rrot(f.R, kin_perp(tp, f.w) + qdj * axis);
      f.p = f.p + rrot(f.R, tp);
    } else {  // revolute_joint.cpp:30-56
      double sn, cs;
      sincos(qj, &sn, &cs);
      f.R = rmul(f.R, mk2(cs, sn));
      if (VEL) f.w = f.w + qdj;
    }
    at(j, f);
    if (j == fr.last && fr.kind == KIN_JOINT_END) return f;
    {  // rigid_link.cpp:87-99
      const d2 P = kin_ld2(J.off_pos);
      if (VEL) f.v = f.v + rrot(f.R, kin_perp(P, f.w));
      f.p = f.p + rrot(f.R, P);
      f.R = rmul(f.R, kin_ld2(J.off_quat));
    }
  }
  return f;
}

struct KinCol2 {  // rows (vx, vy, omega)
  d2 v, vd;
  double w;
};
template <bool DOT>
RKH_DI KinCol2 kin_column2(bool prismatic, d2 axis, const KinFrame2& E, const KinFrame2& T) {
  const d2 d = T.p - E.p;
  KinCol2 c;
  c.v = rrotT(prismatic ? rrot(E.R, axis) : kin_perp(d, 1.0), T.R);
  c.w = prismatic ? 0.0 : 1.0;
  c.vd = mk2(0.0, 0.0);
  if (DOT) {
    const double rel_w = T.w - E.w;  // f2.AngVelocity
    const d2 lin = prismatic ? mk2(0.0, 0.0) : rrotT(kin_perp((T.v - E.v) - kin_perp(d, E.w), 1.0), T.R);
    c.vd = lin - kin_perp(c.v, rel_w);
  }
  return c;
}

// ---- the damped least-squares step (rkh_inverse_kinematics, rkh.h) ----------------------------------------------------
// Pose error of frame T against the target (p*, Q*): e[0..2] = (p* - p) R(Q), e[3..5] = 2 vec(Q^-1 Q*), the short way round.
RKH_DI void kin_pose_error(const KinFrame& T, d3 pstar, d4 Qstar, double* e) {
  const d3 ev = mulT(pstar - T.p, rotmat(T.Q));
  d4 dQ = qmul(qinv(T.Q), Qstar);
  if (dQ.w < 0.0) dQ = d4{-dQ.w, -dQ.x, -dQ.y, -dQ.z};
  e[0] = ev.x; e[1] = ev.y; e[2] = ev.z;
  e[3] = 2.0 * dQ.x; e[4] = 2.0 * dQ.y; e[5] = 2.0 * dQ.z;
}

// A y = e for the symmetric 6 x 6 A (lower triangle, row-major packed: A[i (i + 1) / 2 + j], j <= i), in place in e:
// decompose_Cholesky + backsub_Cholesky (lin_alg/mat_cholesky.hpp:60-100, :160-178), the sequence of the f-eval.
// false: a pivot that is not positive (A is then not positive definite to rounding; e is left undefined).  The pivots
// are tested without leaving the sequence: six nested exits would cost a lane-mask register pair each.
RKH_DI bool kin_cholesky6(const double* A, double* e) {
  double L[21];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j < i; ++j) {
      double s = A[i * (i + 1) / 2 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
      L[i * (i + 1) / 2 + j] = s / L[j * (j + 1) / 2 + j];
    }
    double s = A[i * (i + 1) / 2 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i * (i + 1) / 2 + k] * L[i * (i + 1) / 2 + k];
    ok = ok && (s > 0.0);
    L[i * (i + 1) / 2 + i] = sqrt(s);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int k = 0; k < i; ++k) e[i] -= L[i * (i + 1) / 2 + k] * e[k];
    e[i] /= L[i * (i + 1) / 2 + i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
#pragma unroll
    for (int k = 5; k > i; --k) e[i] -= L[k * (k + 1) / 2 + i] * e[k];
    e[i] /= L[i * (i + 1) / 2 + i];
  }
  return ok;
}

RKH_DI double kin_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

}  // namespace rkh
