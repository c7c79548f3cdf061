"""Test-side CPU twin of the kinematics entries (rkh_direct_kinematics[_2d], rkh_jacobians[_2d], rkh_inverse_kinematics).

Built on tests/kte_ref.py: frames and rates are Chain.do_motion's (kte_map_chain::doMotion with q'' = 0), and a Jacobian
column is jacobian_gen_3D::get_jac_relative_to as the reference writes it (core/kinetostatics/motion_jacobians.hpp:238-251):

    f2 = aFrame->getFrameRelativeTo(Parent)        = Parent.inverse().addBefore(aFrame)   (kte_ref.Frame)
    v    = (qd_avel % f2.Position + qd_vel) * R             R = rotmat(f2.Quat)
    w    = qd_avel * R
    vdot = (qd_avel % f2.Velocity + qd_aacc % f2.Position + qd_acc) * R - f2.AngVelocity % v
    wdot = qd_aacc * R - f2.AngVelocity % w

with the generators the joints register (revolute qd_avel = mAxis, prismatic qd_vel = mAxis, the rest 0).  The device
evaluates the same columns in a world form (reak_amd/csrc/kinematics_device.h); this module does NOT, so the two are
independent restatements.  Planar chains (frame_2D, jacobian_gen_2D :138-146) carry their rates here as well, which
tests/kte_ref_planar.py does not.  The upstream set of a frame follows the op program: a joint gives up[end] = up[base] |
bit(coord), a link up[end] = up[base], the base has none.

ik_solve is the damped least-squares iteration include/rkh.h defines, statement by statement, in Python floats (IEEE
double, sums left to right)."""
import math

import numpy as np

import kte_ref as K
import kte_ref_planar as KP
from reak_amd import types as T

JOINTS_3D = (T.KTE_REVOLUTE_JOINT_3D, T.KTE_PRISMATIC_JOINT_3D)
JOINTS_2D = (T.KTE_REVOLUTE_JOINT_2D, T.KTE_PRISMATIC_JOINT_2D)
LINKS = (T.KTE_RIGID_LINK_3D, T.KTE_RIGID_LINK_2D)


def is_planar(scn):
    return any(o.kind in JOINTS_2D for o in scn.ops)


def upstream(scn):
    """{frame: bitmask of upstream joints} over every frame of the program, frame 0 included."""
    up = {0: 0}
    for o in scn.ops:
        if o.kind in JOINTS_3D + JOINTS_2D:
            up[o.end_frame] = up[o.base_frame] | (1 << o.coord)
        elif o.kind in LINKS:
            up[o.end_frame] = up[o.base_frame]
    return up


def all_frames(scn):
    return sorted(upstream(scn))


def reach(scn):
    """|base position| + the link and mount offsets + the travel of the prismatic joints over the scenario's box: a bound
    on the distance of every frame from the world origin, the scale of the position tolerances."""
    r = math.sqrt(sum(v * v for v in list(scn.base.pose.pos)[:3]))
    for o in scn.ops:
        if o.kind in LINKS:
            r += math.sqrt(sum(v * v for v in list(o.offset.pos)[:3]))
        elif o.kind in (T.KTE_PRISMATIC_JOINT_3D, T.KTE_PRISMATIC_JOINT_2D):
            travel = max(abs(scn.dyn.lower[2 * o.coord]), abs(scn.dyn.upper[2 * o.coord]))
            r += travel * math.sqrt(sum(v * v for v in list(o.axis)[:3]))
    return r


# ---- 3D ---------------------------------------------------------------------------------------------------------------
class Kin3:
    def __init__(self, scn):
        self.scn, self.chain, self.n = scn, K.Chain(scn), scn.n_dof
        self.up = upstream(scn)

    def motion(self, q, qd=None):
        """(frames, jac): kte_ref.Frame per frame id after doMotion with q'' = 0, and the joints' generators."""
        n = self.n
        qd = [0.0] * n if qd is None else [float(v) for v in qd]
        return self.chain.do_motion([float(v) for v in q], qd, [0.0] * n)

    def frame_arrays(self, q, qd, frames):
        fr, _ = self.motion(q, qd)
        return {"pos": np.array([fr[f].pos for f in frames]), "rot": np.array([fr[f].Q for f in frames]),
                "vel": np.array([fr[f].vel for f in frames]), "ang_vel": np.array([fr[f].w for f in frames])}

    def column(self, fr, gen, frame, dot=True):
        parent, qd_vel, qd_avel = gen
        f2 = fr[parent].inverse()
        f2.add_before_frame(fr[frame])
        R = K.q_rotmat(f2.Q)
        v = K.vmul(K.add(K.cross(qd_avel, f2.pos), qd_vel), R)
        w = K.vmul(qd_avel, R)
        if not dot:
            return v, w, K.Z3, K.Z3
        vd = K.sub(K.vmul(K.cross(qd_avel, f2.vel), R), K.cross(f2.w, v))
        wd = K.neg(K.cross(f2.w, w))
        return v, w, vd, wd

    def jacobians(self, q, qd, frame, dot=True):
        """(Jac, JacDot) [6][n] of one frame, rows (velocity, angular velocity) in the frame's own coordinates."""
        fr, jac = self.motion(q, qd)
        J, Jd = np.zeros((6, self.n)), np.zeros((6, self.n))
        for i in range(self.n):
            if not (self.up[frame] >> i) & 1:
                continue
            v, w, vd, wd = self.column(fr, jac[i], frame, dot)
            J[:3, i], J[3:, i], Jd[:3, i], Jd[3:, i] = v, w, vd, wd
        return J, Jd


# ---- planar -----------------------------------------------------------------------------------------------------------
class Frame2:
    __slots__ = ("pos", "R", "vel", "w")

    def __init__(self, pos=KP.Z2, R=(1.0, 0.0), vel=KP.Z2, w=0.0):
        self.pos, self.R, self.vel, self.w = pos, R, vel, w


class Kin2:
    def __init__(self, scn):
        self.scn, self.n = scn, scn.n_dof
        self.ops = KP.Chain(scn).ops
        self.base = Frame2((scn.base.pose.pos[0], scn.base.pose.pos[1]), (scn.base.pose.quat[0], scn.base.pose.quat[1]))
        self.n_frames = max(max(o["base"], o["end"]) for o in self.ops) + 1
        self.up = upstream(scn)

    def motion(self, q, qd=None):
        n = self.n
        q = [float(v) for v in q]
        qd = [0.0] * n if qd is None else [float(v) for v in qd]
        fr = [Frame2() for _ in range(self.n_frames)]
        fr[0] = self.base
        jac = [None] * n
        for o in self.ops:
            k = o["kind"]
            if k == T.KTE_REVOLUTE_JOINT_2D:  # revolute_joint.cpp:30-56
                B, c = fr[o["base"]], o["coord"]
                fr[o["end"]] = Frame2(B.pos, KP.rmul(B.R, (math.cos(q[c]), math.sin(q[c]))), B.vel, B.w + qd[c])
                jac[c] = (o["end"], KP.Z2, 1.0)
            elif k == T.KTE_PRISMATIC_JOINT_2D:  # prismatic_joint.cpp:44-62
                B, c, ax = fr[o["base"]], o["coord"], o["axis"]
                tp, tv = KP.smul(q[c], ax), KP.smul(qd[c], ax)
                fr[o["end"]] = Frame2(KP.add(B.pos, KP.rrot(B.R, tp)), B.R,
                                      KP.add(B.vel, KP.rrot(B.R, KP.add(KP.cross_sv(B.w, tp), tv))), B.w)
                jac[c] = (o["end"], ax, 0.0)
            elif k == T.KTE_RIGID_LINK_2D:  # rigid_link.cpp:87-99
                B = fr[o["base"]]
                fr[o["end"]] = Frame2(KP.add(B.pos, KP.rrot(B.R, o["pos"])), KP.rmul(B.R, o["rot"]),
                                      KP.add(B.vel, KP.rrot(B.R, KP.cross_sv(B.w, o["pos"]))), B.w)
        return fr, jac

    def frame_arrays(self, q, qd, frames):
        fr, _ = self.motion(q, qd)
        return {"pos": np.array([fr[f].pos for f in frames]), "rot": np.array([fr[f].R for f in frames]),
                "vel": np.array([fr[f].vel for f in frames]), "ang_vel": np.array([fr[f].w for f in frames])}

    @staticmethod
    def relative(P, A):
        """frame_2D::getFrameRelativeTo: A seen from P (frame_2D.hpp: the inverse of P put before A)."""
        inv_R = (P.R[0], -P.R[1])
        inv_w = -P.w
        inv_pos = KP.rrotT((-P.pos[0], -P.pos[1]), P.R)
        inv_vel = KP.rrotT(KP.smul(-1.0, KP.add(KP.cross_sv(inv_w, P.pos), P.vel)), P.R)
        pos = KP.add(inv_pos, KP.rrot(inv_R, A.pos))
        vel = KP.add(inv_vel, KP.rrot(inv_R, KP.add(KP.cross_sv(inv_w, A.pos), A.vel)))
        return Frame2(pos, KP.rmul(inv_R, A.R), vel, inv_w + A.w)

    def jacobians(self, q, qd, frame, dot=True):
        """(Jac, JacDot) [3][n], rows (vx, vy, omega) in the frame's own coordinates."""
        fr, jac = self.motion(q, qd)
        J, Jd = np.zeros((3, self.n)), np.zeros((3, self.n))
        for i in range(self.n):
            if not (self.up[frame] >> i) & 1:
                continue
            parent, qd_vel, qd_avel = jac[i]
            f2 = self.relative(fr[parent], fr[frame])
            v = KP.rrotT(KP.add(KP.cross_sv(qd_avel, f2.pos), qd_vel), f2.R)
            J[:2, i], J[2, i] = v, qd_avel
            if dot:
                Jd[:2, i] = KP.sub(KP.rrotT(KP.cross_sv(qd_avel, f2.vel), f2.R), KP.cross_sv(f2.w, v))
        return J, Jd


def kin(scn):
    return Kin2(scn) if is_planar(scn) else Kin3(scn)


# ---- the damped least-squares pose iteration of rkh_inverse_kinematics (include/rkh.h) -----------------------------------
def clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def pose_error(frame, pstar, Qstar):
    """(e [6], |e_v|, |e_w|) of a kte_ref.Frame against the target."""
    ev = K.vmul(K.sub(pstar, frame.pos), K.q_rotmat(frame.Q))
    dQ = K.q_mul(K.q_inv(frame.Q), Qstar)
    if dQ[0] < 0.0:
        dQ = (-dQ[0], -dQ[1], -dQ[2], -dQ[3])
    ew = (2.0 * dQ[1], 2.0 * dQ[2], 2.0 * dQ[3])
    return list(ev) + list(ew), K._norm(ev), K._norm(ew)


def cholesky_solve6(A, e):
    """decompose_Cholesky + backsub_Cholesky (kte_ref.Chain.state_derivative's sequence); None on a pivot <= 0."""
    n = 6
    b = list(e)
    L = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i):
            s = A[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
        s = A[i][i]
        for k in range(i):
            s -= L[i][k] * L[i][k]
        if not s > 0.0:
            return None
        L[i][i] = math.sqrt(s)
    for i in range(n):
        for k in range(i):
            b[i] -= L[i][k] * b[k]
        b[i] /= L[i][i]
    for i in range(n - 1, -1, -1):
        for k in range(n - 1, i, -1):
            b[i] -= L[k][i] * b[k]
        b[i] /= L[i][i]
    return b


def ik_solve(kin3, frame, target, seed, lower, upper, params):
    """One solve: dict q [n], res_pos, res_rot, iters, converged."""
    n = kin3.n
    pstar, Qstar = tuple(target.pos), tuple(target.quat)
    q = [clamp(float(seed[j]), lower[j], upper[j]) for j in range(n)]
    d2 = params.damping * params.damping
    k, conv = 0, False
    while True:
        fr, jac = kin3.motion(q)
        e, rp, rr = pose_error(fr[frame], pstar, Qstar)
        if rp <= params.tol_pos and rr <= params.tol_rot:
            conv = True
            break
        if k == params.max_iters:
            break
        cols = [None] * n
        for i in range(n):
            if (kin3.up[frame] >> i) & 1:
                v, w, _, _ = kin3.column(fr, jac[i], frame, dot=False)
                cols[i] = list(v) + list(w)
        A = [[0.0] * 6 for _ in range(6)]
        for r in range(6):
            for c in range(r + 1):
                s = 0.0
                for i in range(n):
                    if cols[i] is not None:
                        s = s + cols[i][r] * cols[i][c]
                A[r][c] = A[c][r] = s
            A[r][r] = A[r][r] + d2
        y = cholesky_solve6(A, e)
        if y is None:
            break
        dq = [0.0] * n
        for i in range(n):
            if cols[i] is not None:
                s = 0.0
                for r in range(6):
                    s = s + cols[i][r] * y[r]
                dq[i] = s
        mx = max(abs(v) for v in dq)
        if mx > params.max_step:
            sc = params.max_step / mx
            dq = [v * sc for v in dq]
        q = [clamp(q[j] + dq[j], lower[j], upper[j]) for j in range(n)]
        k += 1
    return {"q": np.array(q), "res_pos": rp, "res_rot": rr, "iters": k, "converged": conv}


def fk_pose(kin3, frame, q):
    """T.Pose of `frame` at q (the target of a configuration)."""
    fr, _ = kin3.motion(q)
    return T.make_pose(fr[frame].pos, fr[frame].Q)
