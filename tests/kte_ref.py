"""Test-side CPU restatement of the KTE chain passes for 3D serial chains of revolute AND prismatic groups.

The oracle's KteChain (oracle/reak_kte.hpp) does not know prismatic_joint_3D: its doMotion / doForce fall through
`default: break`, so a prismatic scene handed to it gives wrong numbers without an error.  This module restates, in plain
Python floats (IEEE double, the oracle's operation order), what the tests need on such scenes:

  kte_map_chain::doMotion / clearForce / doForce    oracle/reak_kte.hpp (revolute_joint_3D, rigid_link_3D, inertia_gen,
                                                    inertia_3D, driving_actuator_gen) + prismatic_joint_3D from
                                                    ctrl/mbd_kte/prismatic_joint.cpp:116-222 of the reference
  mass_matrix_calc::getMassMatrix                   reak_kte.hpp getMassMatrix (get_jac_relative_to, Mcm * Tcm, symmetrise)
  kte_nl_system::get_state_derivative               Cholesky solve, pivot < 1e-8 -> Singular
  steer_position_toward (RK4 + is_free)             oracle/reak_planning.hpp DynSpace (orc_steer)
  interp_topo_move_position_toward_pred             oracle/reak_planning.hpp QuasiStaticSpace (orc_qs_move)

Distances: the shapes are posed here (pose_3D::getGlobalPose) and every (robot, environment) pair with a finder goes
through the oracle's closed form (orc_pair_distance); the minimum over those pairs is findMinimumDistance for bounded
shapes.  Revolute-only chains are pinned against the oracle itself (test_prismatic_cpu.py)."""
import math

import numpy as np

from reak_amd import types as T


class Singular(Exception):
    """singularity_error: a Cholesky pivot below 1e-8."""


# ---- vect<double,3>, rot_mat_3D, quaternion, axis_angle (oracle/reak_math.hpp) ------------------------------------
def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def neg(a):
    return (-a[0], -a[1], -a[2])


def smul(s, a):
    return (a[0] * s, a[1] * s, a[2] * s)


def dot(a, b):
    r = 0.0
    for i in range(3):
        r += a[i] * b[i]
    return r


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def rmul(R, v):  # rot_mat * vect; R = row-major 3x3 tuple of rows
    return (R[0][0] * v[0] + R[0][1] * v[1] + R[0][2] * v[2],
            R[1][0] * v[0] + R[1][1] * v[1] + R[1][2] * v[2],
            R[2][0] * v[0] + R[2][1] * v[1] + R[2][2] * v[2])


def vmul(v, R):  # vect * rot_mat
    return (R[0][0] * v[0] + R[1][0] * v[1] + R[2][0] * v[2],
            R[0][1] * v[0] + R[1][1] * v[1] + R[2][1] * v[2],
            R[0][2] * v[0] + R[1][2] * v[1] + R[2][2] * v[2])


def q_rotmat(q):
    t01, t02, t03 = 2.0 * q[0] * q[1], 2.0 * q[0] * q[2], 2.0 * q[0] * q[3]
    t11, t12, t13 = 2.0 * q[1] * q[1], 2.0 * q[1] * q[2], 2.0 * q[1] * q[3]
    t22, t23, t33 = 2.0 * q[2] * q[2], 2.0 * q[2] * q[3], 2.0 * q[3] * q[3]
    return ((1.0 - t22 - t33, t12 - t03, t02 + t13), (t12 + t03, 1.0 - t11 - t33, t23 - t01),
            (t13 - t02, t01 + t23, 1.0 - t11 - t22))


def q_mul(a, b):
    return (b[0] * a[0] - b[1] * a[1] - b[2] * a[2] - b[3] * a[3],
            b[0] * a[1] + b[3] * a[2] - b[2] * a[3] + b[1] * a[0],
            b[0] * a[2] - b[3] * a[1] + b[1] * a[3] + b[2] * a[0],
            b[0] * a[3] + b[2] * a[1] - b[1] * a[2] + b[3] * a[0])


def q_rot(Q, V):
    t0, t1, t2 = Q[0] * Q[1], Q[0] * Q[2], Q[0] * Q[3]
    t3, t4, t5 = -Q[1] * Q[1], Q[1] * Q[2], Q[1] * Q[3]
    t6, t7, t8 = -Q[2] * Q[2], Q[2] * Q[3], -Q[3] * Q[3]
    return (2.0 * ((t6 + t8) * V[0] + (t4 - t2) * V[1] + (t1 + t5) * V[2]) + V[0],
            2.0 * ((t2 + t4) * V[0] + (t3 + t8) * V[1] + (t7 - t0) * V[2]) + V[1],
            2.0 * ((t5 - t1) * V[0] + (t0 + t7) * V[1] + (t3 + t6) * V[2]) + V[2])


def q_inv(Q):
    return (Q[0], -Q[1], -Q[2], -Q[3])


def _norm(v):
    s = 0.0
    for x in v:
        s += x * x
    return math.sqrt(s)


def axis_angle(angle, axis):
    tmp = _norm(axis)
    ax = (axis[0] / tmp, axis[1] / tmp, axis[2] / tmp) if tmp > 0.0000001 else (1.0, 0.0, 0.0)
    return angle, ax


def aa_quat(angle, ax):
    if _norm(ax) == 0.0:
        return (1.0, 0.0, 0.0, 0.0)
    t = math.sin(0.5 * angle)
    return (math.cos(0.5 * angle), ax[0] * t, ax[1] * t, ax[2] * t)


def aa_rotmat(angle, ax):
    ca = math.cos(angle)
    omc = 1.0 - ca
    t11, t22, t33 = ca + omc * ax[0] * ax[0], ca + omc * ax[1] * ax[1], ca + omc * ax[2] * ax[2]
    t12, t13, t23 = omc * ax[0] * ax[1], omc * ax[0] * ax[2], omc * ax[1] * ax[2]
    sa = math.sin(angle)
    t01, t02, t03 = sa * ax[0], sa * ax[1], sa * ax[2]
    return ((t11, t12 - t03, t13 + t02), (t12 + t03, t22, t23 - t01), (t13 - t02, t23 + t01, t33))


Z3 = (0.0, 0.0, 0.0)


class Frame:
    __slots__ = ("pos", "Q", "vel", "w", "acc", "alpha", "F", "Tq")

    def __init__(self):
        self.pos, self.Q = Z3, (1.0, 0.0, 0.0, 0.0)
        self.vel = self.w = self.acc = self.alpha = self.F = self.Tq = Z3

    def copy(self):
        f = Frame()
        for k in Frame.__slots__:
            setattr(f, k, getattr(self, k))
        return f

    def add_before_pose(self, P, PQ):  # frame_3D::addBefore(pose)
        R = q_rotmat(self.Q)
        self.pos = add(self.pos, rmul(R, P))
        self.vel = add(self.vel, rmul(R, cross(self.w, P)))
        self.acc = add(self.acc, rmul(R, add(cross(self.w, cross(self.w, P)), cross(self.alpha, P))))
        R2 = q_rotmat(PQ)
        self.Q = q_mul(self.Q, PQ)
        self.alpha = vmul(self.alpha, R2)
        self.w = vmul(self.w, R2)

    def add_before_frame(self, o):  # frame_3D::addBefore(frame), pose and rates (get_jac_relative_to reads these)
        R = q_rotmat(self.Q)
        self.pos = add(self.pos, rmul(R, o.pos))
        self.vel = add(self.vel, rmul(R, add(cross(self.w, o.pos), o.vel)))
        self.acc = add(self.acc, rmul(R, add(add(add(cross(self.w, cross(self.w, o.pos)), cross(smul(2.0, self.w), o.vel)),
                                                 cross(self.alpha, o.pos)), o.acc)))
        R2 = q_rotmat(o.Q)
        self.Q = q_mul(self.Q, o.Q)
        self.alpha = add(add(vmul(self.alpha, R2), cross(vmul(self.w, R2), o.w)), o.alpha)
        self.w = add(vmul(self.w, R2), o.w)

    def inverse(self):
        R = q_rotmat(self.Q)
        r = Frame()
        r.Q = q_inv(self.Q)
        r.w = rmul(R, neg(self.w))
        r.alpha = rmul(R, neg(self.alpha))
        r.pos = vmul(neg(self.pos), R)
        r.vel = vmul(neg(add(cross(r.w, self.pos), self.vel)), R)
        r.acc = vmul(neg(add(add(add(cross(r.w, cross(r.w, self.pos)), cross(smul(2.0, r.w), self.vel)),
                                 cross(r.alpha, self.pos)), self.acc)), R)
        return r


def _sym_mul(t, V):  # mat<symmetric> * vect (reak_kte.hpp sym_mul)
    a11, a12, a13, a22, a23, a33 = t
    r = [0.0, 0.0, 0.0]
    r[0] += a11 * V[0]
    r[1] += a12 * V[0]
    r[0] += a12 * V[1]
    r[1] += a22 * V[1]
    r[2] += a13 * V[0]
    r[0] += a13 * V[2]
    r[2] += a23 * V[1]
    r[1] += a23 * V[2]
    r[2] += a33 * V[2]
    return tuple(r)


class Chain:
    """kte_map_chain of a scenario's ops (serial 3D chains of revolute / prismatic groups, optional mount links)."""

    JOINTS = (T.KTE_REVOLUTE_JOINT_3D, T.KTE_PRISMATIC_JOINT_3D)

    def __init__(self, scn):
        self.ops = [dict(kind=o.kind, coord=o.coord, base=o.base_frame, end=o.end_frame, joint_op=o.joint_op,
                         upstream=o.upstream, axis=tuple(o.axis), pos=tuple(o.offset.pos), quat=tuple(o.offset.quat),
                         mass=o.mass, inertia=tuple(o.inertia)) for o in scn.ops]
        for o in self.ops:
            assert o["kind"] in (T.KTE_DRIVING_ACTUATOR_GEN, T.KTE_INERTIA_GEN, T.KTE_RIGID_LINK_3D, T.KTE_INERTIA_3D) + \
                self.JOINTS, "kte_ref: 3D serial chains of revolute / prismatic groups only"
        self.n = max(o["coord"] for o in self.ops) + 1
        self.n_frames = max(max(o["base"], o["end"]) for o in self.ops) + 1
        self.base = Frame()
        self.base.pos = tuple(scn.base.pose.pos)
        self.base.Q = tuple(scn.base.pose.quat)
        self.base.acc = tuple(scn.base.acceleration)
        self.gen = [o for o in self.ops if o["kind"] == T.KTE_INERTIA_GEN]
        self.in3 = [o for o in self.ops if o["kind"] == T.KTE_INERTIA_3D]
        self.shapes = list(scn.shapes)

    # kte_map_chain::doMotion
    def do_motion(self, q, qd, qdd):
        fr = [Frame() for _ in range(self.n_frames)]
        fr[0] = self.base.copy()
        jac = [None] * self.n
        for o in self.ops:
            k = o["kind"]
            if k == T.KTE_REVOLUTE_JOINT_3D:  # revolute_joint.cpp:121-148
                B, E, c, ax = fr[o["base"]], fr[o["end"]], o["coord"], o["axis"]
                E.pos, E.vel, E.acc = B.pos, B.vel, B.acc
                tq = aa_quat(*axis_angle(q[c], ax))
                R2 = q_rotmat(tq)
                E.Q = q_mul(B.Q, tq)
                E.w = add(vmul(B.w, R2), smul(qd[c], ax))
                E.alpha = add(add(vmul(B.alpha, R2), cross(vmul(B.w, R2), smul(qd[c], ax))), smul(qdd[c], ax))
                jac[c] = (o["end"], Z3, ax)
            elif k == T.KTE_PRISMATIC_JOINT_3D:  # prismatic_joint.cpp:116-148
                B, E, c, ax = fr[o["base"]], fr[o["end"]], o["coord"], o["axis"]
                R = q_rotmat(B.Q)
                tmp_pos = smul(q[c], ax)
                tmp_vel = smul(qd[c], ax)
                E.pos = add(B.pos, rmul(R, tmp_pos))
                E.vel = add(B.vel, rmul(R, add(cross(B.w, tmp_pos), tmp_vel)))
                E.acc = add(B.acc, rmul(R, add(add(add(cross(B.w, cross(B.w, tmp_pos)), smul(2.0, cross(B.w, tmp_vel))),
                                                   cross(B.alpha, tmp_pos)), smul(qdd[c], ax))))
                E.Q, E.w, E.alpha = B.Q, B.w, B.alpha
                jac[c] = (o["end"], ax, Z3)
            elif k == T.KTE_RIGID_LINK_3D:  # rigid_link.cpp:152-156
                tmp = fr[o["base"]].copy()
                tmp.add_before_pose(o["pos"], o["quat"])
                E = fr[o["end"]]
                tmp.F, tmp.Tq = E.F, E.Tq
                fr[o["end"]] = tmp
        return fr, jac

    # kte_map_chain::clearForce + doForce (reverse op order)
    def do_force(self, fr, q, qdd, u):
        for o in self.ops:
            for k in ("base", "end"):
                if o[k] >= 0:
                    fr[o[k]].F, fr[o[k]].Tq = Z3, Z3
        f = [0.0] * self.n
        for o in reversed(self.ops):
            k = o["kind"]
            if k == T.KTE_DRIVING_ACTUATOR_GEN:  # driving_actuator.cpp:31-39 + the joint's applyReactionForce
                c = o["coord"]
                f[c] += u[c]
                j = self.ops[o["joint_op"]]
                B = fr[j["base"]]
                if j["kind"] == T.KTE_PRISMATIC_JOINT_3D:  # prismatic_joint.cpp:219-222
                    B.F = sub(B.F, smul(u[c], j["axis"]))
                else:  # revolute_joint.cpp:210-213
                    B.Tq = sub(B.Tq, smul(u[c], j["axis"]))
            elif k == T.KTE_INERTIA_GEN:
                f[o["coord"]] -= qdd[o["coord"]] * o["mass"]
            elif k == T.KTE_REVOLUTE_JOINT_3D:  # revolute_joint.cpp:170-181
                B, E, c, ax = fr[o["base"]], fr[o["end"]], o["coord"], o["axis"]
                R = aa_rotmat(*axis_angle(q[c], ax))
                B.F = add(B.F, rmul(R, E.F))
                f[c] += dot(E.Tq, ax)
                B.Tq = add(B.Tq, rmul(R, sub(E.Tq, smul(dot(E.Tq, ax), ax))))
            elif k == T.KTE_PRISMATIC_JOINT_3D:  # prismatic_joint.cpp:150-170
                B, E, c, ax = fr[o["base"]], fr[o["end"]], o["coord"], o["axis"]
                tmp_f = dot(E.F, ax)
                f[c] += tmp_f
                B.F = add(B.F, sub(E.F, smul(tmp_f, ax)))
                B.Tq = add(B.Tq, add(E.Tq, cross(smul(q[c], ax), E.F)))
            elif k == T.KTE_RIGID_LINK_3D:  # rigid_link.cpp:170-178
                B, E = fr[o["base"]], fr[o["end"]]
                R = q_rotmat(o["quat"])
                tf = rmul(R, E.F)
                B.F = add(B.F, tf)
                B.Tq = add(B.Tq, add(rmul(R, E.Tq), cross(o["pos"], tf)))
            elif k == T.KTE_INERTIA_3D:  # inertia.cpp:111-122
                Fr = fr[o["end"]]
                g = Fr.copy()
                Fr.F = sub(Fr.F, smul(o["mass"], q_rot(q_inv(g.Q), g.acc)))
                Fr.Tq = sub(Fr.Tq, add(_sym_mul(o["inertia"], g.alpha), cross(g.w, _sym_mul(o["inertia"], g.w))))
        return f

    def _jac_rel(self, fr, J, a_frame):  # jacobian_gen_3D::get_jac_relative_to, velocity part
        parent, qd_vel, qd_avel = J
        f2 = fr[parent].inverse()
        f2.add_before_frame(fr[a_frame])
        R = q_rotmat(f2.Q)
        return vmul(add(cross(qd_avel, f2.pos), qd_vel), R), vmul(qd_avel, R)

    def mass_matrix(self, fr, jac):  # mass_matrix_calc::getMassMatrix (reak_kte.hpp)
        n = self.n
        m = len(self.gen) + 6 * len(self.in3)
        Tcm = [[0.0] * n for _ in range(m)]
        Mcm = [[0.0] * m for _ in range(m)]
        for i in range(n):
            row = 0
            for o in self.gen:
                if o["upstream"] & (1 << i):
                    Tcm[row][i] = 1.0
                row += 1
            for o in self.in3:
                if o["upstream"] & (1 << i):
                    v, w = self._jac_rel(fr, jac[i], o["end"])
                    for k in range(3):
                        Tcm[row + k][i] = v[k]
                        Tcm[row + 3 + k][i] = w[k]
                row += 6
        row = 0
        blocks = []
        for o in self.gen:
            Mcm[row][row] = o["mass"]
            blocks.append((row, 1))
            row += 1
        for o in self.in3:
            for k in range(3):
                Mcm[row + k][row + k] = o["mass"]
            t = o["inertia"]
            I = ((t[0], t[1], t[2]), (t[1], t[3], t[4]), (t[2], t[4], t[5]))
            for a in range(3):
                for b in range(3):
                    Mcm[row + 3 + a][row + 3 + b] = I[a][b]
            blocks += [(row, 1), (row + 1, 1), (row + 2, 1), (row + 3, 3)]
            row += 6
        # P = Mcm * Tcm (mat_alg_symmetric.hpp:551-566); Mcm is block diagonal, the terms skipped are exact zeros
        P = [[0.0] * n for _ in range(m)]
        blk = [0] * m
        for start, size in blocks:
            for r in range(start, start + size):
                blk[r] = start
        for i in range(m):
            for l in range(n):
                for j in range(blk[i], i):
                    P[j][l] += Mcm[i][j] * Tcm[i][l]
                    P[i][l] += Mcm[i][j] * Tcm[j][l]
                P[i][l] += Mcm[i][i] * Tcm[i][l]
        Mf = [[0.0] * n for _ in range(n)]
        for i in range(n):
            for jj in range(n):
                s = 0.0
                for j in range(m):
                    s += Tcm[j][i] * P[j][jj]
                Mf[i][jj] = s
        M = [[0.0] * n for _ in range(n)]
        for i in range(n):
            for j in range(i):
                v = 0.5 * (Mf[j][i] + Mf[i][j])
                M[i][j] = M[j][i] = v
            M[i][i] = Mf[i][i]
        return M

    def state_derivative(self, x, u):
        """(pd, M, f) of kte_nl_system::get_state_derivative; raises Singular like the reference."""
        n = self.n
        q, qd, qdd = [float(x[2 * j]) for j in range(n)], [float(x[2 * j + 1]) for j in range(n)], [0.0] * n
        u = [float(v) for v in u]
        fr, jac = self.do_motion(q, qd, qdd)
        f = self.do_force(fr, q, qdd, u)
        M = self.mass_matrix(fr, jac)
        b = list(f)
        L = [[0.0] * n for _ in range(n)]  # decompose_Cholesky + backsub_Cholesky (reak_math.hpp)
        for i in range(n):
            for j in range(i):
                L[i][j] = M[i][j]
                for k in range(j):
                    L[i][j] -= L[i][k] * L[j][k]
                L[i][j] /= L[j][j]
            L[i][i] = M[i][i]
            for k in range(i):
                L[i][i] -= L[i][k] * L[i][k]
            if L[i][i] < 1e-8:
                raise Singular()
            L[i][i] = math.sqrt(L[i][i])
        for i in range(n):
            for k in range(i):
                b[i] -= L[i][k] * b[k]
            b[i] /= L[i][i]
        for i in range(n - 1, -1, -1):
            for k in range(n - 1, i, -1):
                b[i] -= L[k][i] * b[k]
            b[i] /= L[i][i]
        pd = np.zeros(2 * n)
        pd[0::2] = qd
        pd[1::2] = b
        return pd, np.array(M), np.array(f)

    def frames(self, x):
        """[n_frames][7] = position, quaternion of every frame after doMotion (apply_kinematics)."""
        n = self.n
        fr, _ = self.do_motion([float(x[2 * j]) for j in range(n)], [float(x[2 * j + 1]) for j in range(n)], [0.0] * n)
        return np.array([list(f.pos) + list(f.Q) for f in fr])

    def posed_shapes(self, x):
        """(robot shapes, environment shapes) as world-anchored rkh_shape copies (pose_3D::getGlobalPose)."""
        fr = self.frames(x)
        robot, env = [], []
        for s in self.shapes:
            c = T.Shape(kind=s.kind, anchor=-1)
            c.dims[:] = list(s.dims)
            if s.anchor >= 0:
                P, Q = tuple(fr[s.anchor][:3]), tuple(fr[s.anchor][3:])
                c.pose = T.make_pose(add(P, q_rot(Q, tuple(s.pose.pos))), q_mul(Q, tuple(s.pose.quat)))
                robot.append(c)
            else:
                c.pose = s.pose
                env.append(c)
        return robot, env


def _brad(s):
    if s.kind == T.SHAPE_SPHERE:
        return s.dims[0]
    if s.kind == T.SHAPE_BOX:
        return 0.5 * math.sqrt(s.dims[0] ** 2 + s.dims[1] ** 2 + s.dims[2] ** 2)
    if s.kind == T.SHAPE_CCYLINDER:
        return 0.5 * s.dims[0] + s.dims[1]
    if s.kind == T.SHAPE_CYLINDER:
        return math.hypot(0.5 * s.dims[0], s.dims[1])
    return math.inf


class Distances:
    """Minimum proxy-pair distance of a configuration: shapes posed by Chain, pairs through orc_pair_distance."""

    def __init__(self, chain, oracle_lib):
        self.chain, self.lib = chain, oracle_lib.load()

    def pair_distances(self, x):
        import ctypes as C

        robot, env = self.chain.posed_shapes(x)
        out = []
        for r in robot:
            for e in env:
                d = self.lib.orc_pair_distance(C.byref(r), C.byref(e))
                if not math.isnan(d):  # no finder for this pair of kinds
                    out.append((d, r, e))
        return out

    def min_distance(self, x):
        ds = [d for d, _, _ in self.pair_distances(x)]
        return min(ds) if ds else math.inf

    def is_free(self, x):
        """manip_dk_proxy_env_impl::is_free's proximity half: no pair closer than 0 (pairs whose bounding spheres are
        apart cannot be, and are skipped)."""
        import ctypes as C

        robot, env = self.chain.posed_shapes(x)
        for r in robot:
            for e in env:
                gap = np.linalg.norm(np.array(r.pose.pos) - np.array(e.pose.pos)) - _brad(r) - _brad(e)
                if gap > 1e-9:
                    continue
                d = self.lib.orc_pair_distance(C.byref(r), C.byref(e))
                if not math.isnan(d) and d < 0.0:
                    return False
        return True


def in_bounds(a, lower, upper):  # hyperbox_is_in_bounds
    for i in range(len(a)):
        if lower[i] < upper[i]:
            if a[i] < lower[i] or a[i] > upper[i]:
                return False
        elif a[i] > lower[i] or a[i] < upper[i]:
            return False
    return True


def euclid(a, b):
    s = 0.0
    for i in range(len(a)):
        d = a[i] - b[i]
        s += d * d
    return math.sqrt(s)


def steer(chain, dist, dyn, a, b, fraction=1.0):
    """DynSpace::steer_position_toward (orc_steer): (last free state, accepted steps, record, min distance of every
    tested state).  RK4 = runge_kutta4_integrate with one step per call."""
    D, n = 2 * chain.n, chain.n
    lower, upper = [dyn.lower[i] for i in range(D)], [dyn.upper[i] for i in range(D)]
    T_goal = fraction * (dyn.steps_per_edge * dyn.dt)
    t_cur = 0.0
    x = [float(v) for v in a]
    b = [float(v) for v in b]
    rec, dmins = [list(x)], []
    n_free = 0
    f = lambda p, uu: list(chain.state_derivative(p, uu)[0])
    while t_cur < T_goal and euclid(x, b) > dyn.goal_tol:
        u = []
        for i in range(n):
            v = dyn.kp * (b[2 * i] - x[2 * i]) + dyn.kd * (b[2 * i + 1] - x[2 * i + 1])
            u.append(dyn.u_max if v > dyn.u_max else (-dyn.u_max if v < -dyn.u_max else v))
        h, t, t_end = dyn.dt, t_cur, t_cur + dyn.dt
        dp = f(x, u)
        e = list(x)
        while t < t_end:
            w = list(e)
            k1 = [h * v for v in dp]
            e = [e[i] + 0.5 * k1[i] for i in range(D)]
            t += h * 0.5
            dp = f(e, u)
            k2 = [h * v for v in dp]
            e = [w[i] + 0.5 * k2[i] for i in range(D)]
            dp = f(e, u)
            k3 = [h * v for v in dp]
            e = [w[i] + k3[i] for i in range(D)]
            t += h * 0.5
            dp = f(e, u)
            e = [e[i] + ((((1.0 / 6.0) * k1[i] + (2.0 / 6.0) * k2[i]) + (h / 6.0) * dp[i]) - (2.0 / 3.0) * k3[i])
                 for i in range(D)]
            if t < t_end:
                dp = f(e, u)
        if not in_bounds(e, lower, upper):
            break
        dm = dist.min_distance(e)
        dmins.append(dm)
        if dm < 0.0:
            break
        x = e
        t_cur += dyn.dt
        n_free += 1
        rec.append(list(x))
    return np.array(x), n_free, np.array(rec), dmins


def qs_move(chain, dist, lower, upper, min_interval, a, b, fraction=1.0):
    """QuasiStaticSpace::move_position_toward (orc_qs_move): (result, is_free calls)."""
    n = chain.n
    a, b = [float(v) for v in a], [float(v) for v in b]
    lin = lambda fr: [a[i] + (b[i] - a[i]) * fr for i in range(n)]
    checked = 0

    def is_free(p):
        nonlocal checked
        checked += 1
        if not in_bounds(p, lower, upper):
            return False
        x = np.zeros(2 * n)
        x[0::2] = p
        return dist.is_free(x)

    dist_tot = euclid(a, b)
    if dist_tot == math.inf:
        return np.array(a), checked
    if dist_tot < min_interval:
        return np.array(lin(fraction)), checked
    dist_inter = dist_tot * fraction
    dist_cur = min_interval
    last = a
    while dist_cur < dist_inter:
        r = lin(dist_cur / dist_tot)
        if not is_free(r):
            return np.array(last), checked
        dist_cur += min_interval
        last = r
    if fraction == 1.0:
        return np.array(b), checked
    if fraction == 0.0:
        return np.array(a), checked
    return np.array(lin(fraction)), checked
