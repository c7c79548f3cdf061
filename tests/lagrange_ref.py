"""Energy-based reference for the f-eval  q'' = M(q)^-1 f(q, q', u)  of a serial chain -- and NO force propagation.

Every other statement of the f-eval in this repository (oracle/reak_kte.hpp, tests/kte_ref.py, tests/kte_ref_planar.py, the
device headers) follows the reference's doMotion / clearForce / doForce passes term by term, so a term transcribed
wrongly once is wrong in all of them.  This module shares no code with them and imports none of them.  It knows only

  * forward kinematics of the ops: the base pose, a rotation by Rodrigues' formula about a revolute joint's (unit) axis,
    the link offsets, and a prismatic end frame at  base + R (q a)  with the axis `a` as given (not normalised);
  * the kinetic energy  T = 1/2 sum_bodies (m |v_cm|^2 + w . I w) + 1/2 sum_rotors j q'^2 : every inertia_3D /
    inertia_2D is a body whose centre of mass is its frame's origin, tensor (a11, a12, a13, a22, a23, a33) in that frame;
  * the potential  V = sum m (a_base . p_cm) : gravity enters as the base's acceleration, in world coordinates;

all in mpmath at 50 decimal digits; results are rounded to the nearest double only at the very end.

M(q) comes from geometric Jacobians of that FK; `evaluate` cross-checks it against the second differences of T(q, q') in
q', where T is computed by propagating velocities frame to frame (T is quadratic in q', so the differences are exact).
c_i = sum_jk (dM_ij/dq_k - 1/2 dM_jk/dq_i) q'_j q'_k  and  dV/dq  come from central differences with step 1e-20: the
truncation error is ~h^2 = 1e-40 and the rounding error ~1e-50 / h = 1e-30 relative, so the derivatives are good to about
1e-30; `evaluate` repeats them at half the step and asserts that they agree to 1e-27.

THE JOINT RULE.  The reference's field is not the Lagrangian one.  revolute_joint_3D::doForce hands its base frame
`Torque - (Torque . axis) axis`, prismatic_joint_3D::doForce does the same with the force, a revolute_joint_2D hands no
torque on at all, and driving_actuator_gen's reaction removes the drive the same way: the component that a joint's
coordinate takes is not transmitted upstream.  Joint k therefore withholds the wrench f_k a_k (a couple for a revolute
joint, a force through the joint's base origin p_k for a prismatic one) from every joint i < k, so

    G(q) f_reference = u - c(q, q') - dV/dq ,     q'' = M^-1 f_reference ,

with G unit upper triangular and, for i < k (world coordinates, a = axis as stored, p = origin of the joint's base frame):

    i revolute,  k revolute :  a_i . a_k              i prismatic, k revolute :  0
    i revolute,  k prismatic:  (a_i x (p_k - p_i)) . a_k     i prismatic, k prismatic:  a_i . a_k

Planar chains are the same mechanism in the z = 0 plane: every revolute axis is +z, a prismatic axis is (a_x, a_y, 0), the
2D cross product is the z component of the 3D one, the tensor is (0, ..., 0, I).

Out of scope: flexible_beam_3D (refused), shapes, the steer control law.

Also here: the seeded case families shared by tests/make_lagrange_golden.py and tests/test_lagrange_feval_{cpu,gpu}.py."""
import math
from dataclasses import dataclass

import mpmath
import numpy as np

import planar_prismatic_scenes as pps
from reak_amd import scenarios
from reak_amd import types as T

MP = mpmath.mp.clone()
MP.dps = 50
mpf = MP.mpf
STEP = mpf(10) ** -20          # central-difference step
DERIV_AGREE = mpf(10) ** -27   # derivatives at STEP and STEP / 2 agree to this (relative to the largest entry)
MASS_AGREE = mpf(10) ** -40    # Jacobian mass matrix against the second differences of T
KAPPA_MAX = 1e6

_REV = (T.KTE_REVOLUTE_JOINT_3D, T.KTE_REVOLUTE_JOINT_2D)
_PRI = (T.KTE_PRISMATIC_JOINT_3D, T.KTE_PRISMATIC_JOINT_2D)
_LINK = (T.KTE_RIGID_LINK_3D, T.KTE_RIGID_LINK_2D)
_BODY = (T.KTE_INERTIA_3D, T.KTE_INERTIA_2D)
_PLANAR = (T.KTE_REVOLUTE_JOINT_2D, T.KTE_PRISMATIC_JOINT_2D, T.KTE_RIGID_LINK_2D, T.KTE_INERTIA_2D)
_ZERO = mpf(0)
_ONE = mpf(1)


# ---- 3-vectors and 3x3 matrices as lists of mpf -----------------------------------------------------------------------
def _vec(v):
    return [mpf(float(x)) for x in v]


def _add(a, b):
    return [a[0] + b[0], a[1] + b[1], a[2] + b[2]]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _scale(s, a):
    return [s * a[0], s * a[1], s * a[2]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _mv(R, v):
    return [_dot(R[0], v), _dot(R[1], v), _dot(R[2], v)]


def _mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _mt(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def _quat_matrix(q):
    w, x, y, z = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def _planar_matrix(c, s):
    return [[c, -s, _ZERO], [s, c, _ZERO], [_ZERO, _ZERO, _ONE]]


def _rodrigues(a, angle):
    """R = I + sin(angle) K + (1 - cos(angle)) K^2, K the cross-product matrix of the unit axis a."""
    s, c = MP.sin(angle), MP.cos(angle)
    K = [[_ZERO, -a[2], a[1]], [a[2], _ZERO, -a[0]], [-a[1], a[0], _ZERO]]
    K2 = _mm(K, K)
    return [[(_ONE if i == j else _ZERO) + s * K[i][j] + (1 - c) * K2[i][j] for j in range(3)] for i in range(3)]


@dataclass
class Result:
    """Doubles (nearest to the mpmath values): M [n][n], c, dVdq, f, qdd, f_lagrange [n], G [n][n], kappa."""
    M: np.ndarray
    c: np.ndarray
    dVdq: np.ndarray
    G: np.ndarray
    f: np.ndarray
    qdd: np.ndarray
    kappa: float
    f_lagrange: np.ndarray   # u - c - dV/dq: what f would be WITHOUT the joint rule


class Model:
    """A scenarios.Scenario's chain as the energy reference sees it."""

    def __init__(self, scn, joint_rule=True):
        self.joint_rule = joint_rule   # False: G = identity (the tests show that this does NOT describe the f-eval)
        kinds = [o.kind for o in scn.ops]
        assert T.KTE_FLEXIBLE_BEAM_3D not in kinds, "lagrange_ref: flexible_beam_3D is out of scope"
        self.planar = any(k in _PLANAR for k in kinds)
        self.n = max(o.coord for o in scn.ops) + 1
        pose = scn.base.pose
        self.base_pos = self._pos(pose)
        self.base_R = self._rot(pose)
        acc = scn.base.acceleration
        self.base_acc = _vec([acc[0], acc[1], 0.0 if self.planar else acc[2]])
        self.steps = []      # FK steps in op order: (what, base, end, coord, vector, matrix)
        self.bodies = []     # (frame, mass, tensor in the frame, declared upstream mask)
        self.rotors = [_ZERO] * self.n
        self.kind = [None] * self.n      # "R" / "P"
        self.joint_base = [None] * self.n
        self.parent = {0: (None, None)}  # frame -> (parent frame, joint coordinate or None)
        for o in scn.ops:
            k = o.kind
            if k in _REV:
                a = _vec([0.0, 0.0, 1.0]) if self.planar else _vec(o.axis)
                assert abs(_dot(a, a) - 1) < mpf(10) ** -12, "lagrange_ref: a revolute axis must be unit"
                self.steps.append(("R", o.base_frame, o.end_frame, o.coord, a, None))
                self.kind[o.coord], self.joint_base[o.coord] = "R", o.base_frame
                self.parent[o.end_frame] = (o.base_frame, o.coord)
            elif k in _PRI:
                a = _vec([o.axis[0], o.axis[1], 0.0 if self.planar else o.axis[2]])
                self.steps.append(("P", o.base_frame, o.end_frame, o.coord, a, None))
                self.kind[o.coord], self.joint_base[o.coord] = "P", o.base_frame
                self.parent[o.end_frame] = (o.base_frame, o.coord)
            elif k in _LINK:
                self.steps.append(("L", o.base_frame, o.end_frame, -1, self._pos(o.offset), self._rot(o.offset)))
                self.parent[o.end_frame] = (o.base_frame, None)
            elif k in _BODY:
                t = [mpf(float(v)) for v in o.inertia]
                I = [[_ZERO] * 3, [_ZERO] * 3, [_ZERO, _ZERO, t[0]]] if self.planar else \
                    [[t[0], t[1], t[2]], [t[1], t[3], t[4]], [t[2], t[4], t[5]]]
                self.bodies.append((o.end_frame, mpf(float(o.mass)), I, int(o.upstream)))
            elif k == T.KTE_INERTIA_GEN:
                assert int(o.upstream) == 1 << o.coord
                self.rotors[o.coord] += mpf(float(o.mass))
            else:
                assert k == T.KTE_DRIVING_ACTUATOR_GEN, "lagrange_ref: unknown element %d" % k
        assert all(k is not None for k in self.kind)
        # the joints that move a body follow from the frame tree alone; the scene's own mask must say the same
        self.body_joints = []
        for frame, _, _, mask in self.bodies:
            js, f = [], frame
            while f is not None:
                f, c = self.parent[f]
                if c is not None:
                    js.append(c)
            assert sum(1 << c for c in js) == mask, "lagrange_ref: upstream mask disagrees with the frame tree"
            self.body_joints.append(sorted(js))

    def _pos(self, pose):
        return _vec([pose.pos[0], pose.pos[1], 0.0 if self.planar else pose.pos[2]])

    def _rot(self, pose):
        if self.planar:
            return _planar_matrix(mpf(float(pose.quat[0])), mpf(float(pose.quat[1])))
        return _quat_matrix([mpf(float(v)) for v in pose.quat])

    # ---- forward kinematics --------------------------------------------------------------------------------------------
    def fk(self, q):
        """(frames, joints): frames[f] = (origin, rotation) in the world; joints[c] = (world axis, base-frame origin)."""
        fr = {0: (self.base_pos, self.base_R)}
        joints = [None] * self.n
        for what, b, e, c, v, Rm in self.steps:
            p, R = fr[b]
            if what == "R":
                fr[e] = (p, _mm(R, _rodrigues(v, q[c])))
                joints[c] = (_mv(R, v), p)
            elif what == "P":
                fr[e] = (_add(p, _mv(R, _scale(q[c], v))), R)
                joints[c] = (_mv(R, v), p)
            else:
                fr[e] = (_add(p, _mv(R, v)), _mm(R, Rm))
        return fr, joints

    def mass_matrix(self, q, with_G=False):
        """M(q) from the geometric Jacobians; V(q); with_G: the screw pairings too."""
        n = self.n
        fr, joints = self.fk(q)
        M = [[_ZERO] * n for _ in range(n)]
        V = _ZERO
        for c in range(n):
            M[c][c] += self.rotors[c]
        for (frame, m, I, _), js in zip(self.bodies, self.body_joints):
            p, R = fr[frame]
            Iw = _mm(_mm(R, I), _mt(R))
            Jv, Jw = {}, {}
            for c in js:
                a, pc = joints[c]
                if self.kind[c] == "R":
                    Jv[c], Jw[c] = _cross(a, _sub(p, pc)), a
                else:
                    Jv[c], Jw[c] = a, [_ZERO] * 3
            for i in js:
                Iwi = _mv(Iw, Jw[i])
                for j in js:
                    M[i][j] += m * _dot(Jv[i], Jv[j]) + _dot(Iwi, Jw[j])
            V += m * _dot(self.base_acc, p)
        if not with_G:
            return M, V
        G = [[_ONE if i == k else _ZERO for k in range(n)] for i in range(n)]
        if self.joint_rule:
            for i in range(n):
                ai, pi = joints[i]
                for k in range(i + 1, n):
                    ak, pk = joints[k]
                    if self.kind[i] == "R" and self.kind[k] == "R":
                        G[i][k] = _dot(ai, ak)
                    elif self.kind[i] == "R":
                        G[i][k] = _dot(_cross(ai, _sub(pk, pi)), ak)
                    elif self.kind[k] == "P":
                        G[i][k] = _dot(ai, ak)
        return M, V, G

    def kinetic_energy(self, q, qd):
        """T(q, q') by carrying (velocity of the origin, angular velocity), world coordinates, from frame to frame."""
        fr, _ = self.fk(q)
        vel = {0: ([_ZERO] * 3, [_ZERO] * 3)}
        for what, b, e, c, a, _ in self.steps:
            v, w = vel[b]
            p, R = fr[b]
            if what == "R":
                vel[e] = (v, _add(w, _scale(qd[c], _mv(R, a))))
            elif what == "P":
                d = _mv(R, a)
                vel[e] = (_add(_add(v, _cross(w, _scale(q[c], d))), _scale(qd[c], d)), w)
            else:
                vel[e] = (_add(v, _cross(w, _sub(fr[e][0], p))), w)
        Tk = _ZERO
        for c in range(self.n):
            Tk += self.rotors[c] * qd[c] * qd[c] / 2
        for frame, m, I, _ in self.bodies:
            v, w = vel[frame]
            wl = _mv(_mt(fr[frame][1]), w)
            Tk += (m * _dot(v, v) + _dot(wl, _mv(I, wl))) / 2
        return Tk

    def _check_mass_matrix(self, q, M):
        n = self.n
        e = [[_ONE if i == j else _ZERO for j in range(n)] for i in range(n)]
        T1 = [self.kinetic_energy(q, e[i]) for i in range(n)]
        scale = max(abs(M[i][i]) for i in range(n))
        for i in range(n):
            assert abs(2 * T1[i] - M[i][i]) <= MASS_AGREE * scale
            for j in range(i):
                T2 = self.kinetic_energy(q, [e[i][k] + e[j][k] for k in range(n)])
                assert abs(T2 - T1[i] - T1[j] - M[i][j]) <= MASS_AGREE * scale
                assert abs(M[i][j] - M[j][i]) <= MASS_AGREE * scale

    def _derivatives(self, q, h):
        n = self.n
        dM, dV = [], []
        for k in range(n):
            qp, qm = list(q), list(q)
            qp[k] += h
            qm[k] -= h
            Mp, Vp = self.mass_matrix(qp)
            Mm, Vm = self.mass_matrix(qm)
            dM.append([[(Mp[i][j] - Mm[i][j]) / (2 * h) for j in range(n)] for i in range(n)])
            dV.append((Vp - Vm) / (2 * h))
        return dM, dV

    def _coriolis(self, dM, qd):
        n = self.n
        c = []
        for i in range(n):
            s = _ZERO
            for j in range(n):
                for k in range(n):
                    s += (dM[k][i][j] - dM[i][j][k] / 2) * qd[j] * qd[k]
            c.append(s)
        return c

    def evaluate_mp(self, x, u, check=True):
        """The mpmath values (M, c, dVdq, G, f, qdd, kappa, f_lagrange) of one state x = (q0, q0', q1, q1', ...), drive u."""
        n = self.n
        q = [mpf(float(x[2 * j])) for j in range(n)]
        qd = [mpf(float(x[2 * j + 1])) for j in range(n)]
        uu = [mpf(float(v)) for v in u]
        M, _, G = self.mass_matrix(q, with_G=True)
        dM, dV = self._derivatives(q, STEP)
        c = self._coriolis(dM, qd)
        if check:
            self._check_mass_matrix(q, M)
            dM2, dV2 = self._derivatives(q, STEP / 2)
            c2 = self._coriolis(dM2, qd)
            scale = max([_ONE] + [abs(v) for v in c] + [abs(v) for v in dV])
            assert max(abs(a - b) for a, b in zip(c + dV, c2 + dV2)) <= DERIV_AGREE * scale
        fl = [uu[i] - c[i] - dV[i] for i in range(n)]
        f = list(fl)
        for i in range(n - 1, -1, -1):       # G is unit upper triangular
            for k in range(i + 1, n):
                f[i] -= G[i][k] * f[k]
        qdd = list(MP.cholesky_solve(MP.matrix(M), MP.matrix(f)))
        ev = MP.eigsy(MP.matrix(M), eigvals_only=True)
        kappa = max(ev) / min(ev)
        assert min(ev) > 0
        return M, c, dV, G, f, qdd, kappa, fl

    def evaluate(self, x, u, check=True):
        M, c, dV, G, f, qdd, kappa, fl = self.evaluate_mp(x, u, check)
        d1 = lambda v: np.array([float(t) for t in v])
        d2 = lambda m: np.array([[float(t) for t in r] for r in m])
        return Result(M=d2(M), c=d1(c), dVdq=d1(dV), G=d2(G), f=d1(f), qdd=d1(qdd), kappa=float(kappa), f_lagrange=d1(fl))


def g_inverse_norm(G):
    """||G^-1||_inf of a (unit upper triangular) G given in doubles."""
    return float(np.abs(np.linalg.inv(G)).sum(axis=1).max())


# ---- tolerances (derived, not tuned: 1e-12 is ~4500 ulp, room for the n-term sums and for sin/cos of another libm) ----
TOL = 1e-12


def bounds(M_ref, G_ref, c_ref, dV_ref, u, qdd_ref, kappa):
    """(bound on |M - M_ref|_max, on |f - f_ref|_inf, on |q'' - q''_ref|_inf) of one state."""
    bM = TOL * np.abs(M_ref).max()
    bf = TOL * g_inverse_norm(G_ref) * (np.abs(u).max() + np.abs(c_ref).max() + np.abs(dV_ref).max())
    bq = TOL * kappa * max(1.0, np.abs(qdd_ref).max())
    return bM, bf, bq


def ratios(M, f, qdd, ref, i):
    """error / bound of (M, f, q'') of state i against a family's golden arrays `ref`."""
    bM, bf, bq = bounds(ref["M"][i], ref["G"][i], ref["c"][i], ref["dVdq"][i], ref["u"][i], ref["qdd"][i], ref["kappa"][i])
    ef = np.abs(f - ref["f"][i]).max()
    return np.abs(M - ref["M"][i]).max() / bM, (ef / bf if bf > 0 else float(ef > 0)), np.abs(qdd - ref["qdd"][i]).max() / bq


# ---- case families -----------------------------------------------------------------------------------------------------
N_STATES = 24
_SCALE = [0.7, 1.3, 0.9, 1.1, 0.8, 1.2, 1.0]   # prismatic axes are not unit length (test_pair_feval_frames_gpu.py)


def mixed_chain(n, prism):
    """make_random_chain(n, seed=n) with the joints in `prism` made prismatic along their scaled, non-unit axes, travel
    +-0.5: the scenes of tests/test_pair_feval_frames_gpu.py::_scene."""
    scn = scenarios.make_random_chain(n, seed=n)
    for j, op in enumerate([o for o in scn.ops if o.kind == T.KTE_REVOLUTE_JOINT_3D]):
        if j in prism:
            op.kind = T.KTE_PRISMATIC_JOINT_3D
            op.axis[:] = [_SCALE[j] * v for v in op.axis]
            scn.dyn.lower[2 * j], scn.dyn.upper[2 * j] = -0.5, 0.5
    scn.name = "mixed%d_p%s" % (n, "".join(map(str, prism)))
    return scn


def hand_chain(name, axes, offsets, masses, tensors, rotors, gravity=(0.0, 0.0, 9.81)):
    n = len(axes)
    ops = scenarios.serial_chain_ops(axes, offsets, masses, tensors, rotors)
    base = T.ChainBase()
    base.pose = T.make_pose((0.1, 0.0, 0.2), (math.cos(0.2), math.sin(0.2) * 0.6, 0.0, math.sin(0.2) * 0.8))
    base.acceleration[:] = list(gravity)
    dyn = T.DynSpace()
    dyn.n_dof, dyn.steps_per_edge, dyn.dt = n, 20, 1e-3
    dyn.kp, dyn.kd, dyn.u_max, dyn.goal_tol = 40.0, 8.0, 40.0, 1e-3
    for j in range(n):
        dyn.lower[2 * j], dyn.upper[2 * j] = -np.pi, np.pi
        dyn.lower[2 * j + 1], dyn.upper[2 * j + 1] = -2.0, 2.0
    return scenarios.Scenario(name=name, ops=ops, base=base, shapes=[], dyn=dyn, n_dof=n, n_frames=2 * n + 1,
                              start=np.zeros(2 * n), goal=np.zeros(2 * n))


_FULL = (0.05, 0.012, -0.009, 0.04, 0.015, 0.03)     # a full, non-diagonal, positive definite tensor
_DIAG = (0.02, 0.0, 0.0, 0.03, 0.0, 0.01)


def hand_parallel():       # G_01 = 1
    return hand_chain("hand_parallel", [(0, 0, 1), (0, 0, 1)], [(0.3, 0.05, 0.1), (0.2, -0.04, 0.05)], [2.0, 1.0],
                      [_DIAG, _FULL], [0.3, 0.2])


def hand_antiparallel():   # G_01 = -1
    return hand_chain("hand_antiparallel", [(0, 0, 1), (0, 0, -1)], [(0.3, 0.05, 0.1), (0.2, -0.04, 0.05)], [2.0, 1.0],
                      [_DIAG, _FULL], [0.3, 0.2])


def hand_orthogonal():     # G_01 = G_12 = 0, G_02 = cos q1
    return hand_chain("hand_orthogonal", [(0, 0, 1), (1, 0, 0), (0, 1, 0)], [(0.0, 0.05, 0.3), (0.2, 0.0, 0.05), (0.0, 0.1, 0.15)],
                      [2.0, 1.5, 1.0], [_DIAG, _FULL, _FULL], [0.3, 0.2, 0.1])


def hand_zero_offset():    # joints 1 and 2 share their origin (a wrist)
    return hand_chain("hand_zero_offset", [(0, 0, 1), (0, -1, 0), (0.6, 0.0, 0.8)], [(0.0, 0.0, 0.3), (0.0, 0.0, 0.0), (0.1, 0.0, 0.2)],
                      [2.0, 1.5, 1.0], [_DIAG, _DIAG, _FULL], [0.3, 0.2, 0.1])


def hand_gyro():
    """Two orthogonal axes through one point, no offsets, no gravity; the last link carries the full tensor.  With u = 0
    nothing but  w x I w  of the spinning last link drives joint 0."""
    return hand_chain("hand_gyro", [(0, 0, 1), (1, 0, 0)], [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0)], [1.0, 2.0],
                      [(0.0,) * 6, _FULL], [0.05, 0.02], gravity=(0.0, 0.0, 0.0))


def _family_list():
    out = [("pendulum", scenarios.make_pendulum, 11), ("c2", scenarios.make_c2, 12)]
    for n in (1, 2, 3, 4, 6, 7):
        out.append(("chain%d" % n, (lambda n=n: scenarios.make_random_chain(n)), 20 + n))
    out.append(("track", scenarios.make_crs_a465_track, 31))
    for n, prism in ((4, (0,)), (3, (2,)), (6, (5,)), (4, (1, 2))):
        out.append(("mixed%d_p%s" % (n, "".join(map(str, prism))), (lambda n=n, p=prism: mixed_chain(n, p)), 40 + n + 7 * len(prism) + prism[0]))
    for k, fn in enumerate((hand_parallel, hand_antiparallel, hand_orthogonal, hand_zero_offset, hand_gyro)):
        out.append((fn.__name__, fn, 60 + k))
    out.append(("c1_planar", (lambda: scenarios.make_c1_planar(dynamics=True)), 71))
    out.append(("crs_a465_2d", (lambda: scenarios.make_crs_a465_2d(dynamics=True)), 72))
    for k, fn in enumerate((pps.lone_p, pps.p_r, pps.r_p, pps.seven)):
        out.append(("planar_" + fn.__name__, fn, 80 + k))
    return out


FAMILIES = _family_list()            # (name, scene maker, state seed)
FAMILY_NAMES = [f[0] for f in FAMILIES]
PLANAR_FAMILIES = [n for n in FAMILY_NAMES if n in ("c1_planar", "crs_a465_2d") or n.startswith("planar_")]
SPATIAL_FAMILIES = [n for n in FAMILY_NAMES if n not in PLANAR_FAMILIES]


def scene(name):
    return {f[0]: f[1] for f in FAMILIES}[name]()


def is_prismatic(scn):
    joints = [o for o in scn.ops if o.kind in _REV + _PRI]
    return [o.kind in _PRI for o in sorted(joints, key=lambda o: o.coord)]


def states(name, scn=None):
    """(x [24][2n], u [24][n]) of a family: q uniform in the scene's position bounds (revolute bounds beyond +-pi are cut
    to +-pi), q' in [-2, 2], u in [-10, 10]; rows 0..5 are the fixed edge rows (at rest; u = 0; one joint at exactly 0; a
    joint at its upper bound, +pi where the bounds allow; a joint at its lower bound, a prismatic one if there is one; all
    q = 0)."""
    scn = scene(name) if scn is None else scn
    seed = {f[0]: f[2] for f in FAMILIES}[name]
    n = scn.n_dof
    prism = is_prismatic(scn)
    lo = np.array([scn.dyn.lower[2 * j] if prism[j] else max(scn.dyn.lower[2 * j], -np.pi) for j in range(n)])
    hi = np.array([scn.dyn.upper[2 * j] if prism[j] else min(scn.dyn.upper[2 * j], np.pi) for j in range(n)])
    rng = np.random.default_rng(9000 + seed)
    q = rng.uniform(lo, hi, size=(N_STATES, n))
    qd = rng.uniform(-2.0, 2.0, size=(N_STATES, n))
    u = rng.uniform(-10.0, 10.0, size=(N_STATES, n))
    rev = [j for j in range(n) if not prism[j]]
    pri = [j for j in range(n) if prism[j]]
    qd[0] = 0.0
    u[1] = 0.0
    q[2, seed % n] = 0.0
    j_up = rev[-1] if rev else pri[-1]
    q[3, j_up] = hi[j_up]
    j_lo = pri[0] if pri else rev[0]
    q[4, j_lo] = lo[j_lo]
    q[5] = 0.0
    x = np.zeros((N_STATES, 2 * n))
    x[:, 0::2], x[:, 1::2] = q, qd
    return x, u


GOLDEN_KEYS = ("x", "u", "M", "f", "qdd", "kappa", "G", "c", "dVdq")


def reference_arrays(name, rows=None, joint_rule=True):
    """The golden arrays of a family (all rows, or the given ones), computed live."""
    scn = scene(name)
    x, u = states(name, scn)
    rows = range(len(x)) if rows is None else rows
    model = Model(scn, joint_rule=joint_rule)
    res = [model.evaluate(x[i], u[i]) for i in rows]
    rows = list(rows)
    return {"x": x[rows], "u": u[rows], "M": np.array([r.M for r in res]), "f": np.array([r.f for r in res]),
            "qdd": np.array([r.qdd for r in res]), "kappa": np.array([r.kappa for r in res]),
            "G": np.array([r.G for r in res]), "c": np.array([r.c for r in res]), "dVdq": np.array([r.dVdq for r in res])}


def load_golden(path):
    z = np.load(path)
    return {name: {k: z[name + "/" + k] for k in GOLDEN_KEYS} for name in FAMILY_NAMES}
