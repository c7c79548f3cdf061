"""Test-side CPU restatement of the KTE chain passes for PLANAR serial chains of revolute_joint_2D AND prismatic_joint_2D
groups, in the style of tests/kte_ref.py.

The oracle's KteChain (oracle/reak_kte.hpp) does not know prismatic_joint_2D: its doMotion / doForce fall through
`default: break`, so such a scene handed to it gives wrong numbers without an error.  This module restates, in plain
Python floats (IEEE double, the oracle's operation order), what the tests need on such scenes:

  kte_map_chain::doMotion / clearForce / doForce    oracle/reak_kte.hpp's 2D branches (revolute_joint_2D, rigid_link_2D,
                                                    inertia_gen, inertia_2D, driving_actuator_gen) + prismatic_joint_2D
                                                    from ctrl/mbd_kte/prismatic_joint.cpp:33-123 of the reference
  mass_matrix_calc::getMassMatrix                   the 2D rows (get_jac_relative_to_2D, Mcm * Tcm, symmetrise)
  kte_nl_system::get_state_derivative               Cholesky solve, pivot < 1e-8 -> Singular
  steer_position_toward (RK4 + is_free)             kte_ref.steer over this chain (oracle/reak_planning.hpp DynSpace)
  interp_topo_move_position_toward_pred             qs_move below, rate-limited coordinates included (QuasiStaticSpace)
  proxy_query_pair_2D::findMinimumDistance          replayed in the scene's finder order with its cull against the running
                                                    minimum (proxy_query_model.cpp:163-189); every pair distance comes from
                                                    the oracle's closed forms (orc_pair_distance)
  generate_rrt                                      oracle/reak_planning.hpp, over either space; samples from
                                                    orc_sample_hyperbox, nearest neighbours from orc_nn1

Revolute-only chains are pinned against the oracle itself, bit for bit (test_prismatic_planar_cpu.py)."""
import ctypes as C
import math

import numpy as np

import kte_ref
from kte_ref import Singular, euclid, in_bounds  # noqa: F401  (re-exported)
from reak_amd import types as T

JOINTS = (T.KTE_REVOLUTE_JOINT_2D, T.KTE_PRISMATIC_JOINT_2D)


# ---- vect<double,2>, rot_mat_2D (oracle/reak_planar.hpp; a rotation is q = (cos, sin)) --------------------------------
def add(a, b):
    return (a[0] + b[0], a[1] + b[1])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1])


def smul(s, a):
    return (a[0] * s, a[1] * s)


def dot(a, b):
    r = 0.0
    for i in range(2):
        r += a[i] * b[i]
    return r


def cross_sv(S, V):  # scalar % vect (vect_alg.hpp:1171-1176)
    return (-V[1] * S, V[0] * S)


def cross_vv(a, b):  # vect % vect (vect_alg.hpp:1142-1144)
    return a[0] * b[1] - a[1] * b[0]


def rmul(a, b):  # rot_mat_2D * rot_mat_2D
    return (a[0] * b[0] - a[1] * b[1], a[1] * b[0] + a[0] * b[1])


def rrot(R, V):  # rot_mat_2D * vect
    return (V[0] * R[0] - V[1] * R[1], V[0] * R[1] + V[1] * R[0])


def rrotT(V, R):  # vect * rot_mat_2D (= transpose(R) * vect)
    return (V[0] * R[0] + V[1] * R[1], V[1] * R[0] - V[0] * R[1])


Z2 = (0.0, 0.0)


class Frame2:
    __slots__ = ("pos", "R", "acc", "w", "alpha", "F", "Tq")

    def __init__(self):
        self.pos, self.R, self.acc, self.w, self.alpha, self.F, self.Tq = Z2, (1.0, 0.0), Z2, 0.0, 0.0, Z2, 0.0


class Chain:
    """kte_map_chain of a scenario's ops (planar serial chains of revolute / prismatic groups)."""

    def __init__(self, scn):
        self.ops = [dict(kind=o.kind, coord=o.coord, base=o.base_frame, end=o.end_frame, joint_op=o.joint_op,
                         upstream=o.upstream, axis=(o.axis[0], o.axis[1]), pos=(o.offset.pos[0], o.offset.pos[1]),
                         rot=(o.offset.quat[0], o.offset.quat[1]), mass=o.mass, inertia=o.inertia[0]) for o in scn.ops]
        for o in self.ops:
            assert o["kind"] in (T.KTE_DRIVING_ACTUATOR_GEN, T.KTE_INERTIA_GEN, T.KTE_RIGID_LINK_2D, T.KTE_INERTIA_2D) + \
                JOINTS, "kte_ref_planar: planar serial chains of revolute / prismatic groups only"
        self.n = max(o["coord"] for o in self.ops) + 1
        self.n_frames = max(max(o["base"], o["end"]) for o in self.ops) + 1
        self.base_pos = (scn.base.pose.pos[0], scn.base.pose.pos[1])
        self.base_R = (scn.base.pose.quat[0], scn.base.pose.quat[1])
        self.base_acc = (scn.base.acceleration[0], scn.base.acceleration[1])
        self.gen = [o for o in self.ops if o["kind"] == T.KTE_INERTIA_GEN]
        self.in2 = [o for o in self.ops if o["kind"] == T.KTE_INERTIA_2D]
        self.shapes = list(scn.shapes)

    # kte_map_chain::doMotion (velocities are not carried: no force term of these elements reads one)
    def do_motion(self, q, qd, qdd):
        fr = [Frame2() for _ in range(self.n_frames)]
        fr[0].pos, fr[0].R, fr[0].acc = self.base_pos, self.base_R, self.base_acc
        jac = [None] * self.n
        for o in self.ops:
            k = o["kind"]
            if k == T.KTE_REVOLUTE_JOINT_2D:  # revolute_joint.cpp:30-56
                B, E, c = fr[o["base"]], fr[o["end"]], o["coord"]
                E.pos, E.acc = B.pos, B.acc
                E.R = rmul(B.R, (math.cos(q[c]), math.sin(q[c])))
                E.w = B.w + qd[c]
                E.alpha = B.alpha + qdd[c]
                jac[c] = (o["end"], Z2, 1.0)
            elif k == T.KTE_PRISMATIC_JOINT_2D:  # prismatic_joint.cpp:44-62
                B, E, c, ax = fr[o["base"]], fr[o["end"]], o["coord"], o["axis"]
                tmp_pos, tmp_vel = smul(q[c], ax), smul(qd[c], ax)
                E.pos = add(B.pos, rrot(B.R, tmp_pos))
                E.acc = add(B.acc, rrot(B.R, add(add(add(smul(-B.w * B.w, tmp_pos), cross_sv(2.0 * B.w, tmp_vel)),
                                                     cross_sv(B.alpha, tmp_pos)), smul(qdd[c], ax))))
                E.R, E.w, E.alpha = B.R, B.w, B.alpha
                jac[c] = (o["end"], ax, 0.0)
            elif k == T.KTE_RIGID_LINK_2D:  # rigid_link.cpp:87-99
                B, E = fr[o["base"]], fr[o["end"]]
                E.pos = add(B.pos, rrot(B.R, o["pos"]))
                E.acc = add(B.acc, rrot(B.R, add(smul(-B.w * B.w, o["pos"]), cross_sv(B.alpha, o["pos"]))))
                E.R = rmul(B.R, o["rot"])
                E.w, E.alpha = B.w, B.alpha
        return fr, jac

    # kte_map_chain::clearForce + doForce (reverse op order)
    def do_force(self, fr, q, qdd, u):
        for f in fr:
            f.F, f.Tq = Z2, 0.0
        f = [0.0] * self.n
        for o in reversed(self.ops):
            k = o["kind"]
            if k == T.KTE_DRIVING_ACTUATOR_GEN:  # driving_actuator.cpp:31-39 + the joint's applyReactionForce
                c = o["coord"]
                f[c] += u[c]
                j = self.ops[o["joint_op"]]
                B = fr[j["base"]]
                if j["kind"] == T.KTE_PRISMATIC_JOINT_2D:  # prismatic_joint.cpp:120-123
                    B.F = sub(B.F, smul(u[c], j["axis"]))
                else:  # revolute_joint.cpp:112-115
                    B.Tq = B.Tq - u[c]
            elif k == T.KTE_INERTIA_GEN:  # inertia.cpp:47-54
                f[o["coord"]] -= qdd[o["coord"]] * o["mass"]
            elif k == T.KTE_REVOLUTE_JOINT_2D:  # revolute_joint.cpp:58-67: nothing reaches the base's torque
                B, E, c = fr[o["base"]], fr[o["end"]], o["coord"]
                B.F = add(B.F, rrot((math.cos(q[c]), math.sin(q[c])), E.F))
                f[c] += E.Tq
            elif k == T.KTE_PRISMATIC_JOINT_2D:  # prismatic_joint.cpp:82-94
                B, E, c, ax = fr[o["base"]], fr[o["end"]], o["coord"], o["axis"]
                tmp_f = dot(E.F, ax)
                f[c] += tmp_f
                B.F = add(B.F, sub(E.F, smul(tmp_f, ax)))
                B.Tq = B.Tq + (E.Tq + cross_vv(smul(q[c], ax), E.F))
            elif k == T.KTE_RIGID_LINK_2D:  # rigid_link.cpp:104-106
                B, E = fr[o["base"]], fr[o["end"]]
                tf = rrot(o["rot"], E.F)
                B.F = add(B.F, tf)
                B.Tq = B.Tq + (E.Tq + cross_vv(o["pos"], tf))
            elif k == T.KTE_INERTIA_2D:  # inertia.cpp:73-81
                Fr = fr[o["end"]]
                Fr.F = sub(Fr.F, smul(o["mass"], rrotT(Fr.acc, Fr.R)))
                Fr.Tq = Fr.Tq - o["inertia"] * Fr.alpha
        return f

    def _jac_rel(self, fr, J, a_frame):  # jacobian_gen_2D::get_jac_relative_to (motion_jacobians.hpp:138-146)
        parent, qd_vel, qd_avel = J
        Pf, A = fr[parent], fr[a_frame]
        inv_pos = rrotT((-Pf.pos[0], -Pf.pos[1]), Pf.R)
        inv_rot = (Pf.R[0], -Pf.R[1])
        f2_pos = add(inv_pos, rrot(inv_rot, A.pos))
        f2_rot = rmul(inv_rot, A.R)
        return rrotT(add(cross_sv(qd_avel, f2_pos), qd_vel), f2_rot), qd_avel

    def mass_matrix(self, fr, jac):  # mass_matrix_calc::getMassMatrix (reak_kte.hpp), 2D rows
        n = self.n
        m = len(self.gen) + 3 * len(self.in2)
        Tcm = [[0.0] * n for _ in range(m)]
        diag = [0.0] * m
        for i in range(n):
            row = 0
            for o in self.gen:
                if o["upstream"] & (1 << i):
                    Tcm[row][i] = 1.0
                row += 1
            for o in self.in2:
                if o["upstream"] & (1 << i):
                    v, w = self._jac_rel(fr, jac[i], o["end"])
                    Tcm[row][i], Tcm[row + 1][i], Tcm[row + 2][i] = v[0], v[1], w
                row += 3
        row = 0
        for o in self.gen:
            diag[row] = o["mass"]
            row += 1
        for o in self.in2:
            diag[row], diag[row + 1], diag[row + 2] = o["mass"], o["mass"], o["inertia"]
            row += 3
        # P = Mcm * Tcm with a diagonal Mcm (mat_alg_symmetric.hpp:551-566): the off-diagonal terms add exact zeros
        P = [[0.0 + diag[j] * Tcm[j][l] for l in range(n)] for j in range(m)]
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
        """[n_frames][4] = position, rotation (cos, sin) of every frame after doMotion (apply_kinematics)."""
        n = self.n
        fr, _ = self.do_motion([float(x[2 * j]) for j in range(n)], [float(x[2 * j + 1]) for j in range(n)], [0.0] * n)
        return np.array([list(f.pos) + list(f.R) for f in fr])

    def posed_shapes(self, x):
        """(robot shapes, environment shapes) as world-anchored rkh_shape copies (pose_2D::getGlobalPose)."""
        fr = self.frames(x)
        robot, env = [], []
        for s in self.shapes:
            if s.anchor >= 0:
                c = T.Shape(kind=s.kind, anchor=-1)
                c.dims[:] = list(s.dims)
                P, R = (fr[s.anchor][0], fr[s.anchor][1]), (fr[s.anchor][2], fr[s.anchor][3])
                gp = add(P, rrot(R, (s.pose.pos[0], s.pose.pos[1])))
                gr = rmul(R, (s.pose.quat[0], s.pose.quat[1]))
                c.pose.pos[:] = [gp[0], gp[1], 0.0]
                c.pose.quat[:] = [gr[0], gr[1], 0.0, 0.0]
                robot.append(c)
            else:
                env.append(s)
        return robot, env


def _brad(s):  # circle.cpp:31-33; rectangle.cpp / capped_rectangle.cpp:31-33: norm_2(mDimensions) * 0.5
    if s.kind == T.SHAPE_CIRCLE:
        return s.dims[0]
    return math.sqrt((0.0 + s.dims[0] * s.dims[0]) + s.dims[1] * s.dims[1]) * 0.5


def _rank(kind):  # createProxFinderList's cascade: the circle is shape1, else the capped rectangle, else model 1's shape
    return {T.SHAPE_CIRCLE: 0, T.SHAPE_CRECT: 1, T.SHAPE_RECTANGLE: 2}[kind]


class Distances:
    """proxy_query_pair_2D::findMinimumDistance of a configuration: shapes posed by Chain, the finders in
    createProxFinderList's i-major / j-minor order, each culled against the running minimum, distances through
    orc_pair_distance.  `closest` keeps the smallest |minimum distance| of every query so far (how near the run came to
    a verdict that rounding could turn)."""

    def __init__(self, chain, oracle_lib):
        self.chain, self.lib = chain, oracle_lib.load()
        self.closest = math.inf
        self.queries = 0

    def min_distance(self, x):
        robot, env = self.chain.posed_shapes(x)
        min_dist, first = math.inf, True
        for r in robot:
            for e in env:
                if not first:
                    s1, s2 = (e, r) if _rank(e.kind) < _rank(r.kind) else (r, e)
                    dx, dy = s2.pose.pos[0] - s1.pose.pos[0], s2.pose.pos[1] - s1.pose.pos[1]
                    if math.sqrt(dx * dx + dy * dy) - _brad(s1) - _brad(s2) > min_dist:
                        continue
                d = self.lib.orc_pair_distance(C.byref(r), C.byref(e))
                if first:
                    min_dist, first = d, False
                elif d < min_dist:
                    min_dist = d
        self.queries += 1
        self.closest = min(self.closest, abs(min_dist))
        return min_dist

    def is_free(self, x):
        return not (self.min_distance(x) < 0.0)


def steer(chain, dist, dyn, a, b, fraction=1.0):
    """DynSpace::steer_position_toward: (last free state, accepted steps, record, min distance of every tested state)."""
    return kte_ref.steer(chain, dist, dyn, a, b, fraction)


def qs_move(chain, dist, lower, upper, min_interval, a, b, fraction=1.0, speed=None):
    """QuasiStaticSpace::move_position_toward: (result, is_free calls, completed).  speed: the rate-limited joint space
    (points hold q_i / speed_i, the model is evaluated at point_i * speed_i)."""
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
        x[0::2] = p if speed is None else [p[i] * float(speed[i]) for i in range(n)]
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


class DynSpace:
    """oracle/reak_planning.hpp DynSpace over the restated chain."""

    def __init__(self, chain, dist, dyn):
        self.chain, self.dist, self.dyn, self.D = chain, dist, dyn, 2 * chain.n
        self.lower, self.upper = [dyn.lower[i] for i in range(self.D)], [dyn.upper[i] for i in range(self.D)]

    def move(self, a, b):
        return steer(self.chain, self.dist, self.dyn, a, b, 1.0)[0]

    def is_free(self, x):
        return in_bounds([float(v) for v in x], self.lower, self.upper) and self.dist.is_free(np.asarray(x, dtype=float))

    def distance(self, a, b):  # MEAQR_topology_with_CD::distance
        r = self.move(a, b)
        return euclid(a, b) if euclid(a, b) * 0.05 > euclid(r, b) else math.inf


class QsSpace:
    """oracle/reak_planning.hpp QuasiStaticSpace over the restated chain (qs: rkh_qs_space, speed_limits honoured)."""

    def __init__(self, chain, dist, qs):
        self.chain, self.dist, self.D = chain, dist, qs.n_dof
        self.lower, self.upper = [qs.lower[i] for i in range(self.D)], [qs.upper[i] for i in range(self.D)]
        self.min_interval = qs.min_interval
        sp = [qs.speed_limits[i] if qs.speed_limits[i] != 0.0 else 1.0 for i in range(self.D)]
        self.speed = sp if any(v != 1.0 for v in sp) else None  # (p * 1.0 == p: the ordinary space either way)

    def move(self, a, b):
        return qs_move(self.chain, self.dist, self.lower, self.upper, self.min_interval, a, b, 1.0, self.speed)[0]

    def is_free(self, p):
        p = [float(v) for v in p]
        if not in_bounds(p, self.lower, self.upper):
            return False
        x = np.zeros(2 * self.D)
        x[0::2] = p if self.speed is None else [p[i] * self.speed[i] for i in range(self.D)]
        return self.dist.is_free(x)

    def distance(self, a, b):  # interp_topo_get_distance_pred
        r = self.move(a, b)
        return euclid(a, b) if euclid(r, b) < np.finfo(float).eps else math.inf


def generate_rrt(space, prm, oracle_lib, max_iterations=-1):
    """generate_rrt of oracle/reak_planning.hpp over `space` (DynSpace or QsSpace): the tree as rkh_planner_get_tree
    gives it (pos, parent, nn_seq, accept, goal_dist) plus iterations, num_solutions and best_cost."""
    lib = oracle_lib.load()
    D = space.D
    start, goal = [prm.start[i] for i in range(D)], [prm.goal[i] for i in range(D)]
    budget = int(max_iterations) if max_iterations >= 0 else 16 * int(prm.max_vertices)
    lo, up = np.array(space.lower, dtype=np.float64), np.array(space.upper, dtype=np.float64)
    samples = np.zeros((max(budget, 1), D))
    lib.orc_sample_hyperbox(int(prm.seed), T.dptr(lo), T.dptr(up), D, budget, T.dptr(samples))
    pos, parent, nn_seq, accept, goal_dist = [start], [0xFFFFFFFF], [], [], []
    added, iterations, num_solutions, best_cost = 0, 0, 0, math.inf
    idx, dd = np.zeros(1, dtype=np.uint32), np.zeros(1)
    while added < prm.max_vertices and prm.max_results > num_solutions and iterations < budget:
        p_rnd = [float(v) for v in samples[iterations]]
        iterations += 1
        pts = np.ascontiguousarray(pos, dtype=np.float64)
        q = np.ascontiguousarray([p_rnd], dtype=np.float64)
        lib.orc_nn1(T.dptr(q), 1, T.dptr(pts), len(pos), D, T.u32ptr(idx), T.dptr(dd))
        u = int(idx[0])
        nn_seq.append(u)
        p_v = [float(v) for v in space.move(pos[u], p_rnd)]
        traveled, best_case = euclid(pos[u], p_v), euclid(pos[u], p_rnd)
        reached = (not math.isinf(traveled)) and traveled < 2.0 * best_case and traveled > prm.steer_tol * best_case
        accept.append(1 if reached else 0)
        if not reached:
            continue
        pos.append(p_v)
        parent.append(u)
        added += 1
        gd = space.distance(p_v, goal)
        goal_dist.append(gd)
        if gd < math.inf:
            total, v = gd, len(parent) - 1
            while parent[v] != 0xFFFFFFFF:
                total += euclid(pos[parent[v]], pos[v])
                v = parent[v]
            if num_solutions == 0 or total < best_cost:
                best_cost = total
                num_solutions += 1
    return {"pos": np.array(pos), "parent": np.array(parent, dtype=np.uint32), "nn_seq": np.array(nn_seq, dtype=np.uint32),
            "accept": np.array(accept, dtype=np.uint8), "goal_dist": np.array(goal_dist), "iterations": iterations,
            "num_solutions": num_solutions, "best_cost": best_cost}
