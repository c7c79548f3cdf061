"""Prismatic joints in planar chains, CPU side: the test-side restatement (tests/kte_ref_planar.py) pinned against the
oracle on revolute chains (bit for bit), against closed forms on prismatic ones and against tests/kte_ref.py on the 3D
twin of the same mechanism, and the resources of the planar prismatic kernel instantiations.  No GPU.

No host-only rule was added for these forms (their launchers reuse the revolute launch shapes), so there is no
stand-alone C++ test to go with them."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kte_ref  # noqa: E402
import kte_ref_planar as krp  # noqa: E402
import oracle_lib  # noqa: E402
import planar_prismatic_scenes as pps  # noqa: E402
from reak_amd import scenarios  # noqa: E402
from reak_amd import types as T  # noqa: E402


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


# ------------------------------------------------------------------------ 1. the restatement against the oracle
def test_restatement_dynamics_match_the_oracle_bit_for_bit():
    """Planar 3R arm with dynamics: pd, M, f, frames, min distances and steer outputs are the oracle's own bits."""
    scn = scenarios.make_c1_planar(dynamics=True)
    osc, ch = oracle_lib.OracleScene(scn), krp.Chain(scn)
    dist = krp.Distances(ch, oracle_lib)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.5, 1.5, size=(16, scn.D))
    u = rng.uniform(-10, 10, size=(16, scn.n_dof))
    rc, pd, M, f = osc.state_derivative(x, u)
    assert rc == 0
    fk, dmin = osc.fk(x), osc.min_distance(x)
    for i in range(len(x)):
        p2, M2, f2 = ch.state_derivative(x[i], u[i])
        assert np.array_equal(p2, pd[i]) and np.array_equal(M2, M[i]) and np.array_equal(f2, f[i])
        assert np.array_equal(ch.frames(x[i]), fk[i][:, [0, 1, 3, 4]])
        assert dist.min_distance(x[i]) == dmin[i]
    a = np.zeros((4, scn.D))
    a[:, 0::2] = rng.uniform(-0.3, 0.3, size=(4, 3))
    b = a + rng.uniform(-0.5, 0.5, size=a.shape)
    rc, out, steps, rec = osc.steer(a, b, record=True)
    assert rc == 0
    for i in range(len(a)):
        xe, n_free, r2, _ = krp.steer(ch, dist, scn.dyn, a[i], b[i])
        assert n_free == steps[i] and np.array_equal(xe, out[i]) and np.array_equal(r2, rec[i][: n_free + 1])


@pytest.mark.parametrize("n", [2, 4, 7])
def test_restatement_position_level_matches_the_oracle_bit_for_bit(n):
    """Mixed planar arms (every 2D pair routine): frames, min distances (finder order and cull) and quasi-static walks."""
    scn = scenarios.make_planar_mixed(seed=2, n=n)
    osc, ch = oracle_lib.OracleScene(scn), krp.Chain(scn)
    dist = krp.Distances(ch, oracle_lib)
    rng = np.random.default_rng(40 + n)
    x = np.zeros((24, 2 * n))
    x[:, 0::2] = rng.uniform(-2.0, 2.0, size=(24, n))
    fk, dmin = osc.fk(x), osc.min_distance(x)
    for i in range(len(x)):
        assert np.array_equal(ch.frames(x[i]), fk[i][:, [0, 1, 3, 4]])
        assert dist.min_distance(x[i]) == dmin[i]
    lo, up, mi = scn.meta["lower"], scn.meta["upper"], scn.meta["min_interval"]
    a, b = rng.uniform(-0.15, 0.15, size=(12, n)), rng.uniform(-2.5, 2.5, size=(12, n))
    b[:3] = a[:3] + 0.01  # shorter than min_interval
    out, nchk = osc.qs_move(lo, up, mi, a, b)
    for i in range(len(a)):
        r, c = krp.qs_move(ch, dist, lo, up, mi, a[i], b[i])
        assert c == nchk[i] and np.array_equal(r, out[i])
    assert nchk.max() >= 2 and (nchk[:3] == 0).all() and (nchk[3:] > 0).all()  # (cluttered scenes: walks end early)


def _same_tree(t, o):
    return (np.array_equal(t["pos"], o["pos"]) and np.array_equal(t["parent"], o["parent"]) and
            np.array_equal(t["nn_seq"], o["nn_seq"]) and np.array_equal(t["accept"], o["accept"]) and
            np.array_equal(t["goal_dist"], o["goal_dist"]))


def test_restatement_rrt_matches_the_oracle_logs():
    """generate_rrt over both spaces, 100 iterations: the oracle's rrt_dyn and rrt_qs logs exactly."""
    scn = scenarios.make_c1_planar(dynamics=True)
    osc, ch = oracle_lib.OracleScene(scn), krp.Chain(scn)
    prm = scn.rrt_params(seed=5, max_vertices=1000)
    rc, out, tree = osc.rrt_dyn(prm, 100)
    assert rc == 0 and out.iterations == 100
    mine = krp.generate_rrt(krp.DynSpace(ch, krp.Distances(ch, oracle_lib), scn.dyn), prm, oracle_lib, 100)
    assert _same_tree(mine, tree) and mine["num_solutions"] == out.num_solutions
    qsn = scenarios.make_c1_planar()
    osq, chq = oracle_lib.OracleScene(qsn), krp.Chain(qsn)
    prm = qsn.rrt_params(seed=6, max_vertices=1000)
    rc, out, tree = osq.rrt_qs(qsn.meta["lower"], qsn.meta["upper"], qsn.meta["min_interval"], prm, 100)
    assert rc == 0 and out.iterations == 100
    from reak_amd import lib as L
    qs = L.make_qs_space(3, qsn.meta["lower"], qsn.meta["upper"], qsn.meta["min_interval"])
    mine = krp.generate_rrt(krp.QsSpace(chq, krp.Distances(chq, oracle_lib), qs), prm, oracle_lib, 100)
    assert _same_tree(mine, tree) and mine["num_solutions"] == out.num_solutions and len(tree["pos"]) > 20


# ------------------------------------------------------------------------ 2. closed forms on prismatic chains
def _chain(kinds, axes, offsets, masses, moments, rotors, gravity, base_angle=0.0):
    ops = scenarios.planar_chain_ops(offsets, dynamics=True, masses=masses, moments=moments, joint_inertias=rotors,
                                     kinds=kinds, axes=axes)
    base = T.ChainBase()
    base.pose = T.make_pose_2d((0.1, 0.2), base_angle)
    base.acceleration[:] = [gravity[0], gravity[1], 0.0]
    n = len(kinds)
    return scenarios.Scenario(name="cf", ops=ops, base=base, shapes=[], dyn=T.DynSpace(), n_dof=n, n_frames=2 * n + 1,
                              start=np.zeros(2 * n), goal=np.zeros(2 * n))


@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_lone_joint_closed_form(scale):
    """A prismatic_joint_2D along the base acceleration carrying mass m on rotor inertia J: q'' = (u - m g) / (J + m);
    with the axis scaled (it is used as given), q'' = (u - m g s) / (J + m s^2)."""
    m, J, g = 3.0, 1.0, 9.81
    ch = krp.Chain(_chain([pps.P], [(0.0, scale)], [0.2], [m], [0.3], [J], (0.0, g)))
    for q, qd, u in [(0.0, 0.0, 0.0), (0.7, -1.3, 12.0), (-2.0, 0.4, -5.0)]:
        pd, Mm, f = ch.state_derivative([q, qd], [u])
        expect = (u - m * g * scale) / (J + m * scale * scale)
        assert pd[0] == qd and abs(pd[1] - expect) <= 1e-12 * max(1.0, abs(expect))
        assert abs(Mm[0, 0] - (J + m * scale * scale)) <= 1e-12 * Mm[0, 0]


def test_planar_cart_pole_closed_form():
    """Cart on a prismatic joint along x, pole of length l with a mass mp of moment I at its tip, angle th from +x,
    gravity as base acceleration +y: M = [[J0 + mc + mp, -mp l sin th], [-mp l sin th, J1 + I + mp l^2]] and the bias
    f = (u0 + mp l cos(th) th'^2, u1 - mp g l cos th).  The cart's own moment of inertia does not enter (omega entry 0)."""
    mc, mp, l, J0, J1, I, g = 2.0, 0.7, 0.45, 0.3, 0.05, 0.02, 9.81
    ch = krp.Chain(_chain([pps.P, pps.R], [(1.0, 0.0), None], [0.0, l], [mc, mp], [5.0, I], [J0, J1], (0.0, g)))
    rng = np.random.default_rng(5)
    for _ in range(20):
        xc, xd, th, thd = rng.uniform(-2, 2, size=4)
        u = rng.uniform(-4, 4, size=2)
        pd, M, f = ch.state_derivative([xc, xd, th, thd], u)
        Me = np.array([[J0 + mc + mp, -mp * l * math.sin(th)], [-mp * l * math.sin(th), J1 + I + mp * l * l]])
        fe = np.array([u[0] + mp * l * math.cos(th) * thd * thd, u[1] - mp * g * l * math.cos(th)])
        assert _rel(M, Me) <= 1e-12 and _rel(f, fe) <= 1e-12
        assert _rel(pd[1::2], np.linalg.solve(Me, fe)) <= 1e-12 and np.array_equal(pd[0::2], [xd, thd])


def test_prismatic_joint_passes_torque_to_the_revolute_joint_below():
    """R then P (unit axis), at rest under gravity with the prismatic joint held by u_1 = -(F . a): the weight of the carried
    mass acts at p = R(th) (d0 + q a), and its moment about the revolute joint, -m g p_x, reaches that joint's coordinate
    only through the torque (q a) % F the prismatic joint hands to its base (without it the arm would be d0 alone)."""
    m, g, d0, a = 1.5, 9.81, 0.4, (0.6, 0.8)
    ch = krp.Chain(_chain([pps.R, pps.P], [None, a], [d0, 0.0], [0.0, m], [0.0, 0.0], [0.1, 0.1], (0.0, g), base_angle=0.0))
    for th, q in [(0.3, 0.5), (-1.1, 0.9), (2.0, -0.4)]:
        ay = math.sin(th) * a[0] + math.cos(th) * a[1]  # the axis in the world: F . a = -m g ay
        _, _, f = ch.state_derivative([th, 0.0, q, 0.0], [0.0, m * g * ay])
        px = math.cos(th) * (d0 + q * a[0]) - math.sin(th) * (q * a[1])
        assert abs(f[0] - (-m * g * px)) <= 1e-12 * max(1.0, abs(m * g * px))
        assert abs(-m * g * px - (-m * g * math.cos(th) * d0)) > 1e-2  # the passed torque is what makes the difference
        assert abs(f[1]) <= 1e-12 * m * g  # held


# ------------------------------------------------------------------------ 3. against kte_ref on the 3D twin
@pytest.mark.parametrize("make", [pps.lone_p, pps.p_r, pps.r_p, pps.seven,
                                  lambda: scenarios.make_crs_a465_2d(dynamics=True)])
def test_restatement_matches_kte_ref_on_the_3d_twin(make):
    """M to 1e-13 and accelerations to 1e-11 (the bars of DESIGN.md section 2's 2D / 3D pin) between the planar
    restatement and tests/kte_ref.py on the twin: z-axis revolute joints, prismatic_joint_3D along (a_x, a_y, 0)."""
    scn = make()
    ch2, ch3 = krp.Chain(scn), kte_ref.Chain(pps.twin_3d(scn))
    rng = np.random.default_rng(17 + scn.n_dof)
    for _ in range(12):
        x = rng.uniform(-1.2, 1.2, size=scn.D)
        u = rng.uniform(-10, 10, size=scn.n_dof)
        p2, M2, f2 = ch2.state_derivative(x, u)
        p3, M3, f3 = ch3.state_derivative(x, u)
        assert _rel(M2, M3) <= 1e-13 and _rel(p2, p3) <= 1e-11 and _rel(f2, f3) <= 1e-11


def test_crs_a465_2d_follows_the_reference_model():
    """The chain, bounds and limits of CRS_A465_2D_analog.cpp:139-360, start and goal at opposite ends of the track, and
    a rate-limited rkh_qs_space."""
    scn = scenarios.make_crs_a465_2d(world_seed=1, n_obstacles=8)
    kinds = [o.kind for o in scn.ops]
    assert kinds == [T.KTE_PRISMATIC_JOINT_2D, T.KTE_RIGID_LINK_2D] + [T.KTE_REVOLUTE_JOINT_2D, T.KTE_RIGID_LINK_2D] * 3
    assert tuple(scn.ops[0].axis) == (1.0, 0.0, 0.0)
    assert [scn.ops[2 * j + 1].offset.pos[0] for j in range(4)] == [0.0, 0.3048, 0.3302, 0.0762]
    sp = scn.meta["speed_limits"]
    assert list(sp) == [0.8, 3.14159265359, 3.14159265359, 3.01941960595]
    qs = scn.meta["qs"]
    assert qs.n_dof == 4 and [qs.speed_limits[i] for i in range(4)] == list(sp)
    assert qs.lower[0] == 0.0 and qs.upper[0] == 3.0 / 0.8 and qs.upper[1] == 3.05432619099 / 3.14159265359
    assert (scn.goal[0] - scn.start[0]) * sp[0] > 2.0
    assert sum(1 for s in scn.shapes if s.anchor < 0) == 8
    d = scenarios.make_crs_a465_2d(dynamics=True)
    assert len(d.ops) == 20 and all(o.mass == 1.0 for o in d.ops if o.kind in (T.KTE_INERTIA_GEN, T.KTE_INERTIA_2D))
    assert d.dyn.upper[1] == 0.8 and len(d.start) == 8
    ch = krp.Chain(scn)
    x = np.zeros(8)
    x[0::2] = scn.meta["q_start"]
    assert krp.Distances(ch, oracle_lib).is_free(x)


def test_planar_chain_ops_default_kinds_are_unchanged():
    """The optional per-joint kind and axis default to revolute: an existing scenario's ops are the same bytes."""
    a = scenarios.planar_chain_ops([0.5, 0.5, 0.3], dynamics=True, masses=[3.0, 2.0, 1.0], moments=[0.06, 0.04, 0.01],
                                   joint_inertias=[0.05, 0.04, 0.02])
    b = scenarios.planar_chain_ops([0.5, 0.5, 0.3], dynamics=True, masses=[3.0, 2.0, 1.0], moments=[0.06, 0.04, 0.01],
                                   joint_inertias=[0.05, 0.04, 0.02], kinds=[pps.R] * 3, axes=[None] * 3)
    scn = scenarios.make_c1_planar(dynamics=True)
    assert bytes(T.as_array(a, T.KteOp)) == bytes(T.as_array(b, T.KteOp)) == bytes(scn.ops_array())


# ------------------------------------------------------------------------ 4. resources
@pytest.fixture(scope="module")
def res():
    import kernel_resources as kr

    from reak_amd import lib

    lib.build()
    return kr.kernel_resources()


def _table():
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "r03_kernel_resources.txt")):
        if line.startswith("#") or line.startswith("kernel") or not line.strip():
            continue
        rows[line[:78].strip()] = [int(v) for v in line[78:].split()]
    return rows


@pytest.mark.parametrize("n", [1, 2, 3, 4, 6, 7])
def test_planar_prismatic_instantiations_exist_and_match_the_table(res, n):
    """rkh::planar_prismatic holds the steer, f-eval, distance and edge-walk forms for every chain length their launchers
    dispatch; the committed table has their rows; and for N <= 6 none spills or has a private segment where the revolute
    form of the same N does not."""
    pairs = [(f"rkh::planar_prismatic::planar_propagate_kernel<{n}>", f"rkh::planar_propagate_kernel<{n}>"),
             (f"rkh::planar_prismatic::planar_state_derivative_kernel<{n}>", f"rkh::planar_state_derivative_kernel<{n}>"),
             (f"rkh::planar_prismatic::min_distance_kernel<{n}>", f"rkh::min_distance_kernel<{n}>")]
    pairs += [(f"rkh::planar_prismatic::edge_check_kernel<{n}, {w}>", f"rkh::edge_check_kernel<{n}, {w}>") for w in (1, 2, 4, 8)]
    rows = _table()
    for k, rev in pairs:
        d, r = res[k], res[rev]
        got = [d["vgpr_count"], d["agpr_count"], d["vgpr_spill_count"], d["sgpr_count"], d["private_segment_fixed_size"],
               d["group_segment_fixed_size"]]
        assert rows[k[:78]][:6] == got, (k, rows[k[:78]], got)
        if n <= 6:
            assert d["vgpr_spill_count"] == 0 or r["vgpr_spill_count"] != 0, (k, d, r)
            assert d["private_segment_fixed_size"] == 0 or r["private_segment_fixed_size"] != 0, (k, d, r)


def test_planar_prismatic_namespace_holds_nothing_else(res):
    heads = ("planar_propagate_kernel<", "planar_state_derivative_kernel<", "min_distance_kernel<", "edge_check_kernel<")
    names = [k for k in res if k.startswith("rkh::planar_prismatic::")]
    assert len(names) == 6 * 3 + 6 * 4
    assert all(k[len("rkh::planar_prismatic::"):].startswith(heads) for k in names)
