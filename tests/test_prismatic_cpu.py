"""Prismatic joints in 3D chains, CPU side: the test-side restatement (tests/kte_ref.py) pinned against the oracle on
revolute chains and against closed forms on prismatic ones, the CRS A465 track scene through `.rkx`, and the resources of
the prismatic kernel instantiations.  No GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kte_ref  # noqa: E402
import oracle_lib  # noqa: E402
from reak_amd import rkx, scenarios  # noqa: E402
from reak_amd import types as T  # noqa: E402


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


@pytest.mark.parametrize("make", [lambda: scenarios.make_c2(world_seed=2)] +
                         [lambda n=n: scenarios.make_random_chain(n, seed=3) for n in (1, 2, 3, 4, 6, 7)])
def test_restatement_matches_the_oracle_on_revolute_chains(make):
    """Before the restatement is trusted on prismatic chains: on revolute chains it gives the oracle's pd, M, f and link
    frames (to 1e-12 relative; in practice the same bits)."""
    scn = make()
    osc, ch = oracle_lib.OracleScene(scn), kte_ref.Chain(scn)
    rng = np.random.default_rng(11 + scn.n_dof)
    x = rng.uniform(-1.5, 1.5, size=(16, scn.D))
    u = rng.uniform(-10, 10, size=(16, scn.n_dof))
    rc, pd, M, f = osc.state_derivative(x, u)
    assert rc == 0
    fk = osc.fk(x)
    for i in range(len(x)):
        p2, M2, f2 = ch.state_derivative(x[i], u[i])
        assert _rel(p2, pd[i]) <= 1e-12 and _rel(M2, M[i]) <= 1e-12 and _rel(f2, f[i]) <= 1e-12
        assert _rel(ch.frames(x[i]), fk[i]) <= 1e-12


def _track_only(axis, link_mass, rotor, gravity=(0.0, 0.0, 9.81)):
    ops = scenarios.serial_chain_ops([axis], [(0.0, 0.0, 0.2)], [link_mass], [(0.3, 0, 0, 0.2, 0, 0.1)], [rotor],
                                     [T.KTE_PRISMATIC_JOINT_3D])
    base = T.ChainBase()
    base.pose = T.make_pose((0.1, 0.2, 0.3), (math.cos(0.3), 0.0, 0.0, math.sin(0.3)))
    base.acceleration[:] = list(gravity)
    return scenarios.Scenario(name="track", ops=ops, base=base, shapes=[], dyn=T.DynSpace(), n_dof=1, n_frames=3,
                              start=np.zeros(2), goal=np.zeros(2))


@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_lone_track_joint_closed_form(scale):
    """A prismatic joint whose axis lies along the base acceleration (gravity) carrying a link of mass M on a rotor of
    inertia m_r: q'' = (u - M (g . a)) / (M |a|^2 + m_r).  The axis is used as given (scale 2.5: not normalised)."""
    M, m_r, g = 3.0, 1.0, 9.81
    a = (0.0, 0.0, scale)
    ch = kte_ref.Chain(_track_only(a, M, m_r, (0.0, 0.0, g)))
    for q, qd, u in [(0.0, 0.0, 0.0), (0.7, -1.3, 12.0), (-2.0, 0.4, -5.0)]:
        pd, Mm, f = ch.state_derivative([q, qd], [u])
        expect = (u - M * (g * scale)) / (M * scale * scale + m_r)
        assert abs(pd[0] - qd) == 0.0
        assert abs(pd[1] - expect) <= 1e-12 * max(1.0, abs(expect))
        assert abs(Mm[0, 0] - (M * scale * scale + m_r)) <= 1e-12 * Mm[0, 0]


def _cart_pole(mc, m, l, j0, j1, g):
    """Cart on a prismatic joint along base x, pole on a revolute joint about +y with a point mass m at distance l
    along the pole's local z.  Angle convention: theta = 0 upright, positive tips the mass toward +x
    (tip = (x + l sin(theta), 0, l cos(theta)))."""
    ops = scenarios.serial_chain_ops([(1.0, 0.0, 0.0), (0.0, 1.0, 0.0)], [(0.0, 0.0, 0.0), (0.0, 0.0, l)], [mc, m],
                                     [(0, 0, 0, 0, 0, 0)] * 2, [j0, j1],
                                     [T.KTE_PRISMATIC_JOINT_3D, T.KTE_REVOLUTE_JOINT_3D])
    base = T.ChainBase()
    base.pose = T.make_pose()
    base.acceleration[:] = [0.0, 0.0, g]
    return scenarios.Scenario(name="cart_pole", ops=ops, base=base, shapes=[], dyn=T.DynSpace(), n_dof=2, n_frames=5,
                              start=np.zeros(4), goal=np.zeros(4))


def test_cart_pole_closed_form():
    """Cart-pole (P then R): M(q) = [[mc + m + j0, m l cos(th)], [m l cos(th), m l^2 + j1]] and the bias forces
    f = (u_x + m l sin(th) th'^2, u_th + m g l sin(th)) with gravity g entering as base acceleration +z."""
    mc, m, l, j0, j1, g = 2.0, 0.7, 0.45, 0.3, 0.05, 9.81
    ch = kte_ref.Chain(_cart_pole(mc, m, l, j0, j1, g))
    rng = np.random.default_rng(5)
    for _ in range(20):
        x_c, xd, th, thd = rng.uniform(-2, 2, size=4)
        u = rng.uniform(-4, 4, size=2)
        pd, M, f = ch.state_derivative([x_c, xd, th, thd], u)
        Me = np.array([[mc + m + j0, m * l * math.cos(th)], [m * l * math.cos(th), m * l * l + j1]])
        fe = np.array([u[0] + m * l * math.sin(th) * thd * thd, u[1] + m * g * l * math.sin(th)])
        assert _rel(M, Me) <= 1e-12 and _rel(f, fe) <= 1e-12
        qdd = np.linalg.solve(Me, fe)
        assert _rel(pd[1::2], qdd) <= 1e-12 and np.array_equal(pd[0::2], [xd, thd])


def test_restatement_prismatic_frames_follow_the_axis():
    """doMotion of the track scene: the end frame of the track joint is the base moved by R(base) (q a), same
    orientation; link_0 (identity offset) coincides with it."""
    scn = scenarios.make_crs_a465_track()
    ch = kte_ref.Chain(scn)
    x = np.zeros(scn.D)
    x[0] = 1.25
    fr = ch.frames(x)
    assert np.allclose(fr[1][:3], [0.0, -3.3 + 1.25, 0.3], rtol=0, atol=1e-15)  # base x axis = global +y
    assert np.array_equal(fr[1][3:], fr[0][3:]) and np.array_equal(fr[2], fr[1])


def test_crs_a465_track_rkx_round_trip_is_bit_identical():
    """make_crs_a465_track() -> .rkx -> scene: the same bits (ops with the prismatic op, base, shapes, start, goal)."""
    scn = scenarios.make_crs_a465_track()
    text = rkx.write_scene(scn)
    back = rkx.read_scene(text, scn)
    robot_then_env = [s for s in scn.shapes if s.anchor >= 0] + [s for s in scn.shapes if s.anchor < 0]
    assert bytes(scn.ops_array()) == bytes(back.ops_array()) and bytes(scn.base) == bytes(back.base)
    assert bytes(T.as_array(robot_then_env, T.Shape)) == bytes(back.shapes_array())
    assert np.array_equal(scn.start, back.start) and np.array_equal(scn.goal, back.goal)
    assert back.n_dof == 7 and back.n_frames == scn.n_frames
    assert rkx.write_scene(back) == text


def test_prismatic_element_lists_its_fields_in_save_order():
    """prismatic_joint_3D (type id 0xC2100006, version 1) writes named_object's name, then mCoord, mAxis, mBase, mEnd,
    mJacobian (prismatic_joint.hpp:157-163)."""
    text = rkx.write_scene(scenarios.make_crs_a465_track())
    lines = text.splitlines()
    # the joint's body is written where the object first appears (inside the actuator's mJoint)
    at = next(i for i, ln in enumerate(lines) if 'type_ID="3255828486.0" version="1" object_ID=' in ln)
    indent = len(lines[at]) - len(lines[at].lstrip())
    fields = []
    for ln in lines[at + 1:]:
        ind = len(ln) - len(ln.lstrip())
        if ind == indent:
            break
        if ind == indent + 4 and not ln.lstrip().startswith("</"):
            fields.append(re.match(r"<(\w+)", ln.lstrip()).group(1))
    assert fields == ["name", "mCoord", "mAxis", "mBase", "mEnd", "mJacobian"]
    assert text.count('type_ID="3255828486.0"') == 2  # written once, referred to once (the actuator's mJoint, mKTEs)


def test_serial_chain_ops_default_kinds_are_unchanged():
    """The optional per-joint kind defaults to revolute: the ops of an existing scenario are the same bytes either way."""
    scn = scenarios.make_c2(world_seed=1)
    axes, _, offsets, masses, inertias, jin = scenarios.crs_like_chain()
    a = scenarios.serial_chain_ops(axes, offsets, masses, inertias, jin)
    b = scenarios.serial_chain_ops(axes, offsets, masses, inertias, jin, [T.KTE_REVOLUTE_JOINT_3D] * 6)
    assert bytes(T.as_array(a, T.KteOp)) == bytes(T.as_array(b, T.KteOp)) == bytes(scn.ops_array())


@pytest.fixture(scope="module")
def res():
    import kernel_resources as kr

    from reak_amd import lib

    lib.build()
    return kr.kernel_resources()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 6, 7])
def test_prismatic_instantiations_exist_without_spill_or_scratch(res, n):
    """The prismatic forms (rkh::prismatic, propagate_prismatic.hip) of the one-wave steer, f-eval, distance and 3D
    edge-walk kernels are built for every chain length their launchers dispatch, without spilled registers and without a
    private segment."""
    names = [f"rkh::prismatic::propagate_kernel<{n}, 64, false, false>", f"rkh::prismatic::state_derivative_kernel<{n}>",
             f"rkh::prismatic::min_distance_kernel<{n}>", f"rkh::prismatic::edge_points_kernel<{n}, false, 32>",
             f"rkh::prismatic::edge_points_kernel<{n}, false, 64>"]
    for k in names:
        d = res[k]
        assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (k, d)
    assert not [k for k in res if k.startswith("rkh::prismatic::") and not any(k.startswith(p.split("<")[0]) for p in names)]
