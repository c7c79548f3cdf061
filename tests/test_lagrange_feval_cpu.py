"""The f-eval's CPU statements against the energy reference (tests/lagrange_ref.py), which propagates no forces: the
oracle, tests/kte_ref.py and tests/kte_ref_planar.py must satisfy  G f = u - c - dV/dq,  q'' = M^-1 f  on every state of
every case family, to the derived bounds of lagrange_ref.bounds (1e-12 relative; DESIGN.md "The f-eval is not the
Lagrangian field").  Reference values come from tests/golden/lagrange_feval.npz; every fourth state is also recomputed
live and must reproduce the file's doubles exactly, and the twins are held to those live values too.  No GPU."""
import functools
import math
import os

import numpy as np
import pytest

import kte_ref
import kte_ref_planar
import lagrange_ref as LR
import planar_prismatic_scenes as pps
from reak_amd import scenarios
from reak_amd import types as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lagrange_feval.npz")
LIVE_ROWS = list(range(0, LR.N_STATES, 4))
REVOLUTE_3D = [n for n in LR.SPATIAL_FAMILIES if n != "track" and not n.startswith("mixed")]


@functools.lru_cache(maxsize=None)
def golden():
    return LR.load_golden(GOLDEN)


@functools.lru_cache(maxsize=None)
def live(name):
    """Every fourth state of a family, computed now in mpmath (once per session)."""
    return LR.reference_arrays(name, rows=LIVE_ROWS)


def _hold(name, twin, label):
    """twin(x, u) -> (pd, M, f) on every state of the family against the file, and on the live rows against the live
    values; prints and returns the worst error / bound of (M, f, q'')."""
    ref = golden()[name]
    worst = np.zeros(3)
    for src, rows in ((ref, range(LR.N_STATES)), (live(name), range(len(LIVE_ROWS)))):
        for i in rows:
            pd, M, f = twin(src["x"][i], src["u"][i])
            assert np.array_equal(pd[0::2], src["x"][i][1::2])
            r = np.array(LR.ratios(M, f, pd[1::2], src, i))
            worst = np.maximum(worst, r)
            assert np.all(r <= 1.0), (label, name, i, "error / bound of (M, f, q'')", r.tolist())
    print("%s %-18s worst error/bound  M %.3g  f %.3g  q'' %.3g" % (label, name, *worst))
    return worst


def _oracle_twin(oracle, scn):
    osc = oracle.OracleScene(scn)

    def twin(x, u):
        rc, pd, M, f = osc.state_derivative(x, u)
        assert rc == 0
        return pd[0], M[0], f[0]

    return twin


# ------------------------------------------------------------------------ the file
def test_golden_holds_every_state_of_every_family():
    """24 states per family, none skipped, kappa_2(M) <= 1e6, the six edge rows in place, G unit upper triangular."""
    g = golden()
    assert sorted(g) == sorted(LR.FAMILY_NAMES)
    for name in LR.FAMILY_NAMES:
        scn = LR.scene(name)
        x, u = LR.states(name, scn)
        ref, n = g[name], scn.n_dof
        assert np.array_equal(ref["x"], x) and np.array_equal(ref["u"], u) and x.shape == (LR.N_STATES, 2 * n)
        assert ref["kappa"].shape == (LR.N_STATES,) and np.all(ref["kappa"] >= 1.0) and np.all(ref["kappa"] <= LR.KAPPA_MAX)
        q, lo, hi = x[:, 0::2], np.array([scn.dyn.lower[2 * j] for j in range(n)]), np.array([scn.dyn.upper[2 * j] for j in range(n)])
        assert np.all(q >= lo) and np.all(q <= hi) and np.all(np.abs(x[:, 1::2]) <= 2.0) and np.all(np.abs(u) <= 10.0)
        assert np.all(x[0, 1::2] == 0.0) and np.all(u[1] == 0.0) and np.any(q[2] == 0.0) and np.all(q[5] == 0.0)
        top = np.array([hi[j] if p else min(hi[j], np.pi) for j, p in enumerate(LR.is_prismatic(scn))])
        bot = np.array([lo[j] if p else max(lo[j], -np.pi) for j, p in enumerate(LR.is_prismatic(scn))])
        assert np.any(q[3] == top) and np.any(q[4] == bot)
        for G in ref["G"]:
            assert np.array_equal(np.tril(G), np.eye(n))
        for key in ("M", "f", "qdd", "c", "dVdq", "G"):
            assert np.all(np.isfinite(ref[key]))


@pytest.mark.parametrize("name", LR.FAMILY_NAMES)
def test_golden_recomputes_exactly(name):
    """Every fourth state, evaluated now at 50 digits (with the module's own cross-checks: M against the second
    differences of T, the derivatives at half the step), rounds to exactly the doubles in the file."""
    ref, now = golden()[name], live(name)
    for key in LR.GOLDEN_KEYS:
        assert np.array_equal(now[key], ref[key][LIVE_ROWS]), key


def test_reference_refuses_what_it_does_not_model():
    scn = scenarios.make_c2(tether=(0.3, 1e4, 1e2))
    with pytest.raises(AssertionError, match="flexible_beam_3D"):
        LR.Model(scn)
    scn = LR.hand_parallel()
    [o for o in scn.ops if o.kind == T.KTE_REVOLUTE_JOINT_3D][1].axis[:] = [0.0, 0.0, 1.1]
    with pytest.raises(AssertionError, match="unit"):
        LR.Model(scn)


# ------------------------------------------------------------------------ the twins
@pytest.mark.parametrize("name", REVOLUTE_3D)
def test_oracle_satisfies_the_energy_relation(oracle, name):
    _hold(name, _oracle_twin(oracle, LR.scene(name)), "oracle")


@pytest.mark.parametrize("name", LR.SPATIAL_FAMILIES)
def test_kte_ref_satisfies_the_energy_relation(name):
    _hold(name, kte_ref.Chain(LR.scene(name)).state_derivative, "kte_ref")


@pytest.mark.parametrize("name", LR.PLANAR_FAMILIES)
def test_kte_ref_planar_satisfies_the_energy_relation(oracle, name):
    scn = LR.scene(name)
    _hold(name, kte_ref_planar.Chain(scn).state_derivative, "kte_ref_planar")
    if not any(LR.is_prismatic(scn)):   # the oracle's planar f-eval knows revolute_joint_2D only
        _hold(name, _oracle_twin(oracle, scn), "oracle")


# ------------------------------------------------------------------------ the joint rule is not optional
@pytest.mark.parametrize("name", ["c2", "hand_parallel", "hand_antiparallel", "c1_planar", "mixed4_p12"])
def test_plain_lagrange_forces_do_not_describe_the_f_eval(oracle, name):
    """Scenes with two successive axes that are not orthogonal: f is NOT u - c - dV/dq.  The two differ by more than 1e-3
    relative in the file, for the twin, and for a reference whose G is the identity."""
    ref = golden()[name]
    scn = LR.scene(name)
    i = 8
    assert np.abs(np.triu(ref["G"][i], 1)).max() > 0.1
    plain = ref["u"][i] - ref["c"][i] - ref["dVdq"][i]
    scale = np.abs(ref["f"][i]).max()
    assert np.abs(plain - ref["f"][i]).max() > 1e-3 * scale
    chain = (kte_ref_planar if name in LR.PLANAR_FAMILIES else kte_ref).Chain(scn)
    _, _, f = chain.state_derivative(ref["x"][i], ref["u"][i])
    assert np.abs(f - plain).max() > 1e-3 * scale
    if not any(LR.is_prismatic(scn)):
        _, _, f = _oracle_twin(oracle, scn)(ref["x"][i], ref["u"][i])
        assert np.abs(f - plain).max() > 1e-3 * scale
    no_rule = LR.Model(scn, joint_rule=False).evaluate(ref["x"][i], ref["u"][i])
    assert np.array_equal(no_rule.G, np.eye(scn.n_dof)) and np.array_equal(no_rule.M, ref["M"][i])
    assert np.abs(no_rule.f - plain).max() <= 1e-14 * scale
    assert np.abs(no_rule.f - f).max() > 1e-3 * scale
    # without drive (row 1) the field still does work on the chain: dE/dt = q' . (M q'' + c + dV/dq) = q' . (f + c + dV/dq)
    power = ref["x"][1][1::2] @ (ref["f"][1] + ref["c"][1] + ref["dVdq"][1])
    assert np.all(ref["u"][1] == 0.0) and abs(power) > 1e-3 * np.abs(ref["f"][1]).max()


def test_gyro_family_has_only_the_gyroscopic_torque_on_joint_0():
    """hand_gyro, u = 0: no gravity, no offsets, orthogonal axes (G = identity) -- f_0 is w x I w of the last link alone,
    and it is there."""
    ref = golden()["hand_gyro"]
    assert np.all(ref["dVdq"] == 0.0) and np.abs(np.triu(ref["G"], 1)).max() < 1e-15   # (the base quaternion's rounding)
    assert abs(ref["f"][1][0] + ref["c"][1][0]) < 1e-15 and abs(ref["f"][1][0]) > 1e-3
    assert np.abs(ref["f"][0] - ref["u"][0]).max() < 1e-14   # at rest the drive is all there is


# ------------------------------------------------------------------------ closed form
def _two_link(l1, l2, m1, m2, I1, I2, j0, j1, g):
    ops = scenarios.planar_chain_ops([l1, l2], dynamics=True, masses=[m1, m2], moments=[I1, I2], joint_inertias=[j0, j1])
    base = T.ChainBase()
    base.pose = T.make_pose_2d()
    base.acceleration[:] = [0.0, g, 0.0]
    dyn = scenarios.make_c1_planar(dynamics=True).dyn
    dyn.n_dof = 2
    return scenarios.Scenario(name="2R-planar", ops=ops, base=base, shapes=[], dyn=dyn, n_dof=2, n_frames=5,
                              start=np.zeros(4), goal=np.zeros(4))


def test_two_link_planar_bias_forces_closed_form(oracle):
    """Planar 2R arm in the x-y plane, gravity along -y, masses (with moments) at the link ends, rotor inertias.  Textbook:
        tau_0 = u_0 + h (2 q0' q1' + q1'^2) - (m1 + m2) g l1 cos q0 - m2 g l2 cos(q0 + q1)
        tau_1 = u_1 - h q0'^2 - m2 g l2 cos(q0 + q1),         h = m2 l1 l2 sin q1.
    The joint rule: a revolute_joint_2D hands no torque to its base, so  f_1 = tau_1  and  f_0 = tau_0 - tau_1."""
    l1, l2, m1, m2, I1, I2, j0, j1, g = 0.4, 0.3, 2.0, 1.5, 0.03, 0.02, 0.05, 0.04, 9.81
    scn = _two_link(l1, l2, m1, m2, I1, I2, j0, j1, g)
    rng = np.random.default_rng(5)
    x = rng.uniform(-3.0, 3.0, size=(12, 4))
    x[:, 1::2] = rng.uniform(-2.0, 2.0, size=(12, 2))
    u = rng.uniform(-10.0, 10.0, size=(12, 2))
    x[0, 1::2], u[1] = 0.0, 0.0
    model = LR.Model(scn)
    twins = {"oracle": _oracle_twin(oracle, scn), "kte_ref_planar": kte_ref_planar.Chain(scn).state_derivative,
             "kte_ref": kte_ref.Chain(pps.twin_3d(scn)).state_derivative,
             "lagrange_ref": lambda xx, uu: (lambda r: (np.ravel(np.column_stack([xx[1::2], r.qdd])), r.M, r.f))(model.evaluate(xx, uu))}
    rule_matters = 0.0
    for i in range(len(x)):
        q0, w0, q1, w1 = x[i]
        h = m2 * l1 * l2 * math.sin(q1)
        c01 = math.cos(q0 + q1)
        tau0 = u[i][0] + h * (2.0 * w0 * w1 + w1 * w1) - (m1 + m2) * g * l1 * math.cos(q0) - m2 * g * l2 * c01
        tau1 = u[i][1] - h * w0 * w0 - m2 * g * l2 * c01
        f_exp = np.array([tau0 - tau1, tau1])
        m01 = m2 * l2 * l2 + m2 * l1 * l2 * math.cos(q1) + I2
        M_exp = np.array([[(m1 + m2) * l1 * l1 + m2 * l2 * l2 + 2.0 * m2 * l1 * l2 * math.cos(q1) + I1 + I2 + j0, m01],
                          [m01, m2 * l2 * l2 + I2 + j1]])
        scale = abs(u[i]).max() + abs(h) * 8.0 + (m1 + m2) * g * (l1 + l2)
        for label, twin in twins.items():
            pd, M, f = twin(x[i], u[i])
            assert np.abs(M - M_exp).max() <= 1e-12 * np.abs(M_exp).max(), label
            assert np.abs(f - f_exp).max() <= 1e-12 * scale, (label, i, f, f_exp)
            assert np.abs(pd[1::2] - np.linalg.solve(M_exp, f_exp)).max() <= 1e-11 * max(1.0, np.abs(pd).max()), label
        rule_matters = max(rule_matters, abs(tau1) / scale)   # f_0 = tau_0 would be off by this much
    assert rule_matters > 0.1
