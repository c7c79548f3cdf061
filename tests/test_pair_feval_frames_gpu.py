"""The two-lanes f-eval's frame bookkeeping (pair_state_derivative, propagate_pair.hip): a lane keeps, per column slot,
the joint's quaternion and (-p) * rotmat(q) formed where the frame is captured; the newest slot (2r == j) takes rotmat
from the sweep and is the only one that masks a lane; slot 0 keeps its rotation matrix in registers for N = 2 .. 6.  None
of it changes an operation, so the two-lanes mapping must stay bit-identical to the one-wave mapping at every place the
slots are laid out differently:

  N = 1, 2     only the newest-slot variant runs / the newest variant for r = 0 and the older one once
  N = 3, 7     odd chains: lane 1's last slot has no joint, its frame is never captured, the spare axis row is read
  N = 4, 6     even chains (6 is C2, the benchmark's chain; its end states are also held against the oracle)
  prismatic    a prismatic root, a prismatic last joint (odd and even chain): the rkh::prismatic forms of the same text

Edges: 96 (three waves of 32) and the first 80 of them (the last wave ragged), 20 steps; sources with joint coordinates
at exactly 0 and at both position bounds (+-pi for revolute joints) and a few at rest.  rkh_propagate launches the
whole-edge kernel; the step-wise kernel is reached through the batch planner (RKH_STEER_SPLIT_MIN_EDGES=0, as
test_stepwise_and_whole_edge_steer_launches_do_not_change_results sets it), whose trees carry the accept bytes."""
import numpy as np
import pytest

from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

STATE_RTOL = 1e-10  # test_gpu_parity.py::test_propagate_c2_matches_oracle
_SCALE = [0.7, 1.3, 0.9, 1.1, 0.8, 1.2, 1.0]  # prismatic axes are not unit length
_CASES = [(1, ()), (2, ()), (3, ()), (4, ()), (6, ()), (7, ()), (4, (0,)), (3, (2,)), (6, (5,))]


def _case_id(case):
    return "n%d" % case[0] + ("_p" + "".join(map(str, case[1])) if case[1] else "")


def _scene(n, prism):
    if n == 6 and not prism:
        return scenarios.make_c2(world_seed=1)
    scn = scenarios.make_random_chain(n, seed=n)
    for j, op in enumerate([o for o in scn.ops if o.kind == T.KTE_REVOLUTE_JOINT_3D]):
        if j in prism:
            op.kind = T.KTE_PRISMATIC_JOINT_3D
            op.axis[:] = [_SCALE[j] * v for v in op.axis]
            scn.dyn.lower[2 * j], scn.dyn.upper[2 * j] = -0.5, 0.5
    return scn


def _edges(scn, count, free=None):
    """`count` (source, target) pairs of the state box; source rows carry joint coordinates at exactly 0, at the upper and
    at the lower position bound (one joint per row, every joint in turn), and rows at rest.  free: keeps the sources it
    accepts (the oracle's proximity test, where the comparison with the oracle needs free starts)."""
    n, D = scn.n_dof, scn.D
    lo = np.array([scn.dyn.lower[i] for i in range(D)])
    hi = np.array([scn.dyn.upper[i] for i in range(D)])
    rng = np.random.default_rng(500 + 10 * n + D)
    m = 4 * count
    a = rng.uniform(lo, hi, size=(m, D))
    a[:, 1::2] *= 0.6
    for i in range(m):
        j, kind = (i // 5) % n, i % 5
        if kind == 0:
            a[i, 2 * j] = 0.0
        elif kind == 1:
            a[i, 2 * j] = hi[2 * j]
        elif kind == 2:
            a[i, 2 * j] = lo[2 * j]
        elif kind == 3 and (i // 5) % 3 == 0:
            a[i, 1::2] = 0.0
    if free is not None:
        a = a[free(a)]
    assert a.shape[0] >= count
    a = a[:count]
    pos = a[:, 0::2]
    assert (pos == 0.0).any() and (pos == hi[0::2]).any() and (pos == lo[0::2]).any() and (a[:, 1::2] == 0.0).all(axis=1).any()
    return a, rng.uniform(lo, hi, size=(count, D))


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


@pytest.mark.parametrize("case", _CASES, ids=_case_id)
def test_whole_edge_launch_is_bit_identical_to_the_one_wave_mapping(L, ctx, oracle, monkeypatch, case):
    """rkh_propagate with records, 96 and 80 edges: end states, free-step counts and every recorded state of the
    two-lanes mapping equal the one-wave mapping's bit for bit; C2's also agree with the oracle."""
    n, prism = case
    scn = _scene(n, prism)
    osc = oracle.OracleScene(scn) if case == (6, ()) else None
    a, b = _edges(scn, 96, free=(lambda s: osc.min_distance(s) > 0.01) if osc else None)
    sc = L.Scene(ctx, scn)
    for B in (96, 80):
        monkeypatch.setenv("RKH_LANES_PER_EDGE", "64")
        ref = sc.steer_position_toward(a[:B], b[:B], record=True)
        assert L.steer_mapping_name() == ("prismatic" if prism else "wave")
        monkeypatch.setenv("RKH_LANES_PER_EDGE", "2")
        got = sc.steer_position_toward(a[:B], b[:B], record=True)
        assert L.steer_mapping_name() == "pair"
        print(_case_id(case), B, "steps_free", np.bincount(ref[1], minlength=scn.dyn.steps_per_edge + 1).tolist())
        assert np.array_equal(got[1], ref[1]), (B, "steps_free")
        assert np.array_equal(got[0], ref[0]), (B, "end state")
        assert np.array_equal(got[2], ref[2], equal_nan=True), (B, "record")
        assert ref[1].max() == scn.dyn.steps_per_edge  # the f-eval ran on whole edges, not only on their first step
        if osc is not None and B == 96:
            rc, rout, rsteps, _ = osc.steer(a, b)
            assert rc == 0 and np.array_equal(got[1], rsteps)
            assert np.allclose(got[0], rout, rtol=STATE_RTOL, atol=1e-12)
    sc.close()


def _planner_run(L, ctx, scn, prms, monkeypatch, env):
    for k in ("RKH_LANES_PER_EDGE", "RKH_LANE_THRESHOLD", "RKH_STEER_SPLIT_MIN_EDGES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("RKH_WAVE_FIT", "0")  # every mapping sees the same rounds: the executed-step counters compare
    sc = L.Scene(ctx, scn)
    pl = L.RrtPlanner(sc, prms)
    name = L.steer_mapping_name()
    pl.solve_planning_query()
    run = {"mapping": name,
           "stats": [(int(s.num_vertices), int(s.iterations), int(s.edges_checked), int(s.num_solutions), float(s.best_cost))
                     for s in pl.all_stats],
           "trees": [pl.tree(i) for i in range(len(prms))], "steps": pl.steer_steps()}
    pl.close()
    sc.close()
    return run


@pytest.mark.parametrize("case", _CASES, ids=_case_id)
def test_step_wise_launches_are_bit_identical_to_the_one_wave_mapping(L, ctx, monkeypatch, case):
    """Four RRT problems of 500 vertices on the batch planner: one wave per edge on every round, the two-lanes whole-edge
    launch on every round, and Auto with every round from 64 edges on the two-lanes step-wise launches (a problem
    offers at least 8 candidates per round, so all but the first rounds).  Positions, parents, NN sequences, accept
    bytes, goal probes, stats and the executed-step counter are identical."""
    n, prism = case
    scn = _scene(n, prism)
    prms = [scn.rrt_params(seed=s, max_vertices=500) for s in range(1, 5)]
    runs = [_planner_run(L, ctx, scn, prms, monkeypatch, env)
            for env in ({"RKH_LANES_PER_EDGE": "64"}, {"RKH_LANES_PER_EDGE": "2"},
                        {"RKH_LANES_PER_EDGE": "0", "RKH_LANE_THRESHOLD": "64", "RKH_STEER_SPLIT_MIN_EDGES": "0"})]
    assert [r["mapping"] for r in runs] == ["prismatic" if prism else "wave", "pair", "auto"]
    first = runs[0]
    assert first["steps"] > 0 and all(s[0] >= 500 for s in first["stats"])
    for other in runs[1:]:
        assert other["stats"] == first["stats"], other["mapping"]
        for i, (ta, tb) in enumerate(zip(first["trees"], other["trees"])):
            for key in ("pos", "parent", "nn_seq", "accept", "goal_dist"):
                assert np.array_equal(ta[key], tb[key]), (other["mapping"], i, key)
        assert other["steps"] == first["steps"], other["mapping"]
