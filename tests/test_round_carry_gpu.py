"""Rounds of the batch RRT planner that reuse the steered edges of the candidates the round before discarded
(reak_amd/csrc/round_carry.h) against the same rounds with RKH_STEER_CARRY=0: results are bit for bit the same, only
steer work is dropped.

The planner carries only in rounds that take the step-wise two-lanes launch with at least RKH_STEER_CARRY_MIN_EDGES
edges, far above what a test can afford by default; RKH_LANE_THRESHOLD=1, RKH_STEER_SPLIT_MIN_EDGES=0 and
RKH_STEER_CARRY_MIN_EDGES=0 send every round there.  Three problems: a round's segment sizes are no multiples of 32, so
the list launch 0 reads ends in a partial wave.  Every configuration runs once (module fixtures)."""
import contextlib
import os

import numpy as np
import pytest

import steer_filter_scenes
from reak_amd import scenarios

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KNOBS = ("RKH_LANE_THRESHOLD", "RKH_STEER_SPLIT_MIN_EDGES", "RKH_STEER_CARRY_MIN_EDGES", "RKH_STEER_CARRY",
          "RKH_STEER_CARRY_FIT", "RKH_WAVE_FIT", "RKH_LANES_PER_EDGE", "RKH_BATCH_FACTOR", "RKH_BATCH_MAX", "RKH_BATCH_MIN")
_EVERY_ROUND = {"RKH_LANE_THRESHOLD": "1", "RKH_STEER_SPLIT_MIN_EDGES": "0", "RKH_STEER_CARRY_MIN_EDGES": "0"}


@contextlib.contextmanager
def _environment(env):
    saved = {k: os.environ.pop(k, None) for k in _KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in _KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


def _run(L, ctx, scn, prms, env):
    with _environment(env):
        pl = L.RrtPlanner(L.Scene(ctx, scn), prms)
        mapping = L.steer_mapping_name()
        pl.solve_planning_query()
        run = {"stats": [(int(s.num_vertices), int(s.iterations), int(s.edges_checked), int(s.num_solutions),
                          float(s.best_cost)) for s in pl.all_stats],
               "trees": [pl.tree(i) for i in range(len(prms))], "steps": pl.steer_steps(), "mapping": mapping}
        run["discarded"], run["reused"] = pl.carry_counts()
        pl.close()
    return run


def _same_results(a, b):
    assert a["stats"] == b["stats"]
    for ta, tb in zip(a["trees"], b["trees"]):
        for key in ("parent", "nn_seq", "accept", "pos", "goal_dist"):
            assert np.array_equal(ta[key], tb[key]), key


def _carry_counters(on, off):
    print(f"carry on: discarded {on['discarded']} reused {on['reused']} steps {on['steps']}; "
          f"off: discarded {off['discarded']} reused {off['reused']} steps {off['steps']}")
    assert on["discarded"] > 0
    assert 0.6 * on["discarded"] <= on["reused"] <= on["discarded"]
    assert off["reused"] == 0
    assert on["steps"] < off["steps"]


@pytest.fixture(scope="module")
def c2_runs(L, ctx):
    """world_seed = 1, seeds 1..3, 1 500 vertices: the runs of tests/golden/c2_golden.npz (tests/make_golden.py)."""
    c2 = scenarios.make_c2(world_seed=1)
    prms = [c2.rrt_params(seed=s, max_vertices=1500) for s in (1, 2, 3)]
    runs = {}
    for fit in ("0", None):
        base = dict(_EVERY_ROUND) if fit is None else dict(_EVERY_ROUND, RKH_WAVE_FIT=fit)
        runs[("on", fit)] = _run(L, ctx, c2, prms, base)
        runs[("off", fit)] = _run(L, ctx, c2, prms, dict(base, RKH_STEER_CARRY="0"))
    default_gate = {k: v for k, v in _EVERY_ROUND.items() if k != "RKH_STEER_CARRY_MIN_EDGES"}
    runs["default gate"] = _run(L, ctx, c2, prms, default_gate)
    return runs


@pytest.mark.parametrize("fit", ["0", None], ids=["wave fit off", "wave fit on"])
def test_c2_rounds_that_carry_give_the_same_trees_with_fewer_steps(c2_runs, fit):
    on, off = c2_runs[("on", fit)], c2_runs[("off", fit)]
    assert on["mapping"] == off["mapping"] == "auto"
    _same_results(on, off)
    # the sequential planner's run of problem 0 (seed 1), recorded from the oracle
    g = np.load(os.path.join(ROOT, "tests", "golden", "c2_golden.npz"))
    t = on["trees"][0]
    assert on["stats"][0][:4] == tuple(int(v) for v in g["rrt1_counts"])
    for key in ("nn_seq", "accept", "parent"):
        assert np.array_equal(t[key], g["rrt1_" + key]), key
    # 3 problems run at batch factor 4, where the round simulation finds 0.88 of the discarded candidates reusable
    # (tests/test_round_carry_cpu.py); 0.6 leaves room for the surplus a smaller next batch drops
    _carry_counters(on, off)


def test_prismatic_chain_rounds_that_carry_give_the_same_trees_with_fewer_steps(L, ctx):
    scn = steer_filter_scenes.prismatic_chain6()
    prms = [scn.rrt_params(seed=s, max_vertices=1000) for s in (1, 2, 3)]
    env = dict(_EVERY_ROUND, RKH_LANES_PER_EDGE="0")
    on = _run(L, ctx, scn, prms, env)
    off = _run(L, ctx, scn, prms, dict(env, RKH_STEER_CARRY="0"))
    assert on["mapping"] == off["mapping"] == "auto"
    _same_results(on, off)
    _carry_counters(on, off)


def test_default_gate_keeps_small_rounds_out(c2_runs):
    """Without RKH_STEER_CARRY_MIN_EDGES the rounds of this size reuse nothing and execute the steps of the switched-off
    run: the executed-step counter stays equal across the steer mappings on such rounds."""
    run, off = c2_runs["default gate"], c2_runs[("off", None)]
    _same_results(run, off)
    assert run["reused"] == 0
    assert run["steps"] == off["steps"]
