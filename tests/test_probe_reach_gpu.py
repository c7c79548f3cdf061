"""Goal probes that cannot reach the goal are settled when their vertex is committed (reak_amd/csrc/probe_reach.h); the
others wait in a per-problem list that the steer launches read (round_plan.h: the granule rule).  RKH_PROBE_REACH=0 at
create turns the certificate off: every probe is steered, as before.  Nothing a planner returns may depend on the switch.

Sizes: three C2 problems of 300 vertices and one of 120 with RKH_BATCH_MIN=1 (tests/test_step_edge_io_gpu.py: they reach
the step-wise launches with carry).  The three problems differ in their goal, chosen on the CPU with the oracle:
  far     the scenario's goal: every vertex is certified
  near    a state the PD law reaches from a vertex of the tree: that probe's result is finite, it registers a solution,
          and every vertex lies inside reach_q + 0.05 n_ab -- the list holds all of them
  mixed   a goal about reach_q away from the root: some vertices are certified and some are not, so the list is a
          proper subsequence of the vertices
No certificate exists for a chain with a prismatic joint, for C2 with a tether, for a planar dynamic scene and for the
quasi-static space: nothing is certified there and every vertex goes through the list."""
import contextlib
import os

import numpy as np
import pytest

from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

STATE_RTOL = 1e-10  # test_gpu_parity.py::test_propagate_c2_matches_oracle
_KNOBS = ("RKH_LANES_PER_EDGE", "RKH_LANE_THRESHOLD", "RKH_STEER_SPLIT_MIN_EDGES", "RKH_STEER_CARRY_MIN_EDGES",
          "RKH_STEER_CARRY", "RKH_WAVE_FIT", "RKH_BATCH_FACTOR", "RKH_BATCH_MAX", "RKH_BATCH_MIN", "RKH_PROBE_REACH",
          "RKH_PROBE_REACH_MIN_EDGES")
_MAPPINGS = {
    "wave": {"RKH_LANES_PER_EDGE": "64"},
    "pair": {"RKH_LANES_PER_EDGE": "2"},
    "auto": {"RKH_LANES_PER_EDGE": "0", "RKH_LANE_THRESHOLD": "1", "RKH_STEER_SPLIT_MIN_EDGES": "0", "RKH_STEER_CARRY": "0"},
    # every round step-wise and carrying (round_carry.h): reused edges are not steered again, so its executed steps are
    # fewer than the other mappings' by design and are compared on against off only
    "auto_carry": {"RKH_LANES_PER_EDGE": "0", "RKH_LANE_THRESHOLD": "1", "RKH_STEER_SPLIT_MIN_EDGES": "0",
                   "RKH_STEER_CARRY_MIN_EDGES": "0"},
}
# Probes are settled only in rounds of at least RKH_PROBE_REACH_MIN_EDGES edges (default: what fills the chip, like the
# round carry); these trees are small, so the tests take the threshold away -- except the one that is about it.
_SMALL = {"RKH_BATCH_MIN": "1", "RKH_PROBE_REACH_MIN_EDGES": "0"}
_OFF = {"RKH_PROBE_REACH": "0"}
C2_REACH = 0.6087  # |T|_2 of C2 (tests/test_probe_reach_cpu.py prints it); the library's value is compared with it below


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


def _with_goal(scn, goal, **kw):
    prm = scn.rrt_params(**kw)
    for d in range(scn.D):
        prm.goal[d] = float(goal[d])
    return prm


@pytest.fixture(scope="module")
def c2_case(oracle):
    """C2, its three problems (far, near, mixed) and one small problem with the near goal; the oracle's trees of all four,
    and what the CPU says about the goals."""
    scn = scenarios.make_c2(world_seed=1)
    osc = oracle.OracleScene(scn)
    far = np.asarray(scn.goal, dtype=np.float64)

    def near_goal(seed, max_vertices, vertex):
        # a state the PD law passes within goal_tol: the fixed point of g -> state after 10 steps of steer(vertex, g)
        rc, _, t = osc.rrt_dyn(scn.rrt_params(seed=seed, max_vertices=max_vertices))
        assert rc == 0
        a = t["pos"][vertex]
        rc, _, _, rec = osc.steer(a, far, record=True)
        g = rec[0, 10].copy()
        for _ in range(30):
            rc, _, steps, rec = osc.steer(a, g, record=True)
            assert rc == 0
            g = rec[0, min(10, int(steps[0]))].copy()
        return g, t

    near, tree2 = near_goal(2, 300, 200)
    near_small, _ = near_goal(5, 120, 60)
    # about reach_q from the root, towards where the third problem's tree spreads most
    rc, _, tree3 = osc.rrt_dyn(scn.rrt_params(seed=3, max_vertices=300))
    q = tree3["pos"][:, 0::2]
    _, _, vt = np.linalg.svd(q - q.mean(axis=0), full_matrices=False)
    mixed = np.zeros(scn.D)
    mixed[0::2] = q[0] + 0.68 * vt[0]
    prms = [_with_goal(scn, far, seed=1, max_vertices=300), _with_goal(scn, near, seed=2, max_vertices=300),
            _with_goal(scn, mixed, seed=3, max_vertices=300)]
    small = [_with_goal(scn, near_small, seed=5, max_vertices=120)]
    case = {"scn": scn, "osc": osc, "prms": prms, "small": small, "oracle": [], "oracle_small": []}
    for key, ps in (("oracle", prms), ("oracle_small", small)):
        for prm in ps:
            rc, rout, rtree = osc.rrt_dyn(prm)
            assert rc == 0
            case[key].append((rout, rtree))
    # what the test is about, asserted on the CPU: finite results, vertices inside and outside the reach
    inside = []
    for prm, (rout, rtree) in zip(prms + small, case["oracle"] + case["oracle_small"]):
        g = np.array([prm.goal[d] for d in range(scn.D)])
        pos = rtree["pos"][1:]
        n_ab = np.linalg.norm(pos - g, axis=1)
        dq = np.linalg.norm(pos[:, 0::2] - g[0::2], axis=1)
        inside.append(int((dq - C2_REACH < 0.05 * n_ab).sum()))
    finite = [int(np.isfinite(rtree["goal_dist"]).sum()) for _, rtree in case["oracle"] + case["oracle_small"]]
    print("vertices inside the reach per problem", inside, "finite goal distances", finite)
    assert inside[0] == 0 and inside[1] == 300 and 0 < inside[2] < 300 and inside[3] == 120
    assert finite[0] == 0 and finite[1] >= 1 and finite[3] >= 1
    assert case["oracle"][1][0].num_solutions >= 1 and case["oracle_small"][0][0].num_solutions >= 1
    return case


def _plan(L, ctx, scn, prms, env, qs=None, rounds_per_sync=None):
    with _environment(env):
        sc = L.Scene(ctx, scn)
        pl = L.RrtPlanner(sc, prms, qs=qs)
        run = {"mapping": L.steer_mapping_name(), "probed": []}
        if rounds_per_sync is None:
            pl.solve_planning_query()
        else:
            for _ in range(100000):
                pl.enqueue(rounds_per_sync)
                pl.sync()
                run["probed"].append([pl.probe_counts(i) for i in range(len(prms))])
                if pl.done:
                    break
        run["stats"] = [(int(s.num_vertices), int(s.iterations), int(s.edges_checked), int(s.num_solutions),
                         float(s.best_cost)) for s in pl.all_stats]
        run["trees"] = [pl.tree(i) for i in range(len(prms))]
        run["solutions"] = [tuple(pl.solution(i)[0].tolist()) + (pl.solution(i)[1],) for i in range(len(prms))]
        run["steps"] = pl.steer_steps() if qs is None else 0
        run["probes"] = [pl.probe_counts(i) for i in range(len(prms))]
        pl.close()
        sc.close()
    return run


def _same_plan(a, b, what):
    assert a["stats"] == b["stats"], what
    assert a["solutions"] == b["solutions"], what
    for i, (ta, tb) in enumerate(zip(a["trees"], b["trees"])):
        for key in ("pos", "parent", "nn_seq", "accept", "goal_dist"):
            assert np.array_equal(ta[key], tb[key]), (what, i, key)


def _probe_balance(run, what):
    """every vertex but the root got its result exactly once: settled at commit or run by a launch; nothing is left open"""
    for stats, pc in zip(run["stats"], run["probes"]):
        assert pc["certified"] + pc["run"] == stats[0] - 1, (what, pc, stats)
        assert pc["open"] == 0 and pc["probed_n"] == stats[0] == pc["first_open"], (what, pc, stats)


_RUNS = {}


def _c2_run(L, ctx, case, which, mapping, on):
    key = (which, mapping, on)
    if key not in _RUNS:
        prms, knobs = (case["prms"], _SMALL) if which == "three" else (case["small"], dict(_SMALL, RKH_BATCH_FACTOR="0.7"))
        # (without the wave fit every mapping sees the same rounds, so the step counters compare; the granule is then 1)
        env = dict(_MAPPINGS[mapping], RKH_WAVE_FIT="0", **knobs, **({} if on else _OFF))
        _RUNS[key] = _plan(L, ctx, case["scn"], prms, env)
        assert _RUNS[key]["mapping"] == mapping.split("_")[0]
    return _RUNS[key]


@pytest.mark.parametrize("which", ["three", "one"])
@pytest.mark.parametrize("mapping", sorted(_MAPPINGS))
def test_results_do_not_depend_on_the_certificate(L, ctx, c2_case, mapping, which):
    """Filter on against RKH_PROBE_REACH=0: stats, states, parents, NN sequences, accept bytes, goal distances and
    solutions are identical; certified + run = vertices - 1 per problem; the far problem runs no probe, the near one
    every probe, the mixed one some; fewer steps are executed with the filter on."""
    on = _c2_run(L, ctx, c2_case, which, mapping, True)
    off = _c2_run(L, ctx, c2_case, which, mapping, False)
    _same_plan(on, off, (mapping, which))
    _probe_balance(on, "on")
    _probe_balance(off, "off")
    print(mapping, which, "probes on", [(p["certified"], p["run"]) for p in on["probes"]], "steps on / off", on["steps"], off["steps"])
    assert all(p["certified"] == 0 and np.isinf(p["reach_q"]) for p in off["probes"])
    assert all(abs(p["reach_q"] - C2_REACH) < 1e-4 for p in on["probes"])
    if which == "three":
        far, near, mixed = on["probes"]
        assert far["run"] == 0 and far["certified"] > 0
        assert near["certified"] == 0 and near["run"] > 0
        assert mixed["certified"] > 0 and mixed["run"] > 0
        assert on["steps"] < off["steps"]
    else:
        assert on["probes"][0]["certified"] == 0  # the whole small tree lies inside the reach of its goal
        assert on["steps"] == off["steps"]


@pytest.mark.parametrize("which", ["three", "one"])
def test_executed_steps_are_the_same_in_every_mapping(L, ctx, c2_case, which):
    """wave, whole-edge and step-wise (without carry, as in tests/test_step_edge_io_gpu.py) run the same probes; the
    carrying run gives the same results with fewer steps."""
    runs = {m: _c2_run(L, ctx, c2_case, which, m, True) for m in sorted(_MAPPINGS)}
    _same_plan(runs["auto_carry"], runs["wave"], "step-wise with carry against one wave")
    assert runs["auto_carry"]["probes"] == runs["wave"]["probes"] and runs["auto_carry"]["steps"] <= runs["wave"]["steps"]
    assert runs["auto"]["steps"] == runs["pair"]["steps"] == runs["wave"]["steps"] > 0
    assert runs["auto"]["probes"] == runs["pair"]["probes"] == runs["wave"]["probes"]
    _same_plan(runs["auto"], runs["wave"], "step-wise against one wave")
    _same_plan(runs["pair"], runs["wave"], "whole-edge against one wave")


@pytest.mark.parametrize("which", ["three", "one"])
def test_trees_solutions_and_costs_equal_the_oracle(L, ctx, c2_case, which):
    """The step-wise run with the filter on against the oracle's sequential planner: the tree, which vertices see the
    goal and at what distance, the registered solutions and the best cost."""
    run = _c2_run(L, ctx, c2_case, which, "auto_carry", True)
    for i, (rout, rtree) in enumerate(c2_case["oracle" if which == "three" else "oracle_small"]):
        t, stats = run["trees"][i], run["stats"][i]
        assert stats[:3] == (rout.num_vertices, rout.iterations, rout.edges_checked)
        assert np.array_equal(t["parent"], rtree["parent"]) and np.array_equal(t["accept"], rtree["accept"])
        assert np.array_equal(t["nn_seq"], rtree["nn_seq"])
        assert np.allclose(t["pos"], rtree["pos"], rtol=STATE_RTOL, atol=1e-12)
        assert np.array_equal(np.isfinite(t["goal_dist"]), np.isfinite(rtree["goal_dist"]))
        fin = np.isfinite(rtree["goal_dist"])
        assert np.allclose(t["goal_dist"][fin], rtree["goal_dist"][fin], rtol=STATE_RTOL, atol=0.0)
        assert stats[3] == rout.num_solutions
        if rout.num_solutions:
            assert stats[4] == pytest.approx(rout.best_cost, rel=STATE_RTOL)
        else:
            assert np.isinf(stats[4])
    if which == "three":
        assert run["stats"][1][3] >= 1 and run["stats"][0][3] == 0  # the near problem registers its solution


def test_small_rounds_steer_every_probe_by_default(L, ctx, c2_case):
    """Without RKH_PROBE_REACH_MIN_EDGES the rounds of these small trees lie under the threshold: nothing is certified,
    every probe runs, and the results are those of the run that certifies."""
    env = dict(_MAPPINGS["auto_carry"], RKH_WAVE_FIT="0", RKH_BATCH_MIN="1")
    default = _plan(L, ctx, c2_case["scn"], c2_case["prms"], env)
    _same_plan(default, _c2_run(L, ctx, c2_case, "three", "auto_carry", True), "default threshold against none")
    _probe_balance(default, "default threshold")
    assert all(p["certified"] == 0 and abs(p["reach_q"] - C2_REACH) < 1e-4 for p in default["probes"])
    assert default["steps"] == _c2_run(L, ctx, c2_case, "three", "auto_carry", False)["steps"]


def test_a_sync_after_every_round_gives_the_same(L, ctx, c2_case):
    """rounds_per_sync = 1 against one solve call (16 rounds per sync), with the wave fit on -- the granule is then 32 and
    open probes wait in the list across syncs.  Results are the same, and at no sync has probed_n passed an open vertex."""
    env = dict(_MAPPINGS["auto_carry"], **_SMALL)
    del env["RKH_LANES_PER_EDGE"]  # the planner's own choice (Auto, wave fit on)
    once = _plan(L, ctx, c2_case["scn"], c2_case["prms"], env)
    every = _plan(L, ctx, c2_case["scn"], c2_case["prms"], env, rounds_per_sync=1)
    _same_plan(every, once, "a sync per round against one solve")
    off = _plan(L, ctx, c2_case["scn"], c2_case["prms"], dict(env, **_OFF))
    _same_plan(once, off, "the certificate on against off, granule 32")
    _probe_balance(off, "off, granule 32")
    assert once["steps"] < off["steps"]
    assert every["probes"] == once["probes"]
    _probe_balance(every, "a sync per round")
    waited = 0
    for at_sync in every["probed"]:
        for pc in at_sync:
            assert 1 <= pc["probed_n"] <= pc["first_open"], pc
            waited += pc["open"] > 0
    print("syncs", len(every["probed"]), "problem-syncs with open probes", waited)
    assert waited > 0  # probes did wait in the list across a sync


def _prismatic_chain():
    scn = scenarios.make_random_chain(4, seed=4)
    op = [o for o in scn.ops if o.kind == T.KTE_REVOLUTE_JOINT_3D][0]
    op.kind = T.KTE_PRISMATIC_JOINT_3D
    op.axis[:] = [0.7 * v for v in op.axis]
    scn.dyn.lower[0], scn.dyn.upper[0] = -0.5, 0.5
    return scn


_NO_CERTIFICATE = {
    "prismatic": lambda: (_prismatic_chain(), 300),
    "tether": lambda: (scenarios.make_c2(world_seed=1, tether=(0.4, 1e4, 1e2)), 300),
    "planar": lambda: (scenarios.make_c1_planar(world_seed=1, dynamics=True), 300),
}


@pytest.mark.parametrize("name", sorted(_NO_CERTIFICATE))
def test_scenes_without_a_certificate_steer_every_probe(L, ctx, oracle, name):
    scn, size = _NO_CERTIFICATE[name]()
    prms = [scn.rrt_params(seed=s, max_vertices=size) for s in (1, 2)]
    run = _plan(L, ctx, scn, prms, _SMALL)
    off = _plan(L, ctx, scn, prms, dict(_SMALL, **_OFF))
    _same_plan(run, off, name)
    _probe_balance(run, name)
    assert run["steps"] == off["steps"]
    if name == "prismatic":
        wave = _plan(L, ctx, scn, prms, dict(_SMALL, RKH_LANES_PER_EDGE="64"))
        assert wave["mapping"] == "prismatic"
        _same_plan(run, wave, "the planner's mapping against the one-wave form")
        assert wave["probes"] == run["probes"]
    osc = oracle.OracleScene(scn)
    for i, prm in enumerate(prms):
        pc, t = run["probes"][i], run["trees"][i]
        assert pc["certified"] == 0 and np.isinf(pc["reach_q"]) and pc["run"] == run["stats"][i][0] - 1
        if name == "prismatic":  # (its planner runs are pinned to the one-wave form, as in tests/test_prismatic_pair_gpu.py)
            continue
        rc, rout, rtree = osc.rrt_dyn(prm)
        assert rc == 0 and run["stats"][i][:3] == (rout.num_vertices, rout.iterations, rout.edges_checked)
        assert np.array_equal(t["parent"], rtree["parent"]) and np.array_equal(t["accept"], rtree["accept"])
        assert np.allclose(t["pos"], rtree["pos"], rtol=STATE_RTOL, atol=1e-12)
        assert np.array_equal(np.isfinite(t["goal_dist"]), np.isfinite(rtree["goal_dist"]))


def test_the_quasi_static_space_steers_every_probe(L, ctx, oracle):
    c1 = scenarios.make_c1(world_seed=1)
    lo, hi, mi = c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"]
    prm = c1.rrt_params(seed=1, max_vertices=600)
    run = _plan(L, ctx, c1, [prm], _SMALL, qs=L.make_qs_space(3, lo, hi, mi))
    _probe_balance(run, "quasi-static")
    pc, t = run["probes"][0], run["trees"][0]
    assert pc["certified"] == 0 and np.isinf(pc["reach_q"]) and pc["run"] == 600
    rc, rout, rtree = oracle.OracleScene(c1).rrt_qs(lo, hi, mi, prm)
    assert rc == 0 and run["stats"][0][:4] == (rout.num_vertices, rout.iterations, rout.edges_checked, rout.num_solutions)
    for key in ("pos", "parent", "nn_seq", "accept", "goal_dist"):
        assert np.array_equal(t[key], rtree[key]), key
    assert run["stats"][0][4] == rout.best_cost
