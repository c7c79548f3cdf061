"""How the two-lanes steer kernels read and write an edge (propagate_pair.hip): the EdgeIO record is resolved in two
levels of independent loads, the state and target rows are read as one batch, the RK4 stage updates load their workspace
slots before they store, the clearance delta takes the step's start angles from the workspace (from the edge's row again
when the step has inner sub-steps), and the finishing edges read their three rows at once.  None of it changes an
operation, so every result stays bit for bit what the one-wave mapping gives, and the step-wise launches give what the
whole-edge launch gives.

  whole-edge kernel   rkh_propagate with RKH_LANES_PER_EDGE=2, at exactly 1, 31, 32, 33 and 65 edges (ragged last waves:
                      idle slots shadow the wave's first edge), with and without record rows
  step kernel         the batch planner with every round on the step-wise launches (RKH_LANE_THRESHOLD=1,
                      RKH_STEER_SPLIT_MIN_EDGES=0).  With RKH_WAVE_FIT=0 and RKH_BATCH_FACTOR=0 the batch rule
                      (round_plan.h) gives every problem exactly RKH_BATCH_MIN candidates in every round: 1, 31, 32, 33
                      and 65, for one and for three problems.  The goal probes of the vertices the round before added
                      ride behind the candidates in the same list, so a chunk mixes a candidates segment (src_idx,
                      d_tgt_off, tgt_stride = D) with a goal-probe segment (d_src_first, tgt_stride = 0): with 31
                      candidates chunk 0 itself, with 32 the chunk after a full one, with 33 and 65 the chunk one over.
                      Further runs follow the default batch rule.  The planner keeps no record rows (only rkh_propagate
                      passes them), so records are compared on the whole-edge kernel only.

NOT covered: launch 0's `first` store (the x_out row of an edge that ends in its first step).  Such an edge is judged
from its source row and never committed, and neither the probe x_out nor the carry stash can be read from Python.

Chains: N = 1, 2, 3, 6 (C2, also against the oracle), 7, and N = 4 with a prismatic root (the rkh::prismatic forms)."""
import contextlib
import os

import numpy as np
import pytest

from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

STATE_RTOL = 1e-10  # test_gpu_parity.py::test_propagate_c2_matches_oracle
_CASES = [(1, ()), (2, ()), (3, ()), (6, ()), (7, ()), (4, (0,))]
_COUNTS = (1, 31, 32, 33, 65)
_KNOBS = ("RKH_LANES_PER_EDGE", "RKH_LANE_THRESHOLD", "RKH_STEER_SPLIT_MIN_EDGES", "RKH_STEER_CARRY_MIN_EDGES",
          "RKH_STEER_CARRY", "RKH_STEER_CARRY_FIT", "RKH_STEER_CLEARANCE", "RKH_WAVE_FIT", "RKH_BATCH_FACTOR",
          "RKH_BATCH_MAX", "RKH_BATCH_MIN")
_WAVE = {"RKH_LANES_PER_EDGE": "64"}
_WHOLE = {"RKH_LANES_PER_EDGE": "2"}
_STEPS = {"RKH_LANES_PER_EDGE": "0", "RKH_LANE_THRESHOLD": "1", "RKH_STEER_SPLIT_MIN_EDGES": "0"}


def _case_id(case):
    return "n%d" % case[0] + ("_p" + "".join(map(str, case[1])) if case[1] else "")


def _scene(n, prism, dt=None):
    if n == 6 and not prism:
        return scenarios.make_c2(world_seed=1) if dt is None else scenarios.make_c2(world_seed=1, dt=dt)
    scn = scenarios.make_random_chain(n, seed=n)
    for j, op in enumerate([o for o in scn.ops if o.kind == T.KTE_REVOLUTE_JOINT_3D]):
        if j in prism:
            op.kind = T.KTE_PRISMATIC_JOINT_3D
            op.axis[:] = [0.7 * v for v in op.axis]  # prismatic axes are not unit length
            scn.dyn.lower[2 * j], scn.dyn.upper[2 * j] = -0.5, 0.5
    return scn


def _inner_counts(dt, steps):
    """runge_kutta4_integrate_impl's loop iterations per step (runge_kutta4_integrator_sys.hpp:73-96), in the fp64
    arithmetic the library's host code evaluates (build_dyn_dev)."""
    out, current = [], 0.0
    for _ in range(steps):
        t, end, it = current, current + dt, 0
        while t < end:
            t += dt * 0.5
            t += dt * 0.5
            it += 1
        out.append(it)
        current += dt
    return out


_OUTWARD = range(1, 7)  # rows of _edges built to leave the hyperbox


def _edges(scn, count):
    """`count` (source, target) pairs of the state box.  Row 0: source == target (the edge ends before its first step
    and stays at its source).  Rows 1 .. 6: joint 0 starts a quarter of the edge's time inside its upper (odd rows) or
    lower position bound, moving outwards at half the speed bound, which the target keeps up: the state leaves the
    hyperbox on the way unless an obstacle ends the edge first (the other joints differ from row to row).  Rows 7 .. 11:
    at rest with a target close by (they run all steps where nothing is in the way).  Then random pairs."""
    D = scn.D
    lo = np.array([scn.dyn.lower[i] for i in range(D)])
    hi = np.array([scn.dyn.upper[i] for i in range(D)])
    rng = np.random.default_rng(900 + D)
    a = rng.uniform(lo, hi, size=(count, D))
    a[:, 1::2] *= 0.6
    b = rng.uniform(lo, hi, size=(count, D))
    b[0] = a[0]
    span = hi[0] - lo[0]
    horizon = scn.dyn.steps_per_edge * scn.dyn.dt
    for row in range(1, min(count, 12)):
        a[row, 1::2] = 0.0
        a[row, 0::2] *= 0.25
        b[row] = a[row]
        b[row, 0::2] += 0.01
        if row in _OUTWARD:
            edge, speed = (hi[0], 0.5 * hi[1]) if row & 1 else (lo[0], 0.5 * lo[1])
            a[row, 0] = edge - 0.25 * horizon * speed
            a[row, 1] = speed
            b[row, 0], b[row, 1] = edge, speed
            assert lo[0] < a[row, 0] < hi[0] and abs(a[row, 0] - edge) < 0.5 * span
    return a, b


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


def _steer(L, sc, a, b, env, record):
    with _environment(env):
        out = sc.steer_position_toward(a, b, record=record)
        return out, L.steer_mapping_name()


def _same_steer(got, ref, what):
    assert np.array_equal(got[1], ref[1]), (what, "steps_free")
    assert np.array_equal(got[0], ref[0]), (what, "end state")
    if ref[2] is not None:
        assert np.array_equal(got[2], ref[2], equal_nan=True), (what, "record")


@pytest.mark.parametrize("case", _CASES, ids=_case_id)
def test_whole_edge_kernel_at_ragged_counts_with_and_without_records(L, ctx, oracle, case):
    """1, 31, 32, 33 and 65 edges, record rows on and off, clearance on and off: end states, free-step counts and every
    recorded state equal the one-wave mapping's bit for bit.  The 65 edges hold an edge that ends before its first step,
    edges that leave the hyperbox mid-way and edges that run all steps; C2's results also agree with the oracle."""
    n, prism = case
    scn = _scene(n, prism)
    steps = scn.dyn.steps_per_edge
    a, b = _edges(scn, max(_COUNTS))
    sc = L.Scene(ctx, scn)
    for B in _COUNTS:
        for record in (False, True):
            ref, name = _steer(L, sc, a[:B], b[:B], _WAVE, record)
            assert name == ("prismatic" if prism else "wave")
            got, name = _steer(L, sc, a[:B], b[:B], _WHOLE, record)
            assert name == "pair"
            _same_steer(got, ref, (B, record, "clearance on"))
            got, _ = _steer(L, sc, a[:B], b[:B], dict(_WHOLE, RKH_STEER_CLEARANCE="0"), record)
            _same_steer(got, ref, (B, record, "clearance off"))
        if B == max(_COUNTS):
            free = ref[1]
            print(_case_id(case), "steps_free", np.bincount(free, minlength=steps + 1).tolist())
            assert free[0] == 0 and np.array_equal(ref[0][0], a[0])  # ended before its first step: stays at its source
            assert free.max() == steps
            left = []  # left the hyperbox on the way: ended mid-way with the last free state within a step of the bound
            for row in _OUTWARD:
                edge, speed = b[row, 0], b[row, 1]
                print("  row", row, "free", free[row], "bound", edge, "last free q0", ref[2][row, free[row], 0])
                left.append(0 < free[row] < steps and abs(ref[2][row, free[row], 0] - edge) <= 1.5 * scn.dyn.dt * abs(speed))
            assert any(left[0::2]) and any(left[1::2]), left  # through the upper and through the lower bound
            if case == (6, ()):
                rc, rout, rsteps, _ = oracle.OracleScene(scn).steer(a, b)
                assert rc == 0 and np.array_equal(got[1], rsteps)
                assert np.allclose(got[0], rout, rtol=STATE_RTOL, atol=1e-12)
    sc.close()


def _plan(L, ctx, scn, prms, env):
    with _environment(dict(env, RKH_WAVE_FIT="0")):  # every mapping sees the same rounds: the step counters compare
        sc = L.Scene(ctx, scn)
        pl = L.RrtPlanner(sc, prms)
        run = {"mapping": L.steer_mapping_name()}
        pl.solve_planning_query()
        run["stats"] = [(int(s.num_vertices), int(s.iterations), int(s.edges_checked), int(s.num_solutions),
                         float(s.best_cost)) for s in pl.all_stats]
        run["trees"] = [pl.tree(i) for i in range(len(prms))]
        run["steps"] = pl.steer_steps()
        run["rounds"] = [(int(s.rounds), int(s.edges_speculated)) for s in pl.all_stats]
        run["carry"] = pl.carry_counts()
        run["clearance"] = sc.steer_clearance_counts()
        pl.close()
        sc.close()
    return run


def _same_plan(a, b, what, steps=True):
    assert a["stats"] == b["stats"], what
    for i, (ta, tb) in enumerate(zip(a["trees"], b["trees"])):
        for key in ("pos", "parent", "nn_seq", "accept", "goal_dist"):
            assert np.array_equal(ta[key], tb[key]), (what, i, key)
    if steps:
        assert a["steps"] == b["steps"], what


def _ran_step_wise(steps, whole):
    """Only the step-wise launches pack the live edges of all segments into full waves step after step, so fewer
    wave-steps run the proximity test than in the whole-edge launch, whose waves keep their 32 edges of one segment (the
    counter counts them with the clearance on or off): a quiet fall-back to the whole-edge launch would show equal counts."""
    assert 0 < steps["clearance"][1] < whole["clearance"][1], (steps["clearance"], whole["clearance"])


@pytest.mark.parametrize("case", _CASES, ids=_case_id)
def test_step_kernel_gives_the_one_wave_and_the_whole_edge_results(L, ctx, oracle, case):
    """One problem whose rounds start at a single candidate, and three problems: trees (states, parents, NN sequences,
    accept bytes, goal distances), stats and the executed-step counter of the step-wise launches equal the one-wave
    mapping's and the whole-edge launch's; without the carried clearance (RKH_STEER_CLEARANCE=0) the step-wise launches
    give the same again.  C2's first tree also agrees with the oracle's sequential planner."""
    n, prism = case
    scn = _scene(n, prism)
    small = {"RKH_BATCH_MIN": "1", "RKH_BATCH_FACTOR": "0.7"}
    for prms, knobs in (([scn.rrt_params(seed=5, max_vertices=120)], small),
                        ([scn.rrt_params(seed=s, max_vertices=300) for s in (1, 2, 3)], {})):
        wave = _plan(L, ctx, scn, prms, dict(_WAVE, **knobs))
        whole = _plan(L, ctx, scn, prms, dict(_WHOLE, **knobs))
        steps = _plan(L, ctx, scn, prms, dict(_STEPS, RKH_STEER_CARRY="0", **knobs))
        plain = _plan(L, ctx, scn, prms, dict(_STEPS, RKH_STEER_CARRY="0", RKH_STEER_CLEARANCE="0", **knobs))
        assert [r["mapping"] for r in (wave, whole, steps, plain)] == ["prismatic" if prism else "wave", "pair", "auto", "auto"]
        assert wave["steps"] > 0 and all(s[0] >= prms[0].max_vertices for s in wave["stats"])
        _same_plan(whole, wave, "whole-edge against one wave")
        _same_plan(steps, wave, "step-wise against one wave")
        _same_plan(steps, whole, "step-wise against whole-edge")
        _same_plan(plain, steps, "clearance off against on")
        print(_case_id(case), len(prms), "clearance counts: whole-edge", whole["clearance"], "step-wise", steps["clearance"],
              "off", plain["clearance"])
        assert plain["clearance"][0] == 0  # nothing is settled by a bound that is switched off
        # the edge-steps the bound settles are the same on both paths (as measured before the edge I/O was batched; the
        # wave-steps that test differ: the step-wise launches pack the live edges of all segments into full waves)
        assert steps["clearance"][0] == whole["clearance"][0]
        _ran_step_wise(steps, whole)
        if case == (6, ()):
            assert steps["clearance"][0] > 0 and whole["clearance"][0] > 0  # C2 carries its clearance
            if len(prms) == 3:
                rc, rout, rtree = oracle.OracleScene(scn).rrt_dyn(prms[0])
                t = steps["trees"][0]
                assert rc == 0 and steps["stats"][0][0] == rout.num_vertices
                assert np.array_equal(t["parent"], rtree["parent"]) and np.array_equal(t["accept"], rtree["accept"])
                assert np.allclose(t["pos"], rtree["pos"], rtol=STATE_RTOL, atol=1e-12)


@pytest.mark.parametrize("problems", [1, 3], ids=["p1", "p3"])
@pytest.mark.parametrize("case", _CASES, ids=_case_id)
def test_step_kernel_at_exact_round_sizes_with_mixed_chunks(L, ctx, case, problems):
    """Exactly 1, 31, 32, 33 and 65 candidates per problem in every round (see the module's text), one problem and
    three: the step-wise launches give the trees, stats and executed steps of the one-wave mapping and of the whole-edge
    launch.  Every round offered exactly that many candidates, and the trees grew, so rounds carried the goal probes of
    new vertices behind their candidates: the mixed chunks ran."""
    n, prism = case
    scn = _scene(n, prism)
    for count in _COUNTS:
        knobs = {"RKH_BATCH_FACTOR": "0", "RKH_BATCH_MIN": str(count), "RKH_BATCH_MAX": str(max(count, 8))}
        size = 40 if count == 1 else 150
        prms = [scn.rrt_params(seed=s, max_vertices=size) for s in range(1, problems + 1)]
        wave = _plan(L, ctx, scn, prms, dict(_WAVE, **knobs))
        whole = _plan(L, ctx, scn, prms, dict(_WHOLE, **knobs))
        steps = _plan(L, ctx, scn, prms, dict(_STEPS, RKH_STEER_CARRY="0", **knobs))
        assert [r["mapping"] for r in (wave, whole, steps)] == ["prismatic" if prism else "wave", "pair", "auto"]
        print(_case_id(case), problems, count, "rounds, candidates", steps["rounds"], "vertices", [s[0] for s in steps["stats"]],
              "tests whole-edge / step-wise", whole["clearance"][1], steps["clearance"][1])
        # edges_speculated = the candidates of all rounds + one goal probe per vertex added (rkh_planner_sync)
        for (rounds, speculated), stats in zip(steps["rounds"], steps["stats"]):
            probes = stats[0] - 1
            assert rounds > 1 and speculated - probes == count * rounds  # exactly `count` candidates in every round
            assert stats[0] >= size and probes > 0  # vertices were added: the rounds after them carried their probes
        assert steps["rounds"] == wave["rounds"] == whole["rounds"]
        _same_plan(steps, wave, (count, "step-wise against one wave"))
        _same_plan(steps, whole, (count, "step-wise against whole-edge"))
        if problems == 3:
            _ran_step_wise(steps, whole)
        else:  # one problem's whole-edge launch has one candidates wave up to 32: the counts can coincide
            assert 0 < steps["clearance"][1] <= whole["clearance"][1]


def test_steps_with_inner_sub_steps_read_their_start_from_the_row(L, ctx):
    """A time step whose schedule gives some steps two RK4 iterations (DynDev::inner[k] == 2): the workspace then holds
    the last sub-step's start, and the clearance delta of the step kernel reads the edge's row again.  C2 with such a
    time step: rkh_propagate and the planner's trees equal the one-wave mapping's, with the clearance on and off."""
    steps = 20
    dt = next(d for d in (1.1e-3, 1.25e-3, 1.9e-3, 2e-3, 1e-2) if max(_inner_counts(d, steps)) > 1)
    inner = _inner_counts(dt, steps)
    print("dt", dt, "inner", inner)
    assert 1 in inner and 2 in inner
    scn = _scene(6, (), dt=dt)
    assert scn.dyn.dt == dt and scn.dyn.steps_per_edge == steps
    a, b = _edges(scn, 65)
    sc = L.Scene(ctx, scn)
    ref, _ = _steer(L, sc, a, b, _WAVE, True)
    got, name = _steer(L, sc, a, b, _WHOLE, True)
    assert name == "pair" and ref[1].max() > inner.index(2)  # edges live through a step with sub-steps
    _same_steer(got, ref, "inner sub-steps")
    sc.close()
    prms = [scn.rrt_params(seed=s, max_vertices=300) for s in (1, 2, 3)]
    wave = _plan(L, ctx, scn, prms, _WAVE)
    on = _plan(L, ctx, scn, prms, dict(_STEPS, RKH_STEER_CARRY="0"))
    off = _plan(L, ctx, scn, prms, dict(_STEPS, RKH_STEER_CARRY="0", RKH_STEER_CLEARANCE="0"))
    _same_plan(on, wave, "step-wise against one wave")
    _same_plan(off, on, "clearance off against on")
    assert on["clearance"][0] > 0


def test_a_carrying_round_reads_its_list_in_launch_0(L, ctx):
    """Three C2 problems with every round carrying (tests/test_round_carry_gpu.py): launch 0 then takes its edges from
    a list, like every later launch, while still writing the `first` rows.  Trees and stats equal RKH_STEER_CARRY=0."""
    scn = scenarios.make_c2(world_seed=1)
    prms = [scn.rrt_params(seed=s, max_vertices=600) for s in (1, 2, 3)]
    env = dict(_STEPS, RKH_STEER_CARRY_MIN_EDGES="0")
    on = _plan(L, ctx, scn, prms, env)
    off = _plan(L, ctx, scn, prms, dict(env, RKH_STEER_CARRY="0"))
    print("carry on", on["carry"], "steps", on["steps"], "off", off["carry"], "steps", off["steps"])
    _same_plan(on, off, "carry on against off", steps=False)
    assert on["carry"][1] > 0 and off["carry"][1] == 0 and on["steps"] < off["steps"]
