"""The batch RRT over the SVP space (rkh_svp_rrt_*) against its Python twin (tests/svp_rrt_ref.py over tests/svp_ref.py):
every problem's vertices, parents, edge times, iteration count, goal parent and solution bit for bit, whatever the batch
holds beside it.  The twin's collision predicate is rkh_min_distance at the same model-unit points (one call per walk), as
the walk tests of tests/test_svp_space_gpu.py batch it.  The arithmetic is fp64 with contraction off on both sides: a
difference is a bug, not a tolerance to widen."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import svp_ref as R
import svp_rrt_ref as RR
from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
NO_INDEX = 0xFFFFFFFF
BRANCHES = ("out_of_bounds", "no_neighbour", "nothing_checked", "no_progress", "committed")


@pytest.fixture(scope="module")
def ctx():
    from reak_amd import lib as L
    return L.Context(0)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def make_walk(sp, scene):
    """The twin's walk with rkh_min_distance as the collision test: all points of the edge in one call"""
    has_pairs = scene.num_pairs > 0

    def walk(a, b, f):
        Tt, peak = R.reach(sp, a, b)
        dist = []
        if Tt < math.inf and has_pairs:
            rows = [R.model_units(sp, R.point(sp, a, b, peak, Tt, d)) for d in R.walk_times(sp, Tt * f)]
            if rows:
                dist = scene.min_distance(np.array(rows)).tolist()
        it = iter(dist)
        return R.edge_walk(sp, a, b, f, (lambda x: not (next(it) < 0.0)) if has_pairs else (lambda x: True))

    return walk


def twin_trees(sp, walk, problems):
    return [RR.rrt(sp, walk, p["start"], p["goal"], p["seed"], p["max_vertices"], p["max_iterations"], p["max_edge_time"],
                   p["steer_tol"]) for p in problems]


def c_params(problems):
    return [T.make_svp_rrt_params(p["start"], p["goal"], p["seed"], p["max_vertices"], p["max_iterations"], p["max_edge_time"],
                                  p["steer_tol"]) for p in problems]


def assert_problem_is_the_twins(planner, i, status, sp, problem, want, tag):
    nv, it, gp = status
    tree = planner.tree(i)
    assert nv[i] == len(want["vertices"]) == len(tree["vertices"]), (tag, i, nv[i], len(want["vertices"]))
    assert it[i] == want["iterations"] and gp[i] == want["goal_parent"], (tag, i, it[i], want["iterations"], gp[i])
    assert tree["parent"].tolist() == want["parent"], (tag, i)
    assert _same(tree["vertices"], np.array(want["vertices"])), (tag, i)
    assert _same(tree["edge_time"], np.array(want["edge_time"])), (tag, i)
    pts, dur = planner.solution(i)
    wpts, wdur = RR.solution(sp, want, problem["goal"]) if problem["goal"] is not None else ([], 0.0)
    assert len(pts) == len(wpts) and (not wpts or _same(pts, np.array(wpts))), (tag, i)
    assert _same(np.array([dur]), np.array([wdur])), (tag, i, dur, wdur)


# ---- C2 ---------------------------------------------------------------------------------------------------------------------
def c2_problems():
    """70 problems on C2: seeds, starts (at rest / in motion), with and without a goal, max_vertices 5 .. 60,
    max_iterations 3 .. 400.  Problem 2 is the one of tests/test_svp_rrt_cpu.py that cannot move (max_edge_time below
    min_interval) and meets a candidate no vertex reaches."""
    import plan_svp_rrt as E
    scn = scenarios.make_c2(world_seed=1)
    n, lower, upper, mi, speed, accel = E.c2_space()
    sp = R.Space(n, lower, upper, mi, speed, accel)
    rest = E.to_space(scn.start[0::2]).tolist()
    moving = list(rest)
    for i in range(n):
        moving[2 * i + 1] = (0.7 if i % 2 == 0 else -0.6) * sp.vm[i]
    goal = E.to_space(E.GOAL).tolist()
    probs = []
    for i in range(70):
        probs.append({"seed": 1 + i, "start": moving if i % 7 == 3 else rest, "goal": None if i % 3 == 1 else goal,
                      "max_vertices": 5 + (i * 11) % 56, "max_iterations": (400, 40, 120, 400, 17, 250, 3)[i % 7],
                      "max_edge_time": (1.0, 1.0, 0.5, 1.0, 0.04)[i % 5], "steer_tol": 0.1})
    probs[0].update(seed=4, max_vertices=40, max_iterations=400, max_edge_time=1.0)
    probs[1].update(seed=2, max_vertices=12, max_iterations=400, max_edge_time=1.0)
    probs[2].update(seed=1, start=moving, goal=goal, max_vertices=40, max_iterations=150, max_edge_time=0.04)
    probs[5].update(goal=None, max_vertices=60, max_iterations=400, max_edge_time=1.0)
    return scn, sp, probs


_C2 = {}


def _c2(ctx):
    """scene, space, the 70 problems and the twin's trees, computed once"""
    if not _C2:
        from reak_amd import lib as L
        scn, sp, probs = c2_problems()
        scene = L.Scene(ctx, scn)
        _C2["v"] = (scene, sp, probs, twin_trees(sp, make_walk(sp, scene), probs))
    return _C2["v"]


def check_c2_conditions(probs, want, P):
    """what the issue asks of the inputs, on the twin's values"""
    sub = want[:P]
    whys = {t["why"] for t in sub}
    if P >= 3:
        assert whys == {"goal", "max_vertices", "max_iterations"}, whys
        for key in BRANCHES:
            assert sum(t["branches"][key] for t in sub) >= 1, key
        # problems end in different rounds: a round takes one candidate that is in bounds (or the last iterations)
        rounds = [t["iterations"] - t["branches"]["out_of_bounds"] for t in sub]
        assert len(set(rounds)) >= 3 and min(rounds) < max(rounds)
    if P == 70:
        assert any(t["goal_parent"] not in (0, NO_INDEX) for t in sub)
        assert max(len(t["vertices"]) for t in sub) == 60 and min(p["max_vertices"] for p in probs) == 5
        assert max(t["iterations"] for t in sub) == 400 and min(t["iterations"] for t in sub) <= 3


@pytest.mark.parametrize("P", [1, 3, 70])
def test_batch_is_the_twins_trees_bit_for_bit(ctx, P):
    from reak_amd import lib as L
    scene, sp, probs, want = _c2(ctx)
    check_c2_conditions(probs, want, P)
    pl = L.SvpRrt(scene, sp.c_space(), c_params(probs[:P]))
    st = pl.solve()
    assert st.problems_finished == P and pl.finished
    status = pl.status()
    for i in range(P):
        assert_problem_is_the_twins(pl, i, status, sp, probs[i], want[i], ("c2", P))
    assert st.iterations == sum(t["iterations"] for t in want[:P])
    assert st.vertices == sum(len(t["vertices"]) for t in want[:P])
    assert st.rounds >= 1 and st.tested_points > 0 and st.walk_passes >= 1
    assert st.window_refills == sum(-(-t["iterations"] // RR.WINDOW) for t in want[:P])
    print("P", P, "rounds", st.rounds, "iterations", st.iterations, "vertices", st.vertices, "walk passes", st.walk_passes,
          "tested points", st.tested_points)
    pl.close()


def test_problem_of_the_batch_equals_the_same_parameters_alone(ctx):
    from reak_amd import lib as L
    scene, sp, probs, want = _c2(ctx)
    batch = L.SvpRrt(scene, sp.c_space(), c_params(probs))
    batch.solve()
    bs = batch.status()
    for i in (0, 2, 5, 33, 69):
        alone = L.SvpRrt(scene, sp.c_space(), c_params([probs[i]]))
        alone.solve()
        s1 = alone.status()
        ta, tb = alone.tree(0), batch.tree(i)
        assert (s1[0][0], s1[1][0], s1[2][0]) == (bs[0][i], bs[1][i], bs[2][i]), i
        assert np.array_equal(ta["parent"], tb["parent"]) and _same(ta["vertices"], tb["vertices"]), i
        assert _same(ta["edge_time"], tb["edge_time"]), i
        (pa, da), (pb, db) = alone.solution(0), batch.solution(i)
        assert _same(pa, pb) and da == db, i
        alone.close()
    batch.close()


# ---- the slice boundary of the nearest sweep ------------------------------------------------------------------------------
def test_trees_across_the_slice_boundary_of_the_nearest_sweep(ctx):
    """The obstacle-free cube of three joints, no goal: trees of 5, 257 and 300 vertices in one batch -- 1, 2 and 2 slices
    of 256 vertices in one launch, the 257th vertex alone in its slice."""
    from reak_amd import lib as L
    scene = L.Scene(ctx, scenarios.make_hidim(3))
    sp = R.Space(3, [0.0] * 3, [1.0] * 3, 0.05)
    start = [0.5, 0.0, 0.5, 0.0, 0.5, 0.0]
    probs = [{"seed": 11 + k, "start": start, "goal": None, "max_vertices": mv, "max_iterations": 4000, "max_edge_time": 0.3,
              "steer_tol": 0.1} for k, mv in enumerate((5, 300, 257))]
    want = twin_trees(sp, make_walk(sp, scene), probs)
    assert [len(t["vertices"]) for t in want] == [5, 300, 257] and all(t["why"] == "max_vertices" for t in want)
    assert RR.SLICE == 256 and max(max(t["parent"][1:]) for t in want) >= RR.SLICE   # a parent from the second slice
    pl = L.SvpRrt(scene, sp.c_space(), c_params(probs))
    pl.solve()
    status = pl.status()
    for i in range(3):
        assert_problem_is_the_twins(pl, i, status, sp, probs[i], want[i], "hidim3")
    pl.close()


# ---- the other scene kinds ------------------------------------------------------------------------------------------------
def _limits(n):
    speed = [(1.0, 0.0, 1.5, 2.0, 0.5)[i % 5] for i in range(n)]
    accel = [(2.0, 4.0, 0.0, 3.0)[i % 4] for i in range(n)]
    return speed, accel


KINDS = {  # the scenes of the walk tests (tests/test_svp_space_gpu.py): scenario, half width of the joint box in model units
    "c1_planar": (scenarios.make_c1_planar, 2.5),
    "track": (lambda: scenarios.make_crs_a465_track(n_obstacles=150), 2.5),
    "c4_meshes": (lambda: scenarios.make_c4(meshes=True), 2.0),
}


@pytest.mark.parametrize("name", sorted(KINDS))
def test_short_batches_on_the_other_scene_kinds(ctx, name):
    from reak_amd import lib as L
    scn = KINDS[name][0]()
    scene = L.Scene(ctx, scn)
    n, half = scn.n_dof, KINDS[name][1]
    speed, accel = _limits(n)
    unit = R.Space(n, [0.0] * n, [1.0] * n, 1.0, speed, accel)
    sp = R.Space(n, [-half / s for s in unit.speed], [half / s for s in unit.speed], 0.06, speed, accel)
    q0 = np.asarray(scn.start, dtype=float)
    q1 = np.asarray(scn.goal, dtype=float)
    q0 = q0[0::2] if len(q0) == 2 * n else q0
    q1 = q1[0::2] if len(q1) == 2 * n else q1
    start, goal = [0.0] * (2 * n), [0.0] * (2 * n)
    start[0::2] = (q0 / np.array(unit.speed)).tolist()
    goal[0::2] = (np.clip(q1, -0.9 * half, 0.9 * half) / np.array(unit.speed)).tolist()
    assert R.in_bounds(sp, start)
    probs = [{"seed": 3 + k, "start": start, "goal": goal if k % 2 == 0 else None, "max_vertices": (30, 12, 20, 30)[k],
              "max_iterations": 200, "max_edge_time": (1.0, 1.0, 0.6, 1.0)[k], "steer_tol": 0.1} for k in range(4)]
    want = twin_trees(sp, make_walk(sp, scene), probs)
    print(name, [(t["why"], len(t["vertices"]), t["iterations"], t["branches"]) for t in want])
    assert sum(t["branches"]["committed"] for t in want) >= 8 and max(len(t["vertices"]) for t in want) >= 12
    if scene.num_pairs > 0:
        assert sum(t["branches"]["no_progress"] for t in want) >= 1
    pl = L.SvpRrt(scene, sp.c_space(), c_params(probs))
    pl.solve()
    status = pl.status()
    for i in range(4):
        assert_problem_is_the_twins(pl, i, status, sp, probs[i], want[i], name)
    pl.close()


# ---- resume ---------------------------------------------------------------------------------------------------------------
def test_one_round_at_a_time_gives_the_same_trees(ctx):
    """solve(max_rounds = 1) until finished against one solve to the end; each problem draws more than two windows of
    candidates (64 each), so the sample stream is refilled at least twice on the way."""
    from reak_amd import lib as L
    scene, sp, probs, _ = _c2(ctx)
    mine = [dict(probs[1], seed=21 + k, goal=None, max_vertices=90, max_iterations=4000) for k in range(2)]
    whole = L.SvpRrt(scene, sp.c_space(), c_params(mine))
    ws = whole.solve()
    steps = L.SvpRrt(scene, sp.c_space(), c_params(mine))
    rounds = 0
    while not steps.finished:
        before = steps.stats.rounds
        st = steps.solve(1)
        rounds += 1
        assert st.rounds == before + 1 and rounds <= 4000
    st = steps.solve(1)   # nothing left: no round runs
    assert st.rounds == rounds == ws.rounds
    a, b = whole.status(), steps.status()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert (a[1] > 2 * RR.WINDOW).all(), a[1]
    assert ws.window_refills == st.window_refills == sum(-(-int(i) // RR.WINDOW) for i in a[1]) >= 3 * len(mine)
    for i in range(len(mine)):
        ta, tb = whole.tree(i), steps.tree(i)
        assert len(ta["vertices"]) == 90
        assert np.array_equal(ta["parent"], tb["parent"]) and _same(ta["vertices"], tb["vertices"]), i
        assert _same(ta["edge_time"], tb["edge_time"]), i
    assert (st.iterations, st.vertices, st.tested_points, st.walk_passes) == (ws.iterations, ws.vertices, ws.tested_points,
                                                                              ws.walk_passes)
    whole.close()
    steps.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_no_planner_behind(ctx):
    from reak_amd import lib as L
    scene, sp, probs, _ = _c2(ctx)
    lib = L.load()
    good = c_params(probs[:1])[0]
    space = sp.c_space()

    def refused(space_, params, P, word):
        h = C.c_void_p(0xDEAD)
        arr = (T.SvpRrtParams * max(len(params), 1))(*params)
        st = lib.rkh_svp_rrt_create_batch(scene.h, C.byref(space_), arr, P, C.byref(h))
        msg = lib.rkh_last_error().decode()
        assert st == -1 and h.value is None and word in msg, (st, h.value, msg, word)

    def changed(**kw):
        p = T.SvpRrtParams.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    refused(space, [changed(struct_size=C.sizeof(T.SvpRrtParams) - 8)], 1, "struct_size")
    small = sp.c_space()
    small.struct_size -= 8
    refused(small, [good], 1, "struct_size")
    three = R.Space(3, [-1.0] * 3, [1.0] * 3, 0.05).c_space()
    refused(three, [good], 1, "n_dof")
    refused(space, [changed(max_vertices=0)], 1, "max_vertices")
    out = T.SvpRrtParams.from_buffer_copy(good)
    out.start[0] = 1.01 * sp.upper[0]
    refused(space, [out], 1, "bounds")
    fast = T.SvpRrtParams.from_buffer_copy(good)
    fast.start[1] = 1.5 * sp.vm[0]
    refused(space, [fast], 1, "bounds")
    nan = T.SvpRrtParams.from_buffer_copy(good)
    nan.start[3] = math.nan
    refused(space, [nan], 1, "finite")
    refused(space, [good, out], 2, "problem 1")   # the second of two
    refused(space, [good], 0, "16384")
    refused(space, [good] * 16385, 16385, "16384")
    # and the binding raises on them
    with pytest.raises(L.RkhError):
        L.SvpRrt(scene, space, [changed(max_vertices=0)])
    # a planner of a valid batch still comes up afterwards
    pl = L.SvpRrt(scene, space, [good])
    assert pl.solve().problems_finished == 1
    pl.close()


def test_an_edge_over_the_walks_point_cap_is_a_capacity_error(ctx):
    """min_interval 1e-7 against reach times of seconds: more than 1 048 576 points to test.  With a goal the probe before
    the loop meets it (no planner comes up); without one the first extension does, and the planner refuses further rounds."""
    from reak_amd import lib as L
    scene, sp, probs, _ = _c2(ctx)
    fine = R.Space(sp.n, sp.lower, sp.upper, 1e-7, sp.speed, sp.accel).c_space()
    with pytest.raises(L.RkhError) as e:
        L.SvpRrt(scene, fine, c_params([probs[0]]))
    assert e.value.status == -6 and "1 048 576" in str(e.value)
    pl = L.SvpRrt(scene, fine, c_params([dict(probs[1], max_edge_time=1.0)]))
    with pytest.raises(L.RkhError) as e:
        pl.solve()
    assert e.value.status == -6
    with pytest.raises(L.RkhError):
        pl.solve()
    assert pl.tree(0)["parent"].tolist() == [NO_INDEX]   # the tree is still readable: the start alone
    pl.close()


def test_a_box_that_rejects_every_candidate_ends_on_max_iterations(ctx):
    """Joint 0's position interval is a single value: a candidate with any velocity on it could not stop inside, so the
    sampler rejects all 5000.  A launch of the sample kernel draws at most 16 windows of 64 per problem: the problem sits
    rounds out instead of holding one launch for max_iterations candidates, and ends as the twin does."""
    from reak_amd import lib as L
    scene = L.Scene(ctx, scenarios.make_hidim(3))
    sp = R.Space(3, [0.5, 0.0, 0.0], [0.5, 1.0, 1.0], 0.05)
    start = [0.5, 0.0, 0.5, 0.0, 0.5, 0.0]
    assert R.in_bounds(sp, start)
    probs = [{"seed": 5, "start": start, "goal": None, "max_vertices": 10, "max_iterations": 5000, "max_edge_time": 0.3,
              "steer_tol": 0.1}]
    want = twin_trees(sp, make_walk(sp, scene), probs)
    assert want[0]["branches"]["out_of_bounds"] == 5000 and want[0]["why"] == "max_iterations"
    pl = L.SvpRrt(scene, sp.c_space(), c_params(probs))
    st = pl.solve()
    assert_problem_is_the_twins(pl, 0, pl.status(), sp, probs[0], want[0], "all rejected")
    assert st.rounds == -(-5000 // (16 * RR.WINDOW)) and st.window_refills == -(-5000 // RR.WINDOW)
    pl.close()
