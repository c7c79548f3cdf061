"""The backward walk (rkh_svp_edge_check_back), the launch with a direction per row (rkh_diag_svp_edge_check_dir) and the
batch bidirectional RRT over the SVP space (rkh_svp_birrt_*) against their Python twins (tests/svp_back_ref.py,
tests/svp_birrt_ref.py over tests/svp_ref.py and tests/svp_rrt_ref.py): every output bit for bit.  The twins' collision
predicate is rkh_min_distance at the same model-unit points.  The arithmetic is fp64 with contraction off on both sides: a
difference is a bug, not a tolerance to widen."""
import ctypes as C
import math

import numpy as np
import pytest

import svp_back_ref as RB
import svp_birrt_ref as BR
import svp_ref as R
import svp_rrt_ref as RR
from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    from reak_amd import lib as L
    return L.Context(0)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


# ---- the walks ----------------------------------------------------------------------------------------------------------------
def _limits(n):
    speed = [(1.0, 0.0, 1.5, 2.0, 0.5)[i % 5] for i in range(n)]
    accel = [(2.0, 4.0, 0.0, 3.0)[i % 4] for i in range(n)]
    return speed, accel


SCENES = {  # the scene kinds of the walk tests: scenario, half width of the joint box in model units
    "c2": (lambda: scenarios.make_c2(world_seed=1), 2.5),
    "c1_planar": (scenarios.make_c1_planar, 2.5),
    "track": (lambda: scenarios.make_crs_a465_track(n_obstacles=150), 2.5),
    "c4_meshes": (lambda: scenarios.make_c4(meshes=True), 2.0),
}


def _walk_case(name, scene, scn, B, seed):
    """space, B edges (the last 6 the special ones of svp_ref.random_pairs) and their fractions"""
    n, half = scn.n_dof, SCENES[name][1]
    speed, accel = _limits(n)
    unit = R.Space(n, [0.0] * n, [1.0] * n, 1.0, speed, accel)
    sp = R.Space(n, [-half / s for s in unit.speed], [half / s for s in unit.speed], 0.06, speed, accel)
    a, b, _ = R.random_pairs(sp, B - 6, seed=seed)
    assert len(a) == B
    rng = np.random.default_rng(seed + 1000)
    # ends that are themselves acceptable (at rest, inside the box) for most edges, so that backward walks get under way
    b[:150, 1::2] = 0.0
    b[:150, 0::2] *= 0.8
    a[:90, 1::2] *= 0.3
    a[:90, 0::2] *= 0.8
    fraction = np.array([(1.0, 0.0)[e % 2] if e % 3 == 0 else rng.uniform(0.02, 0.98) for e in range(B)])
    # an edge shorter than min_interval (rest to rest over 2e-4 vm takes 2 vm sqrt(2e-4)): nothing to test, reached
    a[160], b[160] = 0.0, 0.0
    b[160, 0] = 2e-4 * sp.vm[0]
    fraction[160] = 1.0
    # whole traverses of the box at rest, walked to the end: edges of several passes
    for k, span in enumerate((0.75, 0.6, 0.45, 0.3)):
        a[161 + k], b[161 + k] = 0.0, 0.0
        a[161 + k, 0::2], b[161 + k, 0::2] = span * np.array(sp.lower), span * np.array(sp.upper)
        fraction[161 + k] = 1.0
    if scene.num_pairs > 0:
        # edges that end in a colliding configuration (stopped at their first point from the end) and edges from a colliding
        # one to a free one (stopped later)
        rest = np.zeros((4000, 2 * n))
        rest[:, 0::2] = rng.uniform(0.8 * np.array(sp.lower), 0.8 * np.array(sp.upper), size=(4000, n))
        d = scene.min_distance(np.array([R.model_units(sp, x) for x in rest.tolist()]))
        hit, free = rest[d < 0.0], rest[d > 0.05]
        assert len(hit) >= 4 and len(free) >= 4, (name, len(hit), len(free))
        b[151:155], a[155:159], b[155:159] = hit[:4], hit[:4], free[:4]
        fraction[151:159] = 1.0
    return sp, np.ascontiguousarray(a), np.ascontiguousarray(b), fraction


def _twin_walks(sp, scene, a, b, fraction, back):
    """the twin's walk of every edge in its direction; the collision test of all points of all edges in ONE
    rkh_min_distance call"""
    has_pairs = scene.num_pairs > 0
    edges, rows = [], []
    for ae, be, f, bk in zip(a.tolist(), b.tolist(), fraction, back):
        Tt, peak = R.reach(sp, ae, be)
        pts = [R.point(sp, ae, be, peak, Tt, d) for d in RB.times_dir(sp, Tt, float(f), bk)] if Tt < math.inf else []
        edges.append((len(rows), len(pts)))
        rows.extend(R.model_units(sp, x) for x in pts)
    dist = scene.min_distance(np.array(rows)) if (rows and has_pairs) else np.full(len(rows), np.inf)
    out = []
    for (first, count), ae, be, f, bk in zip(edges, a.tolist(), b.tolist(), fraction, back):
        it = iter(range(first, first + count))
        out.append(RB.walk_dir(sp, ae, be, float(f), bk, lambda x: not (dist[next(it)] < 0.0)) + (count,))
    return out


def _assert_walks(got, want, rows, tag):
    out, rt, nc, re = got
    for k, e in enumerate(rows):
        w = want[k]
        assert _same(out[e], np.array(w[0])), (tag, e, w[4], out[e].tolist(), w[0])
        assert _same(rt[e:e + 1], np.array([w[1]])) and nc[e] == w[2] and re[e] == w[3], (tag, e, w[4], rt[e], nc[e], re[e], w[1:4])


_WALKS = {}


def _walks(ctx, name):
    if name not in _WALKS:
        from reak_amd import lib as L
        scn = SCENES[name][0]()
        scene = L.Scene(ctx, scn)
        sp, a, b, fraction = _walk_case(name, scene, scn, 200, seed=3)
        _WALKS[name] = (scene, sp, a, b, fraction)
    return _WALKS[name]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_backward_walk_is_the_twins_loop(ctx, name):
    from reak_amd import lib as L
    scene, sp, a, b, fraction = _walks(ctx, name)
    B = len(a)
    space = L.SvpSpace(sp.c_space(), scene=scene)
    back = [1] * B
    want = _twin_walks(sp, scene, a, b, fraction, back)
    whys = {}
    for w in want:
        whys[w[4]] = whys.get(w[4], 0) + 1
    print(name, whys, "most points", max(w[5] for w in want))
    # the classes the issue asks for: infinite pairs, an edge of T < min_interval, edges over one and over two passes
    assert whys.get("infeasible", 0) >= 3 and whys.get("zero", 0) >= 1 and whys.get("completed", 0) >= 10
    assert whys.get("bounds", 0) >= 1 and (scene.num_pairs == 0 or whys.get("collision", 0) >= 4)
    assert any(0.0 < w[1] < sp.min_interval for w in want)
    assert any(32 < w[5] <= 64 for w in want) and any(w[5] > 64 for w in want)   # points to test: over one pass, over two
    assert any(w[2] > 32 for w in want)                                          # and a walk that crosses a pass
    assert any(f == 1.0 for f in fraction) and any(f == 0.0 for f in fraction) and any(0.0 < f < 1.0 for f in fraction)
    _assert_walks(space.edge_check_back(a, b, fraction), want, range(B), (name, "fractions"))
    ones = np.ones(B)
    want1 = _twin_walks(sp, scene, a, b, ones, back)
    _assert_walks(space.edge_check_back(a, b, None), want1, range(B), (name, "NULL"))
    # every output but `out` may be NULL; B == 0 is fine
    lib = L.load()
    out = np.zeros((B, 2 * sp.n))
    st = lib.rkh_svp_edge_check_back(scene.h, C.byref(space.space), T.dptr(a), T.dptr(b), B, None, T.dptr(out), None, None, None)
    assert st == 0 and _same(out, np.array([w[0] for w in want1]))
    assert lib.rkh_svp_edge_check_back(scene.h, C.byref(space.space), None, None, 0, None, None, None, None, None) == 0
    assert lib.rkh_svp_edge_check_back(scene.h, C.byref(space.space), T.dptr(a), T.dptr(b), B, None, None, None, None, None) == -1


def test_mixed_launch_walks_each_row_in_its_direction(ctx):
    """B = 257 rows (two blocks of the solve kernel, the last with one lane) with alternating direction bytes: forward
    rows are rkh_svp_edge_check's, backward rows rkh_svp_edge_check_back's, bit for bit"""
    from reak_amd import lib as L
    scene, sp, a, b, fraction = _walks(ctx, "c2")
    idx = np.arange(257) % len(a)
    a2, b2, f2 = np.ascontiguousarray(a[idx]), np.ascontiguousarray(b[idx]), np.ascontiguousarray(fraction[idx])
    f2[200:] = 1.0 - f2[200:]   # the rows that come a second time, with another fraction
    back = (np.arange(257) % 2).astype(np.uint8)
    space = L.SvpSpace(sp.c_space(), scene=scene)
    fwd, bwd = space.edge_check(a2, b2, f2), space.edge_check_back(a2, b2, f2)
    mixed = space.edge_check_dir(a2, b2, back, f2)
    assert fwd[2].max() > 64 and bwd[2].max() > 64 and not _same(fwd[0], bwd[0])
    for e in range(257):
        ref = bwd if back[e] else fwd
        assert _same(mixed[0][e], ref[0][e]) and _same(mixed[1][e:e + 1], ref[1][e:e + 1]), e
        assert mixed[2][e] == ref[2][e] and mixed[3][e] == ref[3][e], e
    # all bytes 0, and no bytes at all, are the forward walk
    for bytes_ in (np.zeros(257, dtype=np.uint8), None):
        if bytes_ is None:
            lib = L.load()
            out = np.zeros((257, 2 * sp.n))
            assert lib.rkh_diag_svp_edge_check_dir(scene.h, C.byref(space.space), T.dptr(a2), T.dptr(b2), 257, T.dptr(f2), None,
                                                   T.dptr(out), None, None, None) == 0
        else:
            out = space.edge_check_dir(a2, b2, bytes_, f2)[0]
        assert _same(out, fwd[0])


def test_backward_walk_over_the_point_cap_is_a_capacity_error(ctx):
    from reak_amd import lib as L
    scene, sp, a, b, _ = _walks(ctx, "c2")
    fine = L.SvpSpace(R.Space(sp.n, sp.lower, sp.upper, 1e-7, sp.speed, sp.accel).c_space(), scene=scene)
    with pytest.raises(L.RkhError) as e:
        fine.edge_check_back(a[:8], b[:8])
    assert e.value.status == -6 and "1 048 576" in str(e.value)


# ---- the planner --------------------------------------------------------------------------------------------------------------
def make_walks(sp, scene):
    """The twins' walks with rkh_min_distance as the collision test: all points of the edge in one call"""
    has_pairs = scene.num_pairs > 0

    def walk_dir(a, b, f, back):
        Tt, peak = R.reach(sp, a, b)
        dist = []
        if Tt < math.inf and has_pairs:
            rows = [R.model_units(sp, R.point(sp, a, b, peak, Tt, d)) for d in RB.times_dir(sp, Tt, f, back)]
            if rows:
                dist = scene.min_distance(np.array(rows)).tolist()
        it = iter(dist)
        return RB.walk_dir(sp, a, b, f, back, (lambda x: not (next(it) < 0.0)) if has_pairs else (lambda x: True))

    return (lambda a, b, f: walk_dir(a, b, f, 0)), (lambda a, b, f: walk_dir(a, b, f, 1))


def c_params(problems):
    return [T.make_svp_rrt_params(p["start"], p["goal"], p["seed"], p["max_vertices"], p["max_iterations"], p["max_edge_time"],
                                  p["steer_tol"]) for p in problems]


def twin_refills(t):
    return -(-t["iterations"] // RR.WINDOW)


def assert_problem_is_the_twins(planner, i, status, want, tag):
    n0, n1, it, j0, j1 = status
    assert (n0[i], n1[i]) == (len(want["V"][0]), len(want["V"][1])), (tag, i, n0[i], n1[i], want["why"])
    assert it[i] == want["iterations"], (tag, i, it[i], want["iterations"])
    assert (j0[i], j1[i]) == (want["join"] if want["join"] is not None else (NO, NO)), (tag, i, j0[i], j1[i], want["join"])
    for side in (0, 1):
        tree = planner.tree(i, side)
        assert tree["parent"].tolist() == want["P"][side], (tag, i, side)
        assert _same(tree["vertices"], np.array(want["V"][side])), (tag, i, side)
        assert _same(tree["edge_time"], np.array(want["E"][side])), (tag, i, side)
    pts, dur = planner.solution(i)
    wpts, wdur = BR.solution(want)
    assert len(pts) == len(wpts) and (not wpts or _same(pts, np.array(wpts))), (tag, i)
    assert _same(np.array([dur]), np.array([wdur])), (tag, i, dur, wdur)


_C2 = {}


def _c2(ctx):
    """scene, space, the 36 shared problems and the twin's results, computed once"""
    if not _C2:
        from reak_amd import lib as L
        scn, sp, probs = BR.c2_inputs()
        scene = L.Scene(ctx, scn)
        walk, walk_back = make_walks(sp, scene)
        _C2["v"] = (scene, sp, probs, [BR.run(sp, walk, walk_back, p) for p in probs])
    return _C2["v"]


@pytest.mark.parametrize("P", [1, 3, 36])
def test_batch_is_the_twins_trees_bit_for_bit(ctx, P):
    from reak_amd import lib as L
    scene, sp, probs, want = _c2(ctx)
    BR.check_c2_conditions(want)
    pl = L.SvpBiRrt(scene, sp.c_space(), c_params(probs[:P]))
    assert pl.stats.vertices == 2 * P and pl.stats.rounds == 0 and not pl.finished
    st = pl.solve()
    assert st.problems_finished == P and pl.finished
    status = pl.status()
    for i in range(P):
        assert_problem_is_the_twins(pl, i, status, want[i], ("c2", P))
    assert st.iterations == sum(t["iterations"] for t in want[:P])
    assert st.vertices == sum(len(t["V"][0]) + len(t["V"][1]) for t in want[:P])
    assert st.window_refills == sum(twin_refills(t) for t in want[:P])
    assert st.rounds >= 1 and st.walk_passes >= 1 and st.tested_points > 0
    print("P", P, "rounds", st.rounds, "iterations", st.iterations, "vertices", st.vertices, "walk passes", st.walk_passes,
          "tested points", st.tested_points)
    pl.close()


def test_problem_of_the_batch_equals_the_same_parameters_alone(ctx):
    from reak_amd import lib as L
    scene, sp, probs, want = _c2(ctx)
    batch = L.SvpBiRrt(scene, sp.c_space(), c_params(probs))
    batch.solve()
    bs = batch.status()
    for i in (0, 4, 5, 19, 35):
        alone = L.SvpBiRrt(scene, sp.c_space(), c_params([probs[i]]))
        alone.solve()
        s1 = alone.status()
        assert [int(x[0]) for x in s1] == [int(x[i]) for x in bs], i
        for side in (0, 1):
            ta, tb = alone.tree(0, side), batch.tree(i, side)
            assert np.array_equal(ta["parent"], tb["parent"]) and _same(ta["vertices"], tb["vertices"]), (i, side)
            assert _same(ta["edge_time"], tb["edge_time"]), (i, side)
        (pa, da), (pb, db) = alone.solution(0), batch.solution(i)
        assert _same(pa, pb) and da == db, i
        alone.close()
    batch.close()


def test_without_iterations_a_problem_runs_on_vertex_targets_only(ctx):
    from reak_amd import lib as L
    scene, sp, probs, _ = _c2(ctx)
    mine = [dict(probs[k], max_iterations=0) for k in (0, 1, 3)]
    walk, walk_back = make_walks(sp, scene)
    want = [BR.run(sp, walk, walk_back, p) for p in mine]
    assert sum(t["br"][0]["committed"] + t["br"][1]["committed"] for t in want) >= 1
    assert all(t["iterations"] == 0 and t["why"] in ("max_iterations", "joined") for t in want)
    assert any(t["why"] == "max_iterations" and t["half_steps"] >= 2 for t in want)
    pl = L.SvpBiRrt(scene, sp.c_space(), c_params(mine))
    st = pl.solve()
    assert st.iterations == 0 and st.window_refills == 0 and st.problems_finished == len(mine)
    status = pl.status()
    for i in range(len(mine)):
        assert_problem_is_the_twins(pl, i, status, want[i], "no iterations")
    pl.close()


def test_trees_across_the_slice_boundary_of_the_nearest_sweep(ctx):
    """Free space: both trees of the long-box problem pass 256 vertices (two slices of the sweep) beside a problem with
    max_vertices 5 and one that joins in its first half step"""
    from reak_amd import lib as L
    scene = L.Scene(ctx, scenarios.make_hidim(3))
    assert scene.num_pairs == 0
    sp, big = BR.free_space_inputs()
    small = dict(big, seed=12, max_vertices=5)
    near = dict(big, seed=13, goal=[0.7, 0.0] * 3, max_vertices=9)
    probs = [big, small, near]
    walk, walk_back = make_walks(sp, scene)
    want = [BR.run(sp, walk, walk_back, p) for p in probs]
    t = want[0]
    assert (len(t["V"][0]), len(t["V"][1]), t["iterations"], t["join"]) == (377, 400, 65, None)
    assert RR.SLICE == 256 and min(len(t["V"][0]), len(t["V"][1])) > RR.SLICE   # both sweeps run over two slices
    assert want[1]["why"] == "max_vertices" and max(len(want[1]["V"][0]), len(want[1]["V"][1])) == 5
    assert want[2]["why"] == "joined" and want[2]["join"] == (0, 0) and want[2]["half_steps"] == 1
    assert R.reach(sp, near["start"], near["goal"])[0] <= near["max_edge_time"]
    pl = L.SvpBiRrt(scene, sp.c_space(), c_params(probs))
    pl.solve()
    status = pl.status()
    for i in range(3):
        assert_problem_is_the_twins(pl, i, status, want[i], "free space")
    pl.close()


def test_parents_from_the_second_slice_of_the_nearest_sweep_in_both_trees(ctx):
    """The long-box problem above fills both trees past 256 vertices, but its twin never picks a parent beyond index 32:
    each side re-extends one early vertex towards the other side's (unchanged) newest vertex.  So the second slice's minima
    are won here: the box [0, 4]^3 with max_edge_time 0.2, where the tree rooted in the middle of the box grows through
    samples -- problem 0 gives tree 0 a parent >= 256, problem 1 (start and goal near opposite corners) tree 1."""
    from reak_amd import lib as L
    scene = L.Scene(ctx, scenarios.make_hidim(3))
    sp = R.Space(3, [0.0] * 3, [4.0] * 3, 0.05)
    base = {"name": "box4", "max_vertices": 450, "max_iterations": 6000, "max_edge_time": 0.2, "steer_tol": 0.1}
    probs = [dict(base, seed=12, start=[2.0, 0.0] * 3, goal=[0.3, 0.0] * 3),
             dict(base, seed=13, start=[0.3, 0.0] * 3, goal=[3.7, 0.0] * 3)]
    walk, walk_back = make_walks(sp, scene)
    want = [BR.run(sp, walk, walk_back, p) for p in probs]
    assert len(want[0]["V"][0]) == 450 and max(want[0]["P"][0][1:]) >= RR.SLICE
    assert len(want[1]["V"][1]) == 450 and max(want[1]["P"][1][1:]) >= RR.SLICE
    assert all(t["iterations"] > 16 * RR.WINDOW for t in want)    # windows refilled on the way, on both sides' behalf
    pl = L.SvpBiRrt(scene, sp.c_space(), c_params(probs))
    st = pl.solve()
    status = pl.status()
    for i in range(2):
        assert_problem_is_the_twins(pl, i, status, want[i], "box4")
    assert st.window_refills == sum(twin_refills(t) for t in want)
    pl.close()


def test_one_round_at_a_time_gives_the_same_trees(ctx):
    from reak_amd import lib as L
    scene, sp, probs, _ = _c2(ctx)
    mine = probs[:6]
    whole = L.SvpBiRrt(scene, sp.c_space(), c_params(mine))
    ws = whole.solve()
    steps = L.SvpBiRrt(scene, sp.c_space(), c_params(mine))
    rounds = 0
    while not steps.finished:
        before = steps.stats.rounds
        st = steps.solve(1)
        rounds += 1
        assert st.rounds == before + 1 and rounds <= 4000
    st = steps.solve(1)   # nothing left: no round runs
    assert st.rounds == rounds == ws.rounds and rounds >= 10
    a, b = whole.status(), steps.status()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for i in range(len(mine)):
        for side in (0, 1):
            ta, tb = whole.tree(i, side), steps.tree(i, side)
            assert np.array_equal(ta["parent"], tb["parent"]) and _same(ta["vertices"], tb["vertices"]), (i, side)
            assert _same(ta["edge_time"], tb["edge_time"]), (i, side)
    assert (st.iterations, st.vertices, st.tested_points, st.walk_passes, st.window_refills, st.problems_finished) == (
        ws.iterations, ws.vertices, ws.tested_points, ws.walk_passes, ws.window_refills, ws.problems_finished)
    whole.close()
    steps.close()


def test_refusals_leave_no_planner_behind(ctx):
    from reak_amd import lib as L
    scene, sp, probs, _ = _c2(ctx)
    lib = L.load()
    good = c_params(probs[:1])[0]
    space = sp.c_space()

    def refused(space_, params, P, *words):
        h = C.c_void_p(0xDEAD)
        arr = (T.SvpRrtParams * max(len(params), 1))(*params)
        st = lib.rkh_svp_birrt_create_batch(scene.h, C.byref(space_), arr, P, C.byref(h))
        msg = lib.rkh_last_error().decode()
        assert st == -1 and h.value is None and all(w in msg for w in words), (st, h.value, msg, words)

    def changed(**kw):
        p = T.SvpRrtParams.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    refused(space, [changed(has_goal=0)], 1, "problem 0", "has_goal")
    refused(space, [good, changed(has_goal=0)], 2, "problem 1", "has_goal")
    out = T.SvpRrtParams.from_buffer_copy(good)
    out.goal[0] = 1.01 * sp.upper[0]
    refused(space, [good, good, out], 3, "problem 2", "goal", "bounds")
    nan = T.SvpRrtParams.from_buffer_copy(good)
    nan.goal[3] = math.inf
    refused(space, [nan], 1, "problem 0", "goal", "finite")
    refused(space, [changed(struct_size=C.sizeof(T.SvpRrtParams) - 8)], 1, "problem 0", "struct_size")
    small = sp.c_space()
    small.struct_size -= 8
    refused(small, [good], 1, "struct_size")
    # what the RRT's create refuses
    refused(space, [changed(max_vertices=0)], 1, "max_vertices")
    bad_start = T.SvpRrtParams.from_buffer_copy(good)
    bad_start.start[0] = 1.01 * sp.upper[0]
    refused(space, [bad_start], 1, "start", "bounds")
    refused(space, [good], 0, "16384")
    refused(space, [good] * 16385, 16385, "16384")
    with pytest.raises(L.RkhError):
        L.SvpBiRrt(scene, space, [changed(has_goal=0)])
    # a planner of a valid batch still comes up afterwards
    pl = L.SvpBiRrt(scene, space, [good])
    assert pl.solve().problems_finished == 1
    pl.close()
