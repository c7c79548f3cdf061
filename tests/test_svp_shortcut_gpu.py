"""rkh_svp_shortcut_paths on the device against its Python twin (tests/svp_shortcut_ref.py over tests/svp_ref.py and the
pair order of tests/shortcut_ref.py): keep, n_keep, n_blocked equal, time_in / time_out bit for bit.  The twin's collision
test is rkh_min_distance at the twin's own model-unit points, all points of all pairs in one call (_twin_walks of
tests/test_svp_space_gpu.py).  The arithmetic is fp64 with contraction off on both sides and the search adds in one fixed
order: a difference is a bug, not a tolerance to widen."""
import math
import os
import sys

import numpy as np
import pytest

import shortcut_ref as S
import svp_ref as R
import svp_shortcut_ref as SS
import test_svp_space_gpu as W   # its helpers: _limits, SCENES, _twin_walks, _same
from reak_amd import scenarios

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIL = 0xFFFFFFFF
LENGTHS = (1, 2, 3, 33, 257)
SPANS = (0, 0, 0, 0, 8)   # 257 points at span 8: the fourth thread slot and the 256 boundary of the search are crossed
SEED = 1                  # the first seed, counting up from 1, at which check_conditions holds


@pytest.fixture(scope="module")
def ctx():
    from reak_amd import lib as L
    return L.Context(0)


def scene_space(name, n, min_interval=0.06):
    """the space of the walk tests (tests/test_svp_space_gpu.py) for a scene kind"""
    half = W.SCENES[name][1]
    speed, accel = W._limits(n)
    unit = R.Space(n, [0.0] * n, [1.0] * n, 1.0, speed, accel)
    if name == "hidim3":
        lower, upper = [0.0] * n, [1.0 / s for s in unit.speed]
    else:
        lower, upper = [-half / s for s in unit.speed], [half / s for s in unit.speed]
    return R.Space(n, lower, upper, min_interval, speed, accel)


def rest_configurations(sp, scene, rng, count=4000):
    """(free, hit): points at rest inside 0.8 of the box, clear of the obstacles by 0.05 / colliding (hit is empty for a scene
    without proxy pairs)"""
    n = sp.n
    lo, hi = np.array(sp.lower), np.array(sp.upper)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rest = np.zeros((count, 2 * n))
    rest[:, 0::2] = rng.uniform(mid - 0.8 * half, mid + 0.8 * half, size=(count, n))
    if scene.num_pairs == 0:
        return rest, rest[:0]
    d = scene.min_distance(np.array([R.model_units(sp, x) for x in rest.tolist()]))
    return rest[d > 0.05], rest[d < 0.0]


def random_walk(sp, rng, L, free, hit, p_hit=0.08, p_jump=0.08, p_tiny=0.05, p_move=0.5, p_edge=0.04):
    """L in-bounds points: small steps from a free configuration, at rest or moving; now and then a step placed on a
    colliding configuration, a jump to another free one (a long walk), a step shorter than min_interval's travel, and a
    fast point near the edge of the box (walks from and to it leave the bounds)."""
    n = sp.n
    lo, hi, vm = np.array(sp.lower), np.array(sp.upper), np.array(sp.vm)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    pts = [free[rng.integers(len(free))].copy()]
    while len(pts) < L:
        x = pts[-1].copy()
        u = rng.uniform()
        x[1::2] = 0.0
        if u < p_hit and len(hit):
            x = hit[rng.integers(len(hit))].copy()
        elif u < p_hit + p_jump:
            x = free[rng.integers(len(free))].copy()
        elif u < p_hit + p_jump + p_tiny:
            x[0::2] += 1e-4 * half * rng.uniform(-1, 1, n)
        elif u < p_hit + p_jump + p_tiny + p_edge:
            x[0::2] = mid + 0.93 * half * rng.choice([-1.0, 1.0], n)
            x[1::2] = 0.2 * vm * rng.uniform(-1, 1, n)
        else:
            x[0::2] = np.clip(x[0::2] + 0.15 * half * rng.uniform(-1, 1, n), mid - 0.8 * half, mid + 0.8 * half)
            if rng.uniform() < p_move:
                x[1::2] = 0.5 * vm * rng.uniform(-1, 1, n)
        if not R.in_bounds(sp, x.tolist()):
            x[1::2] = 0.0
        assert R.in_bounds(sp, x.tolist())
        pts.append(x)
    return np.array(pts)


def make_paths(sp, scene, seed):
    """the five paths of LENGTHS; the 2-point one runs from a free configuration into a colliding one"""
    rng = np.random.default_rng(seed)
    free, hit = rest_configurations(sp, scene, rng)
    assert len(free) >= 4 and len(hit) >= 4
    paths = [random_walk(sp, rng, L, free, hit) for L in LENGTHS]
    paths[1] = np.array([free[0], hit[0]])
    return paths


def twin_all_pairs(sp, scene, paths, spans):
    """per path: (T, reached, why) of every candidate pair under its span, all points of all pairs of all paths through
    ONE rkh_min_distance call"""
    a, b, count = [], [], []
    for path, span in zip(paths, spans):
        pa, pb = SS.pair_rows(path.tolist(), span)
        a.extend(pa), b.extend(pb), count.append(len(pa))
    if not a:
        return [(np.zeros(0), np.zeros(0, dtype=np.uint8), []) for _ in paths]
    walks = W._twin_walks(sp, scene, np.array(a), np.array(b), np.ones(len(a)), scene.num_pairs > 0)
    out, first = [], 0
    for c in count:
        w = walks[first:first + c]
        out.append((np.array([x[1] for x in w]), np.array([x[3] for x in w], dtype=np.uint8), [(x[4], x[2]) for x in w]))
        first += c
    return out


def twin_results(paths, spans, walks):
    return [SS.from_walks(len(p), s, w[0], w[1]) for p, s, w in zip(paths, spans, walks)]


def check_conditions(paths, walks, want):
    """what the issue asks of the inputs, on the twin's values"""
    whys = [x for w in walks for x in w[2]]
    kinds = {k for k, _ in whys}
    assert {"completed", "collision", "bounds", "infeasible", "zero"} <= kinds, kinds
    assert max(nc for _, nc in whys) > 2 * W.PASS          # a walk longer than two passes
    Ls = [len(p) for p in paths]
    assert any(2 < len(r["keep"]) < L for r, L in zip(want, Ls))
    assert any(len(r["keep"]) == 2 for r in want)
    assert any(r["keep"] == list(range(L)) for r, L in zip(want, Ls))
    assert any(r["n_blocked"] > 0 for r in want)
    assert all(r["time_out"] <= r["time_in"] for r in want)


def restricted(path, walk, span):
    """the all-pairs walks of a path cut down to a smaller span"""
    T, re = S.restrict(len(path), span, walk[1], walk[0])[::-1]
    return (T, re, [])


def assert_is_the_twins(got, want, tag):
    keep, t_in, t_out, n_blocked = got
    assert len(keep) == len(want), tag
    for b, r in enumerate(want):
        assert keep[b].tolist() == r["keep"], (tag, b, keep[b].tolist()[:12], r["keep"][:12])
        assert int(n_blocked[b]) == r["n_blocked"], (tag, b, n_blocked[b], r["n_blocked"])
        assert W._same(np.array([t_in[b], t_out[b]]), np.array([r["time_in"], r["time_out"]])), \
            (tag, b, t_in[b], r["time_in"], t_out[b], r["time_out"])


_C2 = {}


def _c2(ctx):
    """scene, space, the five paths, the twin's walks and results, and the mixed batch at span 8; computed once"""
    if not _C2:
        from reak_amd import lib as L
        scn = scenarios.make_c2(world_seed=1)
        scene = L.Scene(ctx, scn)
        sp = scene_space("c2", scn.n_dof)
        paths = make_paths(sp, scene, SEED)
        walks = twin_all_pairs(sp, scene, paths, SPANS)
        want = twin_results(paths, SPANS, walks)
        # the mixed batch runs at span 8: the 33-point path's candidates are a subset of its all-pairs walks
        mixed_walks = [restricted(p, w, 8) if len(p) == 33 else w for p, w in zip(paths, walks)]
        mixed = twin_results(paths, [8] * len(paths), mixed_walks)
        _C2["v"] = (scene, sp, paths, walks, want, mixed)
    return _C2["v"]


def test_c2_paths_are_the_twins_bit_for_bit(ctx):
    from reak_amd import lib as L
    scene, sp, paths, walks, want, mixed = _c2(ctx)
    check_conditions(paths, walks, want)
    print("c2:", [(len(p), len(r["keep"]), r["n_blocked"], r["time_in"], r["time_out"]) for p, r in zip(paths, want)])
    space = L.SvpSpace(sp.c_space(), scene=scene)
    for k, (path, span) in enumerate(zip(paths, SPANS)):
        assert_is_the_twins(space.shortcut_paths([path], span), [want[k]], ("alone", len(path)))
    assert_is_the_twins(space.shortcut_paths(paths[:4], 0), want[:4], "span 0")
    got = space.shortcut_paths(paths, 8)
    assert_is_the_twins(got, mixed, "mixed")
    assert mixed[3]["keep"] != want[3]["keep"] or mixed[3]["time_out"] >= want[3]["time_out"]
    # the slots of keep behind n_keep hold 0xFFFFFFFF, and time_in / n_blocked may be NULL
    import ctypes as C
    from reak_amd import types as T
    pts, path_ptr = L._path_table(paths, 2 * sp.n)
    keep, n_keep, t_out = np.zeros(len(pts), dtype=np.uint32), np.zeros(5, dtype=np.uint32), np.zeros(5)
    st = space.lib.rkh_svp_shortcut_paths(scene.h, C.byref(space.space), T.dptr(pts), T.u32ptr(path_ptr), 5, 8, T.u32ptr(keep),
                                          T.u32ptr(n_keep), None, T.dptr(t_out), None)
    assert st == 0 and W._same(t_out, got[2])
    for b in range(5):
        row = keep[path_ptr[b]:path_ptr[b + 1]]
        assert row[:n_keep[b]].tolist() == mixed[b]["keep"] and (row[n_keep[b]:] == NIL).all()


def test_infinite_hops(ctx):
    """A middle point faster than vm: nothing reaches it and it reaches nothing.  Bypassed, it is dropped; as the goal of a
    2-point path it makes the path no trajectory.  The neighbours in the batch are served as they are alone."""
    from reak_amd import lib as L
    scene, sp, paths, walks, want, _ = _c2(ctx)
    rng = np.random.default_rng(7)
    free, _ = rest_configurations(sp, scene, rng)
    a, c = free[0], free[0].copy()
    c[0::2] += 0.002 * (np.array(sp.upper) - np.array(sp.lower))   # (inside a's clearance of 0.05)
    fast = 0.5 * (a + c)
    fast[1] = 1.5 * sp.vm[0]
    mine = [paths[2], np.array([a, fast, c]), np.array([a, fast]), paths[3], np.array([fast])]
    spans = [0] * 5
    tw = twin_all_pairs(sp, scene, mine, spans)
    exp = twin_results(mine, spans, tw)
    assert math.isinf(tw[1][0][0]) and math.isinf(tw[1][0][2]) and tw[1][1][1] == 1    # only a -> c is finite, and free
    assert exp[1]["keep"] == [0, 2] and math.isinf(exp[1]["time_in"]) and exp[1]["time_out"] < math.inf
    assert exp[2] == {"keep": [], "time_in": math.inf, "time_out": math.inf, "n_blocked": 0}
    assert exp[4]["keep"] == [0] and exp[4]["time_out"] == 0.0
    assert exp[0] == want[2] and exp[3] == want[3]
    space = L.SvpSpace(sp.c_space(), scene=scene)
    got = space.shortcut_paths(mine)
    assert_is_the_twins(got, exp, "infinite")
    # the raw arrays of the path without a trajectory
    import ctypes as C
    from reak_amd import types as T
    pts, path_ptr = L._path_table(mine, 2 * sp.n)
    keep, n_keep, nb = np.zeros(len(pts), dtype=np.uint32), np.full(5, 9, dtype=np.uint32), np.full(5, 9, dtype=np.uint32)
    t_in, t_out = np.zeros(5), np.zeros(5)
    st = space.lib.rkh_svp_shortcut_paths(scene.h, C.byref(space.space), T.dptr(pts), T.u32ptr(path_ptr), 5, 0, T.u32ptr(keep),
                                          T.u32ptr(n_keep), T.dptr(t_in), T.dptr(t_out), T.u32ptr(nb))
    assert st == 0 and n_keep[2] == 0 and nb[2] == 0 and math.isinf(t_out[2]) and math.isinf(t_in[2])
    assert (keep[path_ptr[2]:path_ptr[3]] == NIL).all()
    assert keep[path_ptr[1]:path_ptr[2]].tolist() == [0, 2, NIL] and n_keep[1] == 2


@pytest.mark.parametrize("chunk_pairs", [1, 7, 500])
def test_chunks_do_not_change_the_result(ctx, chunk_pairs):
    """chunk boundaries inside a path's rows (1, 7: the rows hold 8 pairs) and between paths"""
    from reak_amd import lib as L
    scene, sp, paths, _, _, _ = _c2(ctx)
    space = L.SvpSpace(sp.c_space(), scene=scene)
    whole = space.shortcut_paths(paths, 8)
    parts = space.shortcut_paths(paths, 8, chunk_pairs=chunk_pairs)
    n_pairs = sum(len(S.pairs(len(p), 8)) for p in paths)
    assert n_pairs > 500 and n_pairs % 7 != 0 and n_pairs % 500 != 0
    for b in range(len(paths)):
        assert np.array_equal(whole[0][b], parts[0][b]), (chunk_pairs, b)
    assert W._same(whole[1], parts[1]) and W._same(whole[2], parts[2]) and np.array_equal(whole[3], parts[3])


@pytest.mark.parametrize("name", ["c1_planar", "track", "c4_meshes", "hidim3"])
def test_scene_kinds_against_the_existing_entries(ctx, name):
    """4 paths of 17 points: the entry equals the twin's search fed with reach_time and reached of ONE rkh_svp_edge_check
    call over the host-gathered pairs"""
    from reak_amd import lib as L
    scn = W.SCENES[name][0]()
    scene = L.Scene(ctx, scn)
    sp = scene_space(name, scn.n_dof)
    rng = np.random.default_rng(5)
    free, hit = rest_configurations(sp, scene, rng)
    paths = [random_walk(sp, rng, 17, free, hit, p_hit=0.15) for _ in range(4)]
    space = L.SvpSpace(sp.c_space(), scene=scene)
    a, b, count = [], [], []
    for p in paths:
        pa, pb = SS.pair_rows(p.tolist(), 0)
        a.extend(pa), b.extend(pb), count.append(len(pa))
    _, rt, _, reached = space.edge_check(np.array(a), np.array(b))
    assert W._same(rt, space.reach_time(np.array(a), np.array(b), peaks=False))   # the weight is rkh_svp_reach_time's
    exp, first = [], 0
    for p, c in zip(paths, count):
        exp.append(SS.from_walks(len(p), 0, rt[first:first + c], reached[first:first + c]))
        first += c
    print(name, [(len(r["keep"]), r["n_blocked"], r["time_in"], r["time_out"]) for r in exp], "reached", int(reached.sum()),
          "of", len(reached))
    assert 0 < reached.sum() and (scene.num_pairs == 0 or reached.sum() < len(reached))
    assert any(len(r["keep"]) < 17 for r in exp)
    assert_is_the_twins(space.shortcut_paths(paths), exp, name)


def test_planner_solutions(ctx):
    """the solved problems of the first 10 C2 problems of tests/test_svp_rrt_gpu.py, shortcut in one call"""
    from reak_amd import lib as L
    import test_svp_rrt_gpu as P
    scn, sp, probs = P.c2_problems()
    probs = probs[:10]
    scene = L.Scene(ctx, scn)
    pl = L.SvpRrt(scene, sp.c_space(), P.c_params(probs))
    pl.solve()
    _, _, gp = pl.status()
    solved = [i for i in range(10) if gp[i] != NIL]
    assert len(solved) >= 2
    cut = pl.shortcut_solutions()
    assert sorted(cut) == solved
    paths = [cut[i]["points"] for i in solved]
    assert max(len(p) for p in paths) >= 4
    tw = twin_all_pairs(sp, scene, paths, [0] * len(paths))
    exp = twin_results(paths, [0] * len(paths), tw)
    space = L.SvpSpace(sp.c_space(), scene=scene)
    hops_a, hops_b, owner = [], [], []
    for k, i in enumerate(solved):
        c, r = cut[i], exp[k]
        assert c["keep"].tolist() == r["keep"] and c["n_blocked"] == r["n_blocked"], (i, c["keep"], r["keep"])
        assert W._same(np.array([c["time_in"], c["time_out"]]), np.array([r["time_in"], r["time_out"]])), i
        assert c["time_out"] <= c["time_in"]
        # the planner's duration sums the stored edge times in path order; where the re-summed hop times have its bits
        # (asserted on the twin), time_in has them too
        if W._same(np.array([r["time_in"]]), np.array([c["duration"]])):
            assert W._same(np.array([c["time_in"]]), np.array([c["duration"]])), i
        print("problem", i, "points", len(c["points"]), "kept", len(c["keep"]), "blocked", c["n_blocked"], "duration",
              c["duration"], "time_in", c["time_in"], "time_out", c["time_out"])
        if c["n_blocked"] == 0:
            kept = c["points"][c["keep"]]
            hops_a.extend(kept[:-1]), hops_b.extend(kept[1:]), owner.extend([i] * (len(kept) - 1))
    if hops_a:
        _, _, _, reached = space.edge_check(np.array(hops_a), np.array(hops_b))
        assert reached.all(), [owner[e] for e in np.flatnonzero(reached == 0)]
    pl.close()


def test_refusals_that_need_the_device(ctx):
    from reak_amd import lib as L
    scene, sp, paths, _, want, _ = _c2(ctx)
    space = L.SvpSpace(sp.c_space(), scene=scene)
    long_path = np.repeat(paths[0], 1025, axis=0)
    with pytest.raises(L.RkhError) as e:
        space.shortcut_paths([paths[2], long_path], 1)
    assert e.value.status == -6 and "1024" in str(e.value)
    assert_is_the_twins(space.shortcut_paths([np.repeat(paths[0], 1024, axis=0)], 1),
                        [{"keep": list(range(1024)), "time_in": 0.0, "time_out": 0.0, "n_blocked": 0}], "1024 points")
    fine = L.SvpSpace(R.Space(sp.n, sp.lower, sp.upper, 1e-7, sp.speed, sp.accel).c_space(), scene=scene)
    with pytest.raises(L.RkhError) as e:
        fine.shortcut_paths([paths[2], paths[1]])   # (the 2-point path: rest to rest across the box, seconds of travel)
    assert e.value.status == -6 and "1 048 576" in str(e.value)
    three = L.SvpSpace(R.Space(3, [-1.0] * 3, [1.0] * 3, 0.05).c_space(), scene=scene)
    with pytest.raises(L.RkhError) as e:
        three.shortcut_paths([np.zeros((2, 6))])
    assert e.value.status == -1 and "n_dof" in str(e.value)
    # the context still serves a valid call
    assert_is_the_twins(space.shortcut_paths([paths[2]]), [want[2]], "after the refusals")
