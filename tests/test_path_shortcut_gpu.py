"""Path shortcutting on the GPU against tests/shortcut_ref.py (the sequential double loop of include/rkh.h, verdicts from
the oracle's quasi-static walk).  Every comparison is bit for bit:
 (a) the search kernel alone through rkh_diag_shortcut_dp on verdict / weight matrices no scene produces: lengths at the
     wave, workgroup and register-slot edges, spans 0, 1, 2, 5 and L, all ok, none ok, Bernoulli, exact ties, blocked input
     hops that no detour replaces, and one launch that mixes L = 1, 2, 65 and 1024;
 (b) rkh_shortcut_paths on a 3D and on a planar scene (they walk in different kernels), two path sets in one call;
 (c) planner paths: a PRM solution, three multi-query answers with their off-roadmap points, an RRT* solution;
 (d) arguments, capacity, B == 0, a rate-limited space; (e) the C++ adaptor's shortcut_path()."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import shortcut_ref as S
from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1024)
BAD, CAPACITY = -1, -6


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------ (a) the search kernel
def _family(name, n_pts, max_span, rng):
    """(ok, w) per candidate pair of a path of n_pts points"""
    pr = S.pairs(n_pts, max_span)
    n = len(pr)
    w = rng.uniform(0.1, 1.0, n)
    if name == "all_ok":
        ok = np.ones(n, dtype=np.uint8)
    elif name == "none_ok":
        ok = np.zeros(n, dtype=np.uint8)
    elif name == "bernoulli":
        ok = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    elif name == "ties":      # multiples of 0.25: every sum is exact, equal-cost routes abound
        ok = (rng.uniform(size=n) < 0.6).astype(np.uint8)
        w = 0.25 * rng.integers(1, 8, n).astype(np.float64)
    elif name == "blocked":   # no verdict is true across the hop (c, c + 1): every route takes that blocked input hop
        ok = (rng.uniform(size=n) < 0.5).astype(np.uint8)
        c = (n_pts - 1) // 2
        for k, (i, j) in enumerate(pr):
            if i <= c < j:
                ok[k] = 0
    return ok, w


FAMILIES = ("all_ok", "none_ok", "bernoulli", "ties", "blocked")


@pytest.mark.parametrize("name", FAMILIES)
def test_search_kernel_matches_the_double_loop(L, ctx, name):
    rng = np.random.default_rng(FAMILIES.index(name) + 20)
    for n_pts in LENGTHS:
        for max_span in (0, 1, 2, 5, n_pts):
            ok, w = _family(name, n_pts, max_span, rng)
            rk, rc, rb = S.dp_rows(n_pts, max_span, ok, w)
            if name == "none_ok":
                assert rk == list(range(n_pts)) and rb == n_pts - 1     # the input, every hop of it blocked
            if name == "blocked" and n_pts >= 2:
                assert rb > 0
            keep, cost, nb = L.diag_shortcut_dp(ctx, [n_pts], ok, w, max_span)
            assert list(keep[0]) == rk, (name, n_pts, max_span)
            assert _bits(cost[0]) == _bits(rc) and nb[0] == rb, (name, n_pts, max_span, cost[0], rc, nb[0], rb)


def test_planted_tie_resolves_to_the_lowest_predecessor(L, ctx):
    from test_path_shortcut_cpu import planted_tie

    ok, w = planted_tie(8)
    keep, cost, nb = L.diag_shortcut_dp(ctx, [8], ok, w, 0)
    assert (list(keep[0]), cost[0], nb[0]) == ([0, 1, 5, 7], 2.5, 0)
    # the same tie in every path of a launch, behind paths of other lengths
    lens = [8, 1, 8, 2, 8]
    oks = [ok, [], ok, [0], ok]
    ws = [w, [], w, [0.75], w]
    keep, cost, nb = L.diag_shortcut_dp(ctx, lens, np.concatenate([np.asarray(o, dtype=np.uint8) for o in oks]),
                                        np.concatenate([np.asarray(x, dtype=np.float64) for x in ws]), 0)
    assert [list(k) for k in keep] == [[0, 1, 5, 7], [0], [0, 1, 5, 7], [0, 1], [0, 1, 5, 7]]
    assert cost.tolist() == [2.5, 0.0, 2.5, 0.75, 2.5] and nb.tolist() == [0, 0, 0, 1, 0]


@pytest.mark.parametrize("max_span", [0, 5])
def test_one_launch_mixes_lengths(L, ctx, max_span):
    rng = np.random.default_rng(31 + max_span)
    lens = [1, 2, 65, 1024, 2, 1, 257]
    fam = [_family("bernoulli", n, max_span, rng) for n in lens]
    ref = [S.dp_rows(n, max_span, ok, w) for n, (ok, w) in zip(lens, fam)]
    keep, cost, nb = L.diag_shortcut_dp(ctx, lens, np.concatenate([f[0] for f in fam]), np.concatenate([f[1] for f in fam]),
                                        max_span)
    for b, (rk, rc, rb) in enumerate(ref):
        assert list(keep[b]) == rk and _bits(cost[b]) == _bits(rc) and nb[b] == rb, (b, lens[b])


# ------------------------------------------------------------------------------------------ (b) scenes
def free_points(osc, lo, hi):
    pts = np.random.default_rng(4).uniform(lo, hi, (4000, 3))
    x = np.zeros((len(pts), 6))
    x[:, 0::2] = pts
    return pts[osc.min_distance(x) > 1e-3]


def walk_paths(osc, lo, hi, free, n_paths=8, n_pts=33, sigma=0.6, seed=6):
    """Gaussian random walks over free points from free[192 + p]; a step out of the box or not free is drawn again"""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(n_paths):
        path = [free[192 + p].copy()]
        while len(path) < n_pts:
            c = path[-1] + rng.normal(0.0, sigma, 3)
            if (c < lo).any() or (c > hi).any():
                continue
            x = np.zeros((1, 6))
            x[0, 0::2] = c
            if osc.min_distance(x)[0] > 1e-3:
                path.append(c)
        out.append(np.array(path))
    return out


def _same(got, refs, what):
    keep, cost_in, cost_out, n_blocked = got
    assert len(keep) == len(refs)
    for b, r in enumerate(refs):
        assert list(keep[b]) == r["keep"], (what, b, list(keep[b]), r["keep"])
        assert _bits(cost_in[b]) == _bits(r["cost_in"]) and _bits(cost_out[b]) == _bits(r["cost_out"]), (what, b)
        assert n_blocked[b] == r["n_blocked"], (what, b)
        assert cost_out[b] <= cost_in[b], (what, b)


@pytest.mark.parametrize("kind", ["3d", "planar"])
def test_scene_paths_match_the_oracle_made_reference(L, ctx, oracle, kind):
    scn = (scenarios.make_c1 if kind == "3d" else scenarios.make_c1_planar)(world_seed=1, n_obstacles=40)
    sc, osc = L.Scene(ctx, scn), oracle.OracleScene(scn)
    lo, hi, mi = np.asarray(scn.meta["lower"]), np.asarray(scn.meta["upper"]), scn.meta["min_interval"]
    free = free_points(osc, lo, hi)
    sets = {"U": [free[12 * p:12 * p + 12] for p in range(16)], "W": walk_paths(osc, lo, hi, free)}
    full = {k: [S.strict_verdicts(osc, lo, hi, mi, p, 0) for p in paths] for k, paths in sets.items()}
    refs = {ms: {k: [S.reference(osc, lo, hi, mi, p, ms, full=f) for p, f in zip(paths, full[k])] for k, paths in sets.items()}
            for ms in (0, 3)}
    # the reference itself is worth comparing with: some shortcuts, not all, blocked and clean answers
    for k, paths in sets.items():
        nc_ok = nc = c_ok = 0
        for p, (ok, _) in zip(paths, full[k]):
            for (i, j), o in zip(S.pairs(len(p), 0), ok):
                nc += j > i + 1
                nc_ok += int(o) if j > i + 1 else 0
                c_ok += int(o) if j == i + 1 else 0
        r0 = refs[0][k]
        print(kind, k, "non-consecutive ok", nc_ok, "of", nc, "consecutive ok", c_ok, "removed",
              sorted(len(p) - len(r["keep"]) for p, r in zip(paths, r0)))
        assert 0.05 <= nc_ok / nc <= 0.60
        assert len({len(r["keep"]) for r in r0}) >= 3
        assert any(r["n_blocked"] > 0 for r in r0) and any(r["n_blocked"] == 0 for r in r0)
        if k == "U":    # the figures the oracle alone gives for this set
            assert (nc_ok, nc, c_ok) == (97, 880, 26)
    qs = L.make_qs_space(3, lo, hi, mi)
    paths = sets["U"] + sets["W"]                          # both sets in one call
    for ms in (0, 3):
        got = sc.shortcut_paths(qs, paths, ms)
        _same(got, refs[ms]["U"] + refs[ms]["W"], (kind, ms))
        again = sc.shortcut_paths(qs, paths, ms)           # a rerun gives identical output
        assert all(np.array_equal(a, b) for a, b in zip(got[0], again[0]))
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got[1:3], again[1:3])) and np.array_equal(got[3], again[3])
    # a path alone equals its answer in the batch
    one = sc.shortcut_paths(qs, [sets["W"][3]], 0)
    _same(one, [refs[0]["W"][3]], (kind, "alone"))


# ------------------------------------------------------------------------------------------ (c) planner paths
def test_planner_paths(L, ctx, oracle):
    c1 = scenarios.make_c1(world_seed=1)
    lo, hi, mi = c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"]
    sc, osc = L.Scene(ctx, c1), oracle.OracleScene(c1)
    qs = L.make_qs_space(3, lo, hi, mi)
    pl = L.PrmPlanner(sc, c1.prm_params(seed=1, max_vertices=800, sampling_radius=1.0), qs)
    st = pl.solve_planning_query()
    assert st.num_vertices >= 800
    pos = pl.graph()["pos"]
    path, cost = pl.solution()
    assert len(path) >= 2 and np.isfinite(cost)
    paths = [L.path_points(pos, path)]
    # three multi-query answers, their off-roadmap start and goal in front and behind
    pts = np.random.default_rng(4).uniform(lo, hi, size=(600, 3))
    x = np.zeros((len(pts), 6))
    x[:, 0::2] = pts
    free = pts[osc.min_distance(x) > 1e-3]
    starts, goals = free[:40], free[40:80]
    qcost, qpaths = pl.query_paths(starts, goals, 6, 0.6)
    found = [b for b in range(40) if np.isfinite(qcost[b])][:3]
    assert len(found) == 3
    for b in found:
        paths.append(L.path_points(pos, qpaths[b], start=starts[b], goal=goals[b]))
        assert len(paths[-1]) == len(qpaths[b]) + 2
    pl.close()
    star = L.RrtStarPlanner(sc, c1.rrt_params(seed=1, max_vertices=1200), qs)
    sst = star.solve_planning_query()
    spath, _ = star.solution()
    assert sst.num_solutions > 0 and len(spath) >= 2
    paths.append(L.path_points(star.graph()["pos"], spath))
    star.close()
    refs = [S.reference(osc, lo, hi, mi, p, 0) for p in paths]
    got = sc.shortcut_paths(qs, paths)
    print("planner paths: points", [len(p) for p in paths], "kept", [len(k) for k in got[0]], "n_blocked", got[3].tolist())
    _same(got, refs, "planner")          # (equality and cost_out <= cost_in; n_blocked is whatever conn_tol let through)
    assert _bits(got[1][0]) != _bits(0.0)


# ------------------------------------------------------------------------------------------ (d) arguments
def test_arguments_capacity_and_empty_batch(L, ctx):
    c1 = scenarios.make_c1(world_seed=1)
    sc = L.Scene(ctx, c1)
    lo, hi, mi = c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"]
    qs = L.make_qs_space(3, lo, hi, mi)
    lib, h = sc.lib, sc.h
    pts = np.zeros((4, 3))
    pts[:, 0] = [0.0, 0.01, 0.02, 0.03]
    pp = np.array([0, 4], dtype=np.uint32)
    keep, nk, nb = np.full(8, 0xABCD, dtype=np.uint32), np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    cin, cout = np.zeros(2), np.zeros(2)

    def call(scene=h, space=qs, points=pts, path_ptr=pp, B=1, ms=0, k=keep, n=nk, ci=cin, co=cout, b=nb):
        return lib.rkh_shortcut_paths(scene, C.byref(space) if space is not None else None,
                                      T.dptr(points) if points is not None else None,
                                      T.u32ptr(path_ptr) if path_ptr is not None else None, B, ms,
                                      T.u32ptr(k) if k is not None else None, T.u32ptr(n) if n is not None else None,
                                      T.dptr(ci) if ci is not None else None, T.dptr(co) if co is not None else None,
                                      T.u32ptr(b) if b is not None else None)

    assert call() == 0 and nk[0] == 2 and keep[:2].tolist() == [0, 3]    # hops below min_interval
    assert (keep[2:4] == 0xFFFFFFFF).all() and (keep[4:] == 0xABCD).all()   # unused slots of the path; nothing behind it
    assert call(ci=None, b=None) == 0                                                         # the optional outputs
    for kw in ({"scene": None}, {"space": None}, {"points": None}, {"path_ptr": None}, {"k": None}, {"n": None}, {"co": None}):
        assert call(**kw) == BAD, kw
    assert call(path_ptr=np.array([1, 4], dtype=np.uint32)) == BAD                            # not from 0
    assert call(path_ptr=np.array([0, 2, 2, 4], dtype=np.uint32), B=3) == BAD                 # an empty path
    assert call(path_ptr=np.array([0, 3, 2], dtype=np.uint32), B=2) == BAD                    # not ascending
    assert call(space=L.make_qs_space(2, lo, hi, mi)) == BAD                                  # n_dof
    assert call(space=L.make_qs_space(3, lo, hi, 0.0)) == BAD                                 # min_interval
    bad = pts.copy()
    bad[2, 1] = np.nan
    assert call(points=bad) == BAD
    for B0 in ({"B": 0}, {"B": 0, "points": None, "path_ptr": None, "k": None, "n": None, "co": None}):
        assert call(**B0) == 0                                                                # B == 0
    # capacity: 1025 points, refused before anything is launched or written
    big = np.zeros((1025, 3))
    big[:, 0] = np.linspace(0.0, 1.0, 1025)
    bk = np.full(1025, 0xABCD, dtype=np.uint32)
    assert call(points=big, path_ptr=np.array([0, 1025], dtype=np.uint32), k=bk) == CAPACITY
    assert (bk == 0xABCD).all() and b"1024" in lib.rkh_last_error()
    assert call(points=big, path_ptr=np.array([0, 1024], dtype=np.uint32), k=bk, ms=2) == 0
    assert bk[0] == 0 and bk[1024] == 0xABCD
    # more candidate pairs than one call takes: 4101 paths of 1024 points, all pairs (4100 fit: 2 147 481 600 pairs)
    n_paths = 4101
    huge_ptr = (np.arange(n_paths + 1, dtype=np.uint64) * 1024).astype(np.uint32)
    huge = np.zeros((n_paths * 1024, 3))                   # (never read: the count is taken from path_ptr first)
    hk, hn, hc = np.zeros(n_paths * 1024, dtype=np.uint32), np.zeros(n_paths, dtype=np.uint32), np.zeros(n_paths)
    assert call(points=huge, path_ptr=huge_ptr, B=n_paths, k=hk, n=hn, ci=None, co=hc, b=None) == CAPACITY
    assert b"2147483647" in lib.rkh_last_error()
    # the diagnostic entry: the same layout rules, and its weights
    ok1, w1 = np.ones(6, dtype=np.uint8), np.full(6, 0.5)
    with pytest.raises(L.RkhError):
        L.diag_shortcut_dp(ctx, [1025], np.ones(1, dtype=np.uint8), np.ones(1), 1)
    with pytest.raises(L.RkhError):
        L.diag_shortcut_dp(ctx, [4, 0], ok1, w1, 0)
    with pytest.raises(L.RkhError):
        L.diag_shortcut_dp(ctx, [4], ok1, -w1, 0)
    with pytest.raises(L.RkhError):
        L.diag_shortcut_dp(ctx, [4], ok1, w1 * np.inf, 0)
    assert L.diag_shortcut_dp(ctx, [], [], [], 0)[0] == []


def test_rate_limited_space_reaches_the_walk(L, ctx, oracle):
    """The same points under speed limits (2, 1, 0.5): the model is posed at point * limit, so the verdicts change and
    follow the oracle's rate-limited space."""
    scn = scenarios.make_c1(world_seed=1, n_obstacles=40)
    sc, osc = L.Scene(ctx, scn), oracle.OracleScene(scn)
    speed = np.array([2.0, 1.0, 0.5])
    lo, hi, mi = np.asarray(scn.meta["lower"]), np.asarray(scn.meta["upper"]), scn.meta["min_interval"]
    free = free_points(osc, lo, hi)
    paths = [free[12 * p:12 * p + 12] / speed for p in range(6)]   # free configurations, as points of the limited space
    lo_s, hi_s = lo / speed, hi / speed
    oracle.set_qs_speed_limits(speed)
    try:
        refs = [S.reference(osc, lo_s, hi_s, mi, p, 0) for p in paths]
    finally:
        oracle.set_qs_speed_limits(None)
    plain = [S.reference(osc, lo_s, hi_s, mi, p, 0) for p in paths]   # the same points without the limits
    assert any(not np.array_equal(a["ok"], b["ok"]) for a, b in zip(refs, plain))
    got = sc.shortcut_paths(L.make_qs_space(3, lo_s, hi_s, mi, speed_limits=speed), paths)
    _same(got, refs, "rate-limited")
    _same(sc.shortcut_paths(L.make_qs_space(3, lo_s, hi_s, mi), paths), plain, "ordinary")


# ------------------------------------------------------------------------------------------ (e) the adaptor
def test_the_cpp_adaptor_shortcuts_a_path(L, ctx, tmp_path):
    """tests/cpp/shortcut_smoke.cpp (g++ against librkh.so, built like prm_paths_smoke.cpp):
    manip_quasi_static_free_space::shortcut_path is the Python binding's answer for the same points."""
    c1 = scenarios.make_c1(world_seed=1)
    lo, hi, mi = c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"]
    src, exe = os.path.join(ROOT, "tests", "cpp", "shortcut_smoke.cpp"), os.path.join(ROOT, "tests", "cpp", "shortcut_smoke")
    newer = [src, os.path.join(ROOT, "include", "rkh_adaptors.hpp"), os.path.join(ROOT, "include", "rkh.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(f) for f in newer)):
        lib_dir = os.path.join(ROOT, "reak_amd")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                        "-L", lib_dir, "-lrkh", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    rng = np.random.default_rng(9)
    path = np.cumsum(rng.normal(0.0, 0.25, (20, 3)), axis=0).clip(-3.0, 3.0)
    qs = L.make_qs_space(3, lo, hi, mi)
    blob = tmp_path / "shortcut_scene.bin"
    with open(blob, "wb") as f:
        f.write(np.int32(len(c1.ops)).tobytes())
        f.write(bytes(c1.ops_array()))
        f.write(bytes(c1.base))
        f.write(np.int32(len(c1.shapes)).tobytes())
        f.write(bytes(c1.shapes_array()))
        f.write(bytes(qs))
        f.write(np.int32(len(path)).tobytes())
        f.write(np.ascontiguousarray(path).tobytes())
    run = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = json.loads(run.stdout.strip().splitlines()[-1])
    sc = L.Scene(ctx, c1)
    for ms, key in ((0, "all"), (3, "span3")):
        keep, cin, cout, nb = sc.shortcut_paths(qs, [path], ms)
        assert out[key]["keep"] == [int(v) for v in keep[0]] and out[key]["n_blocked"] == int(nb[0])
        assert out[key]["cost_in"] == cin[0] and out[key]["cost_out"] == cout[0]
    assert out["single_point"] == [0] and out["empty_path_throws"]
