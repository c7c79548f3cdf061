"""Roadmap queries on the GPU against tests/roadmap_ref.py (a heapq Dijkstra with the predecessor rule of include/rkh.h
applied after the search).  Distances must be bit-identical and predecessors equal:
 (a) the search kernel through rkh_diag_sssp on graphs a planner never builds -- path graphs whose n - 1 rounds end at wave
     and block edges, a star, two components, zero-weight edges, duplicate edges, a 1500-vertex k-NN graph with two
     planted equal-cost routes, seed lists of 1, 3 and 70 entries with a seed that ties with a graph route -- each in the
     LDS form and (RKH_PRM_PATHS_LDS_MAX lowered) in the global form, with 1, 2 and 65 searches per launch;
 (b) rkh_prm_shortest_paths / rkh_prm_get_solution on C1 roadmaps: finished, empty, stopped and resumed, a batch, and a
     dynamic roadmap;
 (c) rkh_prm_query_paths against connections made with the oracle's k-NN and quasi-static walk;
 (d) bad arguments; (e) the C++ adaptor's roadmap_solution()."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import roadmap_ref as R
from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"lds": None, "global": "1"}   # RKH_PRM_PATHS_LDS_MAX


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


def _set_form(monkeypatch, form):
    if FORMS[form] is None:
        monkeypatch.delenv("RKH_PRM_PATHS_LDS_MAX", raising=False)
    else:
        monkeypatch.setenv("RKH_PRM_PATHS_LDS_MAX", FORMS[form])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------ (a) the kernel
FAMILIES = R.families()
_REF = {}


def _ref(name, s):
    """reference search of family `name` from vertex s, computed once"""
    if (name, s) not in _REF:
        n, eu, ev, ew = FAMILIES[name]
        _REF[(name, s)] = R.vertex_search(R.adjacency(n, eu, ev, ew), s)
    return _REF[(name, s)]


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_search_kernel_matches_dijkstra(L, ctx, monkeypatch, name, form):
    _set_form(monkeypatch, form)
    n, eu, ev, ew = FAMILIES[name]
    row_ptr, col, w = R.csr(n, eu, ev, ew)
    for S in (1, 2, 65):
        sources = [0, n - 1][:S] if S <= 2 else [(7 * i + 3) % n for i in range(S)]
        if name == "knn1500_tie" and S == 2:
            sources = [n - 3, n - 2]   # the two ends of the planted equal-cost routes
        dist, pred, rounds = L.diag_sssp(ctx, row_ptr, col, w, [[(s, 0.0)] for s in sources], [R.NIL] * S)
        for i, s in enumerate(sources):
            rd, rp = _ref(name, s)
            assert np.array_equal(_bits(dist[i]), _bits(rd)), (name, form, S, s)
            assert np.array_equal(pred[i], rp), (name, form, S, s)
        assert 1 <= rounds.min() and rounds.max() <= n
    if name == "two_components":
        dist, pred, _ = L.diag_sssp(ctx, row_ptr, col, w, [[(0, 0.0)]], [R.NIL])
        assert np.isinf(dist[0, 40:]).all() and (pred[0, 40:] == R.NIL).all() and np.isfinite(dist[0, :40]).all()
    if name == "knn1500_tie":   # the tie rule decided: through the lower id, from either end
        lo, a, b = n - 4, n - 3, n - 2
        dist, pred, _ = L.diag_sssp(ctx, row_ptr, col, w, [[(a, 0.0)], [(b, 0.0)]], [R.NIL] * 2)
        assert dist[0, b] == 0.75 and pred[0, b] == lo and dist[1, a] == 0.75 and pred[1, a] == lo


@pytest.mark.parametrize("form", sorted(FORMS))
def test_search_kernel_seed_lists(L, ctx, monkeypatch, form):
    """Seed lists of 1, 3 and 70 entries as a query point's connections; b's seed (0.75) ties with the graph route from a."""
    _set_form(monkeypatch, form)
    n, eu, ev, ew = FAMILIES["knn1500_tie"]
    lo, a, b = n - 4, n - 3, n - 2
    adj = R.adjacency(n, eu, ev, ew)
    row_ptr, col, w = R.csr(n, eu, ev, ew)
    rng = np.random.default_rng(11)
    many = [(a, 0.0), (b, 0.75)] + [(int(v), float(x)) for v, x in zip(rng.integers(0, n, 68), rng.uniform(0.0, 2.0, 68))]
    lists = [[(a, 0.0)], [(a, 0.0), (b, 0.75), (lo, 0.625)], many, [(b, 0.75)], []]
    marks = [R.QUERY_POINT] * len(lists)
    refs = [R.search(adj, sl, R.QUERY_POINT) for sl in lists]
    assert refs[1][1][b] == R.QUERY_POINT and refs[1][1][lo] == a and refs[2][1][b] == R.QUERY_POINT
    dist, pred, _ = L.diag_sssp(ctx, row_ptr, col, w, lists, marks)          # all in one launch
    for i, (rd, rp) in enumerate(refs):
        assert np.array_equal(_bits(dist[i]), _bits(rd)) and np.array_equal(pred[i], rp), (form, i)
    for i in (1, 2):                                                          # and alone
        d1, p1, _ = L.diag_sssp(ctx, row_ptr, col, w, [lists[i]], [R.QUERY_POINT])
        assert np.array_equal(_bits(d1[0]), _bits(refs[i][0])) and np.array_equal(p1[0], refs[i][1])
    assert np.isinf(dist[4]).all() and (pred[4] == R.NIL).all()              # no seed: nothing is reached


def test_path_graph_takes_every_round(L, ctx):
    for n in (2, 65, 257):
        row_ptr, col, w = R.csr(*R.path_graph(n))
        dist, pred, rounds = L.diag_sssp(ctx, row_ptr, col, w, [[(0, 0.0)]], [R.NIL])
        assert np.array_equal(dist[0], np.arange(n, dtype=np.float64)) and rounds[0] <= n
        assert np.array_equal(pred[0, 1:], np.arange(n - 1)) and pred[0, 0] == R.NIL


# ------------------------------------------------------------------------------------------ (b) roadmaps
def _c1():
    c1 = scenarios.make_c1(world_seed=1)
    return c1, c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"]


def _adj(g):
    return R.adjacency(len(g["pos"]), g["edge_u"], g["edge_v"], g["edge_w"])


def _check_solution(g, adj, path, cost):
    d, pred = R.vertex_search(adj, 0)
    assert _bits(cost) == _bits(d[1])
    if np.isinf(d[1]):
        assert len(path) == 0
        return
    assert list(path) == R.walk(pred, 1) and path[0] == 0 and path[-1] == 1
    wmin = {}
    for u, v, w in zip(g["edge_u"], g["edge_v"], g["edge_w"]):
        key = (min(int(u), int(v)), max(int(u), int(v)))
        wmin[key] = min(wmin.get(key, np.inf), float(w))
    s = 0.0
    for u, v in zip(path[:-1], path[1:]):
        key = (min(int(u), int(v)), max(int(u), int(v)))
        assert key in wmin, "consecutive path vertices share no edge"
        s += wmin[key]                      # left to right
    assert _bits(s) == _bits(cost)


@pytest.fixture(scope="module")
def roadmap(L, ctx):
    c1, lo, hi, mi = _c1()
    sc = L.Scene(ctx, c1)
    prm = c1.prm_params(seed=1, max_vertices=800, sampling_radius=1.0)
    pl = L.PrmPlanner(sc, prm, L.make_qs_space(3, lo, hi, mi))
    st = pl.solve_planning_query()
    g = pl.graph()
    assert st.num_vertices >= 800 and st.merged_at_vertex > 0
    return {"pl": pl, "g": g, "adj": _adj(g), "c1": c1, "prm": prm, "sc": sc}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_roadmap_shortest_paths_and_solution(L, roadmap, monkeypatch, form):
    _set_form(monkeypatch, form)
    pl, g, adj = roadmap["pl"], roadmap["g"], roadmap["adj"]
    n = len(g["pos"])
    sources = [0, 1, n - 1] + [v for v in range(n) if not adj[v]][:1]
    dist, pred = pl.shortest_paths(sources)
    for i, s in enumerate(sources):
        rd, rp = R.vertex_search(adj, s)
        assert np.array_equal(_bits(dist[i]), _bits(rd)) and np.array_equal(pred[i], rp), (form, s)
    d1, _ = pl.shortest_paths([0, 1])        # a second call reuses the CSR: the same answer
    assert np.array_equal(_bits(d1), _bits(dist[:2]))
    path, cost = pl.solution()
    assert np.isfinite(cost) and _bits(cost) == _bits(dist[0][1])
    _check_solution(g, adj, path, cost)


def test_empty_roadmap_reports_no_path_like_the_other_planners(L, ctx):
    c1, lo, hi, mi = _c1()
    sc = L.Scene(ctx, c1)
    qs = L.make_qs_space(3, lo, hi, mi)
    pl = L.PrmPlanner(sc, c1.prm_params(seed=1, max_vertices=250, sampling_radius=1.0), qs)
    st = pl.solve_planning_query(max_loop_iterations=0)
    assert (st.num_vertices, st.num_edges) == (2, 0)
    path, cost = pl.solution()
    star = L.RrtStarPlanner(sc, c1.rrt_params(seed=1, max_vertices=50), qs)
    star.solve_planning_query(max_loop_iterations=0)
    spath, scost = star.solution()
    assert len(path) == len(spath) == 0 and cost == scost == np.inf
    dist, pred = pl.shortest_paths([1])
    assert dist.tolist() == [[np.inf, 0.0]] and pred.tolist() == [[R.NIL, R.NIL]]
    pl.close(), star.close()


def test_stopped_and_resumed_roadmap_answers_for_each_stage(L, ctx):
    c1, lo, hi, mi = _c1()
    sc = L.Scene(ctx, c1)
    pl = L.PrmPlanner(sc, c1.prm_params(seed=1, max_vertices=250, sampling_radius=1.0), L.make_qs_space(3, lo, hi, mi))
    pl.solve_planning_query(max_loop_iterations=100)
    g1 = pl.graph()
    p1, c1_cost = pl.solution()
    _check_solution(g1, _adj(g1), p1, c1_cost)
    pl.solve_planning_query()
    g2 = pl.graph()
    assert len(g2["pos"]) > len(g1["pos"])
    p2, c2_cost = pl.solution()
    _check_solution(g2, _adj(g2), p2, c2_cost)
    assert np.isfinite(c2_cost) and c2_cost <= c1_cost
    dist, _ = pl.shortest_paths([0])
    assert _bits(dist[0][1]) == _bits(c2_cost)
    pl.close()


def test_batch_solutions_equal_single_problem_runs(L, ctx):
    c1, lo, hi, mi = _c1()
    sc = L.Scene(ctx, c1)
    qs = L.make_qs_space(3, lo, hi, mi)
    prms = [c1.prm_params(seed=s, max_vertices=m, sampling_radius=1.0) for s, m in ((5, 250), (6, 400), (7, 300))]
    pl = L.PrmPlanner(sc, prms, qs)
    pl.solve_planning_query()
    got = [pl.solution(i) for i in range(3)]
    for i, prm in enumerate(prms):
        g = pl.graph(i)
        _check_solution(g, _adj(g), *got[i])
        one = L.PrmPlanner(sc, prm, qs)
        one.solve_planning_query()
        path, cost = one.solution()
        assert list(path) == list(got[i][0]) and _bits(cost) == _bits(got[i][1]), i
        one.close()
    assert len({len(pl.graph(i)["pos"]) for i in range(3)}) == 3
    pl.close()


def test_dynamic_roadmap_searches_and_refuses_multi_query(L, ctx):
    c2 = scenarios.make_c2(world_seed=1)
    sc = L.Scene(ctx, c2)
    prm = c2.prm_params(seed=3, max_vertices=200, sampling_radius=1.0)
    prm.base.conn_tol = 3.0
    pl = L.PrmPlanner(sc, prm, c2.dyn)
    st = pl.solve_planning_query()
    g = pl.graph()
    adj = _adj(g)
    assert st.num_edges > 100
    n = len(g["pos"])
    sources = [0, 1, n - 1]
    dist, pred = pl.shortest_paths(sources)
    for i, s in enumerate(sources):
        rd, rp = R.vertex_search(adj, s)
        assert np.array_equal(_bits(dist[i]), _bits(rd)) and np.array_equal(pred[i], rp), s
    _check_solution(g, adj, *pl.solution())
    pts = np.zeros((1, 12))
    cost, npth = np.zeros(1), np.zeros(1, dtype=np.uint32)
    rc = pl.lib.rkh_prm_query_paths(pl.h, 0, T.dptr(pts), T.dptr(pts), 1, 4, 1.0, 0, T.dptr(cost), None, T.u32ptr(npth))
    assert rc == -5 and b"quasi-static" in pl.lib.rkh_last_error()
    pl.close()


# ------------------------------------------------------------------------------------------ (c) multi-query
def make_queries(c1, osc, seed=4, n_pairs=40):
    """40 random free (start, goal) pairs in the sampling box of C1 (free: the oracle's distance is positive) and one
    point inside an obstacle."""
    lo, hi = np.asarray(c1.meta["lower"]), np.asarray(c1.meta["upper"])
    rng = np.random.default_rng(seed)
    pts = rng.uniform(lo, hi, size=(600, 3))
    x = np.zeros((len(pts), 6))
    x[:, 0::2] = pts
    d = osc.min_distance(x)
    free, hit = pts[d > 1e-3], pts[d < -1e-3]
    assert len(free) >= 2 * n_pairs and len(hit) >= 1
    return free[:n_pairs].copy(), free[n_pairs:2 * n_pairs].copy(), hit[0].copy()


def reference_queries(oracle_lib, osc, c1, g, adj, conn_tol, starts, goals, k, radius):
    lo, hi, mi = c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"]
    out = []
    for a, b in zip(starts, goals):
        sc = R.connections(oracle_lib, osc, lo, hi, mi, conn_tol, g["pos"], a, k, radius, True)
        gc = R.connections(oracle_lib, osc, lo, hi, mi, conn_tol, g["pos"], b, k, radius, False)
        out.append(R.query(adj, sc, gc))
    return out


def _same_queries(got_cost, got_paths, ref):
    for i, (rc, rp) in enumerate(ref):
        assert _bits(got_cost[i]) == _bits(rc), (i, got_cost[i], rc)
        assert list(got_paths[i]) == rp, i


@pytest.mark.parametrize("form", sorted(FORMS))
def test_multi_query_matches_oracle_made_connections(L, oracle, roadmap, monkeypatch, form):
    _set_form(monkeypatch, form)
    pl, g, adj, c1 = roadmap["pl"], roadmap["g"], roadmap["adj"], roadmap["c1"]
    osc = oracle.OracleScene(c1)
    conn_tol = roadmap["prm"].base.conn_tol
    starts, goals, inside = make_queries(c1, osc)
    k, radius = 6, 0.6
    ref = reference_queries(oracle, osc, c1, g, adj, conn_tol, starts, goals, k, radius)
    found = sum(1 for c, _ in ref if np.isfinite(c))
    print("reference finds a path for", found, "of", len(ref))
    assert found >= 30 and found < len(ref)   # not passing on nothing, and the no-path answer is exercised
    cost, paths = pl.query_paths(starts, goals, k, radius)
    _same_queries(cost, paths, ref)
    assert all(len(p) == 0 for c, p in zip(cost, paths) if np.isinf(c)) and all(len(p) >= 1 for c, p in zip(cost, paths) if np.isfinite(c))
    # a pair equal to two roadmap vertices (weight-0 connections); a start inside an obstacle; k = 1 and k = 12
    v1, v2 = 0, 1
    s2 = np.array([g["pos"][v1], inside, starts[0], starts[1]])
    g2 = np.array([g["pos"][v2], goals[0], goals[0], goals[1]])
    for kk in (1, 12):
        ref2 = reference_queries(oracle, osc, c1, g, adj, conn_tol, s2, g2, kk, radius)
        cost2, paths2 = pl.query_paths(s2, g2, kk, radius)
        _same_queries(cost2, paths2, ref2)
        assert np.isinf(cost2[1]) and len(paths2[1]) == 0
        d, pred = R.vertex_search(adj, v1)
        if kk == 1:   # only the coincident vertices connect: the answer of rkh_prm_get_solution
            assert _bits(cost2[0]) == _bits(d[v2]) and list(paths2[0]) == R.walk(pred, v2) == list(pl.solution()[0])
        else:
            assert cost2[0] <= d[v2]
    # a radius that excludes everything
    cost3, paths3 = pl.query_paths(starts[:3], goals[:3], k, 1e-9)
    assert np.isinf(cost3).all() and all(len(p) == 0 for p in paths3)
    # a capacity below the path length: the count is the full length, the slots hold its first vertices
    i = int(np.argmax([len(p) for p in paths]))
    cost4, paths4 = pl.query_paths(starts[i:i + 1], goals[i:i + 1], k, radius, capacity=2)
    assert _bits(cost4[0]) == _bits(cost[i]) and list(paths4[0]) == list(paths[i][:2])


# ------------------------------------------------------------------------------------------ (d) bad arguments
def test_bad_arguments(L, ctx, roadmap):
    pl = roadmap["pl"]
    lib, h = pl.lib, pl.h
    n = len(roadmap["g"]["pos"])
    src = np.array([0, n], dtype=np.uint32)
    dist, pred = np.zeros((2, n)), np.zeros((2, n), dtype=np.uint32)
    BAD = -1
    assert lib.rkh_prm_shortest_paths(h, 0, T.u32ptr(src), 2, T.dptr(dist), T.u32ptr(pred)) == BAD      # a source >= n
    assert lib.rkh_prm_shortest_paths(h, 0, None, 1, T.dptr(dist), T.u32ptr(pred)) == BAD               # no sources
    assert lib.rkh_prm_shortest_paths(h, 1, T.u32ptr(src), 1, T.dptr(dist), T.u32ptr(pred)) == BAD      # problem
    assert lib.rkh_prm_shortest_paths(h, 0, T.u32ptr(src), 1, None, None) == BAD                        # both NULL
    assert lib.rkh_prm_shortest_paths(None, 0, T.u32ptr(src), 1, T.dptr(dist), T.u32ptr(pred)) == BAD
    assert lib.rkh_prm_shortest_paths(h, 0, None, 0, T.dptr(dist), T.u32ptr(pred)) == 0                 # S == 0
    rd, rp = R.vertex_search(roadmap["adj"], 0)
    dist[:] = -1.0
    assert lib.rkh_prm_shortest_paths(h, 0, T.u32ptr(src), 1, T.dptr(dist), None) == 0                  # either alone
    assert np.array_equal(_bits(dist[0]), _bits(rd))
    assert lib.rkh_prm_shortest_paths(h, 0, T.u32ptr(src), 1, None, T.u32ptr(pred)) == 0
    assert np.array_equal(pred[0], rp)
    # rkh_prm_get_solution: the rules of rkh_rrtstar_get_solution
    npth, cost = C.c_uint32(7), C.c_double(-1.0)
    assert lib.rkh_prm_get_solution(h, 0, None, 0, None, C.byref(cost)) == BAD
    assert lib.rkh_prm_get_solution(h, 1, None, 0, C.byref(npth), C.byref(cost)) == BAD
    assert lib.rkh_prm_get_solution(h, 0, None, 0, C.byref(npth), None) == 0 and npth.value >= 2
    buf = np.full(npth.value + 2, 0xABCD, dtype=np.uint32)
    assert lib.rkh_prm_get_solution(h, 0, T.u32ptr(buf), npth.value - 1, C.byref(npth), C.byref(cost)) == -6   # capacity
    assert (buf == 0xABCD).all()
    assert lib.rkh_prm_get_solution(h, 0, T.u32ptr(buf), npth.value, C.byref(npth), C.byref(cost)) == 0
    assert buf[0] == 0 and buf[npth.value - 1] == 1 and buf[npth.value] == 0xABCD and cost.value == rd[1]
    # rkh_prm_query_paths
    a = np.zeros((1, 3))
    c, m = np.zeros(1), np.zeros(1, dtype=np.uint32)
    assert lib.rkh_prm_query_paths(h, 0, None, T.dptr(a), 1, 4, 1.0, 0, T.dptr(c), None, T.u32ptr(m)) == BAD
    assert lib.rkh_prm_query_paths(h, 0, T.dptr(a), None, 1, 4, 1.0, 0, T.dptr(c), None, T.u32ptr(m)) == BAD
    assert lib.rkh_prm_query_paths(h, 0, T.dptr(a), T.dptr(a), 1, 0, 1.0, 0, T.dptr(c), None, T.u32ptr(m)) == BAD
    assert lib.rkh_prm_query_paths(h, 0, T.dptr(a), T.dptr(a), 1, 4, 1.0, 0, None, None, T.u32ptr(m)) == BAD
    assert lib.rkh_prm_query_paths(h, 0, T.dptr(a), T.dptr(a), 1, 4, 1.0, 0, T.dptr(c), None, None) == BAD
    assert lib.rkh_prm_query_paths(h, 3, T.dptr(a), T.dptr(a), 1, 4, 1.0, 0, T.dptr(c), None, T.u32ptr(m)) == BAD
    assert lib.rkh_prm_query_paths(h, 0, None, None, 0, 4, 1.0, 0, None, None, None) == 0               # B == 0
    # rkh_diag_sssp refuses a CSR it could not index safely
    row_ptr, col, w = R.csr(*R.path_graph(4))
    bad_col = col.copy()
    bad_col[0] = 4
    with pytest.raises(L.RkhError):
        L.diag_sssp(ctx, row_ptr, bad_col, w, [[(0, 0.0)]], [R.NIL])
    with pytest.raises(L.RkhError):
        L.diag_sssp(ctx, row_ptr, col, w, [[(4, 0.0)]], [R.NIL])
    with pytest.raises(L.RkhError):
        L.diag_sssp(ctx, row_ptr[::-1].copy(), col, w, [[(0, 0.0)]], [R.NIL])


# ------------------------------------------------------------------------------------------ (e) the adaptor
def test_the_cpp_adaptor_returns_the_roadmap_solution(L, ctx, tmp_path):
    """tests/cpp/prm_paths_smoke.cpp (g++ against librkh.so, built like prox_records_smoke.cpp): roadmap_solution() of
    hip_prm_planner after solve_planning_query is the Python binding's solution for the same seed."""
    c1, lo, hi, mi = _c1()
    src, exe = os.path.join(ROOT, "tests", "cpp", "prm_paths_smoke.cpp"), os.path.join(ROOT, "tests", "cpp", "prm_paths_smoke")
    newer = [src, os.path.join(ROOT, "include", "rkh_adaptors.hpp"), os.path.join(ROOT, "include", "rkh.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(f) for f in newer)):
        lib_dir = os.path.join(ROOT, "reak_amd")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                        "-L", lib_dir, "-lrkh", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    qprm = c1.rrt_params(seed=2, max_vertices=400)
    radius = 1.0
    blob = tmp_path / "qs_scene.bin"
    with open(blob, "wb") as f:
        f.write(np.int32(len(c1.ops)).tobytes())
        f.write(bytes(c1.ops_array()))
        f.write(bytes(c1.base))
        f.write(np.int32(len(c1.shapes)).tobytes())
        f.write(bytes(c1.shapes_array()))
        f.write(bytes(L.make_qs_space(3, lo, hi, mi)))
        f.write(bytes(qprm))
        f.write(np.float64(radius).tobytes())
    run = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = json.loads(run.stdout.strip().splitlines()[-1])
    sc = L.Scene(ctx, c1)
    pl = L.PrmPlanner(sc, c1.prm_params(seed=2, max_vertices=400, sampling_radius=radius), L.make_qs_space(3, lo, hi, mi))
    st = pl.solve_planning_query()
    path, cost = pl.solution()
    pl.close()
    assert (out["vertices"], out["edges"]) == (st.num_vertices, st.num_edges)
    assert out["path"] == [int(v) for v in path] and out["cost"] == cost and len(path) >= 2
    assert out["edges_ok"] and out["weight_sum"] == cost and out["no_roadmap_throws"] and out["repeatable"]
    assert out["register_calls"] == 0   # still nothing is registered with the query
