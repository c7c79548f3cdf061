"""Size-independent properties at BASELINE's full sizes (where the oracle would take minutes to hours): the HIP path must
satisfy what the domain guarantees.  GPU only; everything goes through the C-ABI."""
import numpy as np
import pytest

from reak_amd import scenarios

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


def test_nn_sweep_properties_at_one_million_vertices(L, ctx):
    """BASELINE C3 tree size (1 M vertices, 6-D): a vertex is its own nearest neighbour at distance 0; the answer does not
    depend on how the queries are batched; the first of the k nearest is the nearest; k-NN distances ascend and respect
    the radius; appending vertices can only shrink a query's NN distance."""
    n, D = 1_000_000, 6
    nn = L.HipNeighborSearch(ctx, D, n + 64)
    nn.fill_uniform(n, seed=11)
    rng = np.random.default_rng(3)
    q = rng.random((96, D))
    idx, dist = nn.nearest(q)
    assert idx.max() < n and np.all(dist > 0)
    for lo, hi in ((0, 1), (1, 9), (9, 96)):       # any batching gives the same answers
        i2, d2 = nn.nearest(q[lo:hi])
        assert np.array_equal(i2, idx[lo:hi]) and np.array_equal(d2, dist[lo:hi])
    kidx, kdist, kcnt = nn.k_nearest(q[:16], 80, radius=np.inf)
    assert np.all(kcnt == 80)
    assert np.array_equal(kidx[:, 0], idx[:16]) and np.array_equal(kdist[:, 0], dist[:16])
    assert np.all(np.diff(kdist, axis=1) >= 0)
    r = float(np.median(kdist[:, 40]))
    kidx2, kdist2, kcnt2 = nn.k_nearest(q[:16], 80, radius=r)
    for b in range(16):
        m = int((kdist[b] < r).sum())
        assert kcnt2[b] == m and np.array_equal(kidx2[b, :m], kidx[b, :m])
    nn.added_vertices(q[:64])                        # the queries themselves become vertices n .. n+63
    i3, d3 = nn.nearest(q)
    assert np.array_equal(i3[:64], np.arange(n, n + 64)) and np.all(d3[:64] == 0.0)
    assert np.all(d3[64:] <= dist[64:])


def test_full_size_rrt_run_invariants(L, ctx):
    """BASELINE C2 at its full tree size (100 000 vertices), four seeds in one batch: structural invariants of
    generate_rrt, the vertex budget, bounds and collision-freedom of every vertex, and run-to-run determinism."""
    c2 = scenarios.make_c2(world_seed=1)
    sc = L.Scene(ctx, c2)
    mv = 100_000
    prms = [c2.rrt_params(seed=900 + i, max_vertices=mv) for i in range(4)]
    pl = L.RrtPlanner(sc, prms)
    pl.solve_planning_query()
    lo = np.array([c2.dyn.lower[i] for i in range(12)])
    hi = np.array([c2.dyn.upper[i] for i in range(12)])
    first = None
    for i in range(4):
        st, t = pl.all_stats[i], pl.tree(i)
        n, it = int(st.num_vertices), int(st.iterations)
        assert n == mv + 1 and it >= mv                      # keep_going(): the root is not counted
        assert st.edges_checked == it + (n - 1)              # one steer per iteration + one goal probe per vertex
        assert int(t["accept"].sum()) == n - 1               # every accepted steer added exactly one vertex
        par = t["parent"]
        assert par[0] == 0xFFFFFFFF and np.all(par[1:] < np.arange(1, n))   # a parent precedes its child
        # the k-th accepted sample created vertex k+1; its parent is that sample's nearest neighbour
        acc_iter = np.flatnonzero(t["accept"])
        assert np.array_equal(par[1:], t["nn_seq"][acc_iter])
        # the nearest neighbour of sample s existed when s was drawn
        n_before = 1 + np.concatenate(([0], np.cumsum(t["accept"])[:-1]))
        assert np.all(t["nn_seq"] < n_before)
        assert np.all(t["pos"] >= lo - 1e-12) and np.all(t["pos"] <= hi + 1e-12)
        sub = t["pos"][:: max(1, n // 4000)]
        assert np.all(sc.min_distance(sub) >= 0.0)           # vertices are collision-free states
        if i == 0:
            first = (par.copy(), t["pos"].copy())
    pl.close()
    pl2 = L.RrtPlanner(sc, prms[:1])                          # same seed alone: identical tree (batching is invisible)
    pl2.solve_planning_query()
    t2 = pl2.tree(0)
    assert np.array_equal(t2["parent"], first[0]) and np.array_equal(t2["pos"], first[1])


def _components(n, eu, ev):
    root = np.arange(n)

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a

    for a, b in zip(eu, ev):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            root[rb] = ra
    return np.array([find(i) for i in range(n)])


def test_c3_rrtstar_at_two_hundred_thousand_vertices(L, ctx):
    """BASELINE config C3 (6-DOF chain, 50 obstacles, RRT* with k-NN rewiring) for one problem at the largest size that
    fits a test run: 200 000 vertices (about 50 s; iterations are sequential, 3-4 000 per second per problem, so the
    configuration's 1 M vertices would take several minutes -- the 1 M k-NN sweep itself is covered by
    test_nn_sweep_properties_at_one_million_vertices and bench.py's c3_rrtstar object).  The oracle's linear k-NN makes
    a comparison impractical here; checked are the invariants of the reference's bookkeeping."""
    c3 = scenarios.make_c3(world_seed=1)
    sc = L.Scene(ctx, c3)
    lo, hi, mi = c3.meta["lower"], c3.meta["upper"], c3.meta["min_interval"]
    nv = 200000
    pl = L.RrtStarPlanner(sc, c3.rrt_params(seed=1, max_vertices=nv), L.make_qs_space(6, lo, hi, mi))
    st = pl.solve_planning_query()
    g = pl.graph()
    pred, dist, pos = g["pred"].astype(np.int64), g["dist"], g["pos"]
    assert st.num_vertices == nv + 2 and len(pred) == nv + 2 and pred[0] == 0 and dist[0] == 0.0
    v = np.arange(1, len(pred))
    conn = v[pred[v] != 0xFFFFFFFF]
    assert len(conn) > 0.99 * nv
    seg = np.sqrt(((pos[conn] - pos[pred[conn]]) ** 2).sum(axis=1))
    dw = dist[conn] - dist[pred[conn]]
    # an edge's weight is the distance travelled along it; can_be_connected (planning_visitors.hpp:385-395) accepts a walk
    # that stops up to conn_tol = 5 % short of its target, so dist[v] - dist[pred] lies in [|edge| / 1.05, |edge|]
    assert np.all(dw > 0.0) and np.all(dw <= seg + 1e-9) and np.all(dw >= seg / 1.05 - 1e-9)
    assert np.all(np.isfinite(dist[conn]))
    # every connected vertex reaches the start through its predecessors (no cycles): costs strictly decrease towards it
    assert np.all(dist[pred[conn]] < dist[conn])
    # triangle inequality up to the connection tolerance
    assert np.all(dist[conn] >= 0.95 * np.sqrt(((pos[conn] - pos[0]) ** 2).sum(axis=1)) - 1e-9)
    assert st.rewires > 50000 and st.num_solutions >= 1 and st.best_cost == dist[1]
    # the rewiring radius shrinks as the tree grows: late vertices sit closer to their predecessors than early ones
    early, late = conn[conn < 5000], conn[conn > nv - 5000]
    assert np.median(seg[np.isin(conn, late)]) < np.median(seg[np.isin(conn, early)])
    pl.close()


def test_rrtstar_and_prm_invariants_at_scale(L, ctx):
    """6-DOF chain / 50 obstacles in the quasi-static space, sizes the oracle needs minutes for: RRT* cost bookkeeping
    (accumulated cost = predecessor's + edge length, the start is the only root, costs dominate straight-line
    distances) and PRM roadmap bookkeeping (the union-find roots partition the vertices exactly like the edge list
    does, densities in [0, 1], every loop iteration accounted for)."""
    c3 = scenarios.make_c3(world_seed=1)
    sc = L.Scene(ctx, c3)
    lo, hi, mi = c3.meta["lower"], c3.meta["upper"], c3.meta["min_interval"]
    qs = L.make_qs_space(6, lo, hi, mi)
    ps = L.RrtStarPlanner(sc, [c3.rrt_params(seed=40 + i, max_vertices=15000) for i in range(4)], qs)
    ps.solve_planning_query()
    for i in range(4):
        st, g = ps.all_stats[i], ps.graph(i)
        n = int(st.num_vertices)
        pred, dist, pos = g["pred"], g["dist"], g["pos"]
        assert n == 15002 and pred[0] == 0 and dist[0] == 0.0
        conn = np.flatnonzero((pred != 0xFFFFFFFF) & (np.arange(n) != 0))
        seg = np.sqrt(((pos[conn] - pos[pred[conn]]) ** 2).sum(axis=1))
        assert np.all(np.isfinite(dist[conn])) and np.all(dist[pred[conn]] < dist[conn])      # costs grow along the tree
        assert np.all(np.abs(dist[conn] - (dist[pred[conn]] + seg)) <= 0.05 * seg + 1e-12)    # within the connection tol.
        # triangle inequality, up to the connection tolerance (an edge's weight is the distance actually travelled)
        assert np.all(dist[conn] >= 0.95 * np.sqrt(((pos[conn] - pos[0]) ** 2).sum(axis=1)) - 1e-9)
        assert st.rewires > 1000 and st.num_solutions >= 1 and st.best_cost == dist[1]
    ps.close()
    pp = L.PrmPlanner(sc, [c3.prm_params(seed=60 + i, max_vertices=8000, sampling_radius=1.0) for i in range(8)], qs)
    pp.solve_planning_query()
    for i in range(8):
        st, g = pp.all_stats[i], pp.graph(i)
        n, ne = int(st.num_vertices), int(st.num_edges)
        assert n == 8002 and ne == len(g["edge_u"]) and np.all(g["edge_w"] > 0)
        assert np.all(g["edge_u"] < g["edge_v"])             # an edge joins an older vertex to the newest one
        comp = _components(n, g["edge_u"], g["edge_v"])
        assert len(np.unique(comp)) == st.num_components
        mine = _components(n, np.arange(n), g["cc_root"])     # the planner's parent pointers define the same partition
        assert np.array_equal(np.unique(comp, return_inverse=True)[1], np.unique(mine, return_inverse=True)[1])
        assert np.all((g["density"] >= 0.0) & (g["density"] <= 1.0))
        k = np.bincount(g["kind"], minlength=3)
        assert k.sum() == st.loop_iterations and k[0] + k[1] == n - 2


def test_c5_workload_on_one_rank():
    """BASELINE config C5 (independent RRT* seeds sharded over the ranks, best-cost all-reduce) through its own entry,
    `bench.py --workload c5`, on the one rank a test box has: the child process plans two seeds to 40 000 vertices each
    (the configuration's 1 M per seed is three minutes of sequential RRT* iterations per problem -- run once outside
    the suite: 188 s, profiles/r03_c5_one_rank_1M.log; 200 000 vertices: 34 s) and must print the bench contract's JSON line with consistent
    counters.  The N > 1 control path (seed blocks per rank, reductions) is covered on the CPU by
    tests/test_distributed.py; no 8-GPU node is available to the builder."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    nv, P = 40000, 2
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "c5", "--gpus", "1", "--c5-vertices",
                          str(nv), "--c5-problems", str(P), "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                         timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["n_gpus"] == 1 and rec["steps"] == 1 and rec["scaling"] == "weak" and rec["dtype"] == "f64"
    assert "C5" in rec["config"]["workload"] and rec["config"]["vertices_per_seed"] == nv and rec["config"]["seeds_per_gpu"] == P
    secs = rec["ms_per_step"] * 1e-3
    # every seed grew its tree to the budget (+ start and goal vertices); an RRT* iteration adds at most one vertex
    assert abs(rec["vertices_per_s"] * secs - P * (nv + 2)) < 1.0
    assert rec["value"] * secs >= P * nv and rec["edges_collision_checked_per_s"] > rec["value"]
    assert rec["best_solution_cost"] is not None and 0.0 < rec["best_solution_cost"] < 50.0


def test_c2_plain_run_prints_the_headline_only_and_full_adds_the_rest():
    """`bench.py` without --full prints the headline and what the timed steps measure (roofline), none of the objects
    that take runs of their own; --full adds them (here steer_kernels alone: --no-microbench / --no-cpu-baseline leave
    out the side runs).  A small C2 workload, so that the two child processes take seconds."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--problems", "8",
            "--max-vertices", "3000"]
    side = ("steer_kernels", "nn_sweep_hbm", "nn_sweep_mfma", "single_problem", "collide", "c3_rrtstar", "c4_prm_meshes",
            "cpu_baseline", "cpu_baseline_all_cores", "nn_published_config")
    recs = []
    for extra in ([], ["--full", "--no-microbench", "--no-cpu-baseline"]):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        recs.append(json.loads(out.stdout.strip().splitlines()[-1]))
    plain, full = recs
    for rec in recs:
        assert rec["unit"] == "valid node expansions/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
        assert rec["steps"] == 1 and rec["warmup"] == 0 and rec["config"]["problems_per_gpu"] == 8
        assert abs(rec["value"] * rec["ms_per_step"] * 1e-3 - 8 * 3000) < 1.0   # every tree grown to its budget
        assert rec["roofline"]["launches"] > 0
    assert not any(k in plain for k in side)
    assert full["steer_kernels"]["executed_steps"] > 0 and not any(k in full for k in side if k != "steer_kernels")
