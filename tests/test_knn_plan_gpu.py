"""rkh_nn_queryk over the whole range of requests its launch plan takes (reak_amd/csrc/knn_plan.h, knn_sweep.hip),
against the plain reference tests/knn_ref.py: distances, counts and indices with np.array_equal, ties included.

The plan's edges: the query-block switch at B = 8 / 9, a second row of query blocks at B = 32 / 33, lanes past the
last query, trailing blocks without a tile (600 tiles on 512 blocks), ksel between 1 and 8, lists of 2048 / 4096 slots,
the strict radius, ties across rank k and across blocks -- and the requests the first pass alone cannot serve (few
tiles and a large k; live rows in few tiles after removals), which the exact retry answers."""
import time

import numpy as np
import pytest

import knn_ref

pytestmark = pytest.mark.gpu

CAPACITY = -6  # RKH_ERR_CAPACITY


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


def _store(L, ctx, pts, removed=None):
    nn = L.HipNeighborSearch(ctx, pts.shape[1], pts.shape[0])
    nn.added_vertices(pts)
    if removed is not None:
        for i in removed:
            nn.removed_vertex(int(i))
    return nn


def _same(got, ref):
    idx, dist, cnt = got
    ridx, rdist, rcnt = ref
    assert np.array_equal(cnt, rcnt)
    assert np.array_equal(dist, rdist)
    assert np.array_equal(idx, ridx)


# (n, B, k).  The plan (knn_plan_test N B K) gives m_sub < k with n > cmax -- no bound at all, a request the first pass
# alone had to refuse with RKH_ERR_CAPACITY -- for (2304, 9, 73), (3000, 1, 100), (3000, 33, 100), (5000, 5, 200),
# (8192, 32, 257) and (8000, 3, 1024).  Before the exact retry those six failed in both widths, and so did
# (2049, 8, 72) and (32768, 33, 1024): m_sub = k there, the bound is the LARGEST subset minimum and names more than
# cmax vertices ((32767, 2, 1024), planned alike, happened to fit).
PLAN_GRID =[(257, 9, 1), (2049, 8, 72), (2304, 9, 73), (3000, 1, 100), (3000, 33, 100), (5000, 5, 200), (8192, 32, 257),
             (8000, 3, 1024), (32767, 2, 1024), (32768, 33, 1024), (153600, 7, 16), (153600, 40, 300)]


@pytest.mark.parametrize("D", [3, 12])
@pytest.mark.parametrize("n,B,k", PLAN_GRID)
def test_plan_grid(L, ctx, n, B, k, D):
    rng = np.random.default_rng(7 * n + 13 * B + k + D)
    pts = rng.uniform(-3, 3, size=(n, D))
    q = rng.uniform(-3, 3, size=(B, D))
    nn = _store(L, ctx, pts)
    got = nn.k_nearest(q, k)
    _same(got, knn_ref.knn(q, pts, k))
    if k == 1:
        i1, d1 = nn.nearest(q)
        assert np.array_equal(i1, got[0][:, 0]) and np.array_equal(d1, got[1][:, 0])


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6, 7, 8, 12])
def test_every_padded_width(L, ctx, D):
    rng = np.random.default_rng(50 + D)
    pts = rng.uniform(-3, 3, size=(777, D))
    q = rng.uniform(-3, 3, size=(9, D))
    _same(_store(L, ctx, pts).k_nearest(q, 10), knn_ref.knn(q, pts, 10))


@pytest.mark.parametrize("B", [1, 7, 8, 9, 31, 32, 33])
def test_lanes_past_the_last_query(L, ctx, B):
    """The last query lies far from the others: a lane that took another query's bound for it would drop neighbours."""
    rng = np.random.default_rng(70 + B)
    pts = rng.uniform(-3, 3, size=(600, 3))
    q = rng.uniform(-3, 3, size=(B, 3))
    q[-1] = [40.0, -35.0, 50.0]
    _same(_store(L, ctx, pts).k_nearest(q, 5), knn_ref.knn(q, pts, 5))


def test_radius_is_strict(L, ctx):
    n, k = 5000, 12
    rng = np.random.default_rng(90)
    pts = rng.uniform(-3, 3, size=(n, 3))
    q = rng.uniform(-3, 3, size=(3, 3))
    nn = _store(L, ctx, pts)
    d = np.sort(knn_ref.distances(q[:1], pts)[0])
    assert np.unique(d[:k + 2]).size == k + 2  # no ties among the distances the radius is set to
    for j in (0, 1, k - 1, k):
        want = min(j, k)
        for radius, count in ((d[j], want), (np.nextafter(d[j], np.inf), min(j + 1, k))):
            got = nn.k_nearest(q, k, radius)
            assert got[2][0] == count, (j, radius)
            _same(got, knn_ref.knn(q, pts, k, radius))


def test_ties_across_blocks_in_index_order(L, ctx):
    """Every base point four times, the copies in different blocks of the sweep; rank k = 6 cuts through a group."""
    n = 153600
    rng = np.random.default_rng(91)
    pts = rng.uniform(50, 60, size=(n, 3))  # the other rows lie far off: every neighbour is a copy of a base point
    base = rng.uniform(-3, 3, size=(400, 3))
    for off in (0, 70000, 140000, 150000):
        pts[off:off + 400] = base
    q = base[:9] + 1e-3
    got = _store(L, ctx, pts).k_nearest(q, 6)
    ref = knn_ref.knn(q, pts, 6)
    for b in range(9):  # the nearest four are the copies of base point b, in index order, and rank 6 splits a group
        assert ref[0][b, :4].tolist() == [b, b + 70000, b + 140000, b + 150000]
        assert ref[1][b, 4] == ref[1][b, 5] and ref[0][b, 5] == ref[0][b, 4] + 70000
    _same(got, ref)


def test_coincident_vertices_lowest_indices_first(L, ctx):
    rng = np.random.default_rng(92)
    pts = rng.uniform(-3, 3, size=(3000, 3))
    where = np.sort(rng.choice(3000, size=1500, replace=False))
    pts[where] = [0.25, -1.5, 2.0]
    q = np.array([[0.25, -1.5, 2.0]])
    got = _store(L, ctx, pts).k_nearest(q, 40)
    assert got[0][0].tolist() == where[:40].tolist() and (got[1] == 0.0).all()
    _same(got, knn_ref.knn(q, pts, 40))


def test_more_coincident_vertices_than_a_list_holds(L, ctx):
    """The one capacity limit left (include/rkh.h, rkh_nn_queryk): more vertices at exactly the k-th distance than the
    candidate list holds next to the k nearest.  RKH_ERR_CAPACITY, and the text names coincident vertices, not the
    radius; a query that does not end inside the group is served."""
    rng = np.random.default_rng(93)
    pts = rng.uniform(-3, 3, size=(6000, 3))
    pts[500:5500] = [1.0, 1.0, 1.0]
    nn = _store(L, ctx, pts)
    with pytest.raises(L.RkhError) as e:
        nn.k_nearest(np.array([[1.0, 1.0, 1.0]]), 10)
    assert e.value.status == CAPACITY
    assert "coincident" in str(e.value) and "shrink the radius" not in str(e.value)
    far = np.array([[-2.9, -2.9, 2.9]])
    d = knn_ref.distances(far, pts)[0]
    k = int((d < d[500]).sum())  # the vertices nearer than the group
    assert 1 <= k <= 1000
    _same(nn.k_nearest(far, k), knn_ref.knn(far, pts, k))  # the list ends just before the group


REMOVAL_N, REMOVAL_K = 40000, 24


@pytest.fixture(scope="module")
def removal_data():
    rng = np.random.default_rng(94)
    return rng.uniform(-3, 3, size=(REMOVAL_N, 12)), rng.uniform(-3, 3, size=(20, 12))


def _live_sets():
    n = REMOVAL_N
    every64 = np.zeros(n, dtype=bool)
    for t in range(0, (n + 255) // 256, 64):
        every64[t * 256:(t + 1) * 256] = True
    few = np.zeros(n, dtype=bool)
    few[[5, 300, 9000, 39999] + list(range(20000, 20000 + REMOVAL_K - 1 - 4))] = True
    return {"first_3000": np.arange(n) < 3000, "last_3000": np.arange(n) >= n - 3000, "every_64th_tile": every64,
            "none": np.zeros(n, dtype=bool), "k_minus_1": few}


@pytest.mark.parametrize("which", ["first_3000", "last_3000", "every_64th_tile", "none", "k_minus_1"])
def test_removed_rows(L, ctx, removal_data, which):
    """Live rows in few tiles: most blocks of the bound sweep see removed rows only and hand on +inf minima."""
    pts, q = removal_data
    live = _live_sets()[which]
    removed = np.nonzero(~live)[0]
    t0 = time.perf_counter()
    nn = _store(L, ctx, pts, removed=removed)
    print("removed", removed.size, "rows in %.2f s" % (time.perf_counter() - t0))
    assert nn.live_size() == int(live.sum())
    got = nn.k_nearest(q, REMOVAL_K)
    ref = knn_ref.knn(q, pts, REMOVAL_K, removed=removed)
    want = {"none": 0, "k_minus_1": REMOVAL_K - 1}.get(which, REMOVAL_K)
    assert (ref[2] == want).all()
    _same(got, ref)


@pytest.mark.parametrize("s", [1e-150, 1e-9, 1e9, 1e150])
def test_scale(L, ctx, s):
    """The collect sweep's threshold tau * tau * (1 + 8 eps) at both ends of the exponent range (squares stay normal)."""
    rng = np.random.default_rng(95)
    pts = rng.uniform(-3, 3, size=(3000, 12)) * s
    q = rng.uniform(-3, 3, size=(5, 12)) * s
    ref = knn_ref.knn(q, pts, 20)
    assert np.isfinite(ref[1]).all() and (ref[1] > 0).all()
    _same(_store(L, ctx, pts).k_nearest(q, 20), ref)


def test_workspace_reuse_across_plans(L, ctx):
    """One handle, requests whose plans differ: a stale overflow word or a stale carve of the workspace would show."""
    rng = np.random.default_rng(96)
    pts = rng.uniform(-3, 3, size=(6000, 6))
    nn = _store(L, ctx, pts)
    for B, k in ((2, 1024), (2, 1), (257, 3), (1, 3), (3, 1024), (1, 100)):
        q = rng.uniform(-3, 3, size=(B, 6))
        _same(nn.k_nearest(q, k), knn_ref.knn(q, pts, k))


def test_planner_steps_take_the_retry_and_keep_their_results(L, ctx, monkeypatch):
    """The planners' path (launch_nnk_table, one job per problem): with candidate lists of 128 slots (RKH_KNN_LIST_CAP,
    rkh_diag.h) nearly every RRT* step of two problems overflows in one problem or both, the exact retry redoes those
    searches and the step's edge walks run again on its results.  The graphs equal those of the full lists, vertex for
    vertex: a problem's retry changes neither its own result nor its neighbour's."""
    from reak_amd import scenarios

    c1 = scenarios.make_c1(world_seed=1)
    lo, hi, mi = c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"]
    sc = L.Scene(ctx, c1)
    retries = L.load().rkh_diag_knn_retries

    def run():
        prms = [c1.rrt_params(seed=1, max_vertices=700), c1.rrt_params(seed=2, max_vertices=500)]
        for prm in prms:  # free configurations 4.5 apart: the star radius, 3 |start - goal| (log N / N)^(1/3), then
            for i, (s, g) in enumerate(zip((2.5, -2.5, 2.5), (2.0, 2.0, 2.0))):  # holds hundreds of vertices
                prm.start[i], prm.goal[i] = s, g
        pl = L.RrtStarPlanner(sc, prms, L.make_qs_space(3, lo, hi, mi))
        before = retries()
        pl.solve_planning_query()
        out = [pl.graph(i) for i in range(2)], [(s.num_vertices, s.loop_iterations, s.rewires, s.edges_checked, s.best_cost)
                                                for s in pl.all_stats], retries() - before
        pl.close()
        return out

    monkeypatch.delenv("RKH_KNN_LIST_CAP", raising=False)
    graphs, stats, n_retry = run()
    assert n_retry == 0 and all(s[2] > 50 and s[3] > 1000 for s in stats)  # fewer than 2048 vertices: a full list cannot overflow
    monkeypatch.setenv("RKH_KNN_LIST_CAP", "1")
    graphs_c, stats_c, n_retry_c = run()
    print("steps that took the retry:", n_retry_c, "of", sum(s[1] for s in stats))
    assert n_retry_c > 50
    assert stats_c == stats
    for g, gc in zip(graphs, graphs_c):
        for key in ("near_seq", "pred", "pos", "dist"):
            assert np.array_equal(g[key], gc[key]), key


def test_short_lists_give_the_same_neighbours(L, ctx, monkeypatch):
    """rkh_nn_queryk with lists of 2 k slots (rounded up to 128) over 1000 rows = 4 tiles x 8 subset minima: k = 33 and
    k = 50 have no bound, every first pass overflows and the retry answers; k = 1 and k = 7 are bounded and fit."""
    rng = np.random.default_rng(98)
    pts = rng.uniform(-3, 3, size=(1000, 6))
    q = rng.uniform(-3, 3, size=(33, 6))
    nn = _store(L, ctx, pts)
    monkeypatch.setenv("RKH_KNN_LIST_CAP", "1")
    retries = L.load().rkh_diag_knn_retries
    for k in (1, 7, 33, 50):
        before = retries()
        _same(nn.k_nearest(q, k), knn_ref.knn(q, pts, k))
        assert retries() - before == 1 or k < 33, k  # one retry per call serves all of its overflowed queries


def test_roadmap_queries_with_a_large_k(L, ctx, oracle):
    """rkh_prm_query_paths with k = 100 over a roadmap of more than 2048 vertices: 9 tiles x 8 subset minima < k, the
    request the first pass alone refused."""
    import roadmap_ref as R
    from reak_amd import scenarios

    c1 = scenarios.make_c1(world_seed=1)
    lo, hi, mi = c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"]
    sc = L.Scene(ctx, c1)
    prm = c1.prm_params(seed=1, max_vertices=2200, sampling_radius=1.0)
    pl = L.PrmPlanner(sc, prm, L.make_qs_space(3, lo, hi, mi))
    t0 = time.perf_counter()
    st = pl.solve_planning_query()
    print("roadmap of", st.num_vertices, "vertices built in %.2f s" % (time.perf_counter() - t0))
    g = pl.graph()
    assert len(g["pos"]) > 2048
    adj = R.adjacency(len(g["pos"]), g["edge_u"], g["edge_v"], g["edge_w"])
    osc = oracle.OracleScene(c1)
    rng = np.random.default_rng(97)
    cand = rng.uniform(np.asarray(lo), np.asarray(hi), size=(60, 3))
    x = np.zeros((len(cand), 6))
    x[:, 0::2] = cand
    free = cand[osc.min_distance(x) > 1e-3]
    starts, goals = free[:2], free[2:4]
    k, radius = 100, np.inf
    cost, paths = pl.query_paths(starts, goals, k, radius)
    for i in range(2):
        s = R.connections(oracle, osc, lo, hi, mi, prm.base.conn_tol, g["pos"], starts[i], k, radius, True)
        e = R.connections(oracle, osc, lo, hi, mi, prm.base.conn_tol, g["pos"], goals[i], k, radius, False)
        rc, rp = R.query(adj, s, e)
        assert np.float64(cost[i]).view(np.uint64) == np.float64(rc).view(np.uint64), (i, cost[i], rc)
        assert list(paths[i]) == rp
    assert np.isfinite(cost).any()
