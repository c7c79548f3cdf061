"""A batch planner's device memory is one arena that its context keeps for the next planner: a planner that starts in
memory another one left behind -- smaller, larger, poisoned, released in between, next to a live one -- computes what
it computes in fresh memory.

Every problem is compared with the sequential CPU oracle on the same seeded problem (parents, the nearest-neighbour
sequence, accept bits, counts: bit for bit).  States: bit for bit with the oracle in the quasi-static space (pure IEEE
arithmetic); in the dynamic space within 1e-10 relative of the oracle (sin / cos are OCML on the device and glibc in the
oracle) and bit for bit with a planner that solved the problem alone under RKH_ARENA_CACHE=0.  No test looks at free
device memory or at timings."""
import contextlib
import os

import numpy as np
import pytest

from reak_amd import scenarios

pytestmark = pytest.mark.gpu

QS_VERTICES = 300
A_BATCH = [(11, 300), (12, 200), (13, 250)]         # (seed, max_vertices): its slab is what B and C find
B_BATCH = [(1, 200), (2, 200)]                      # fits into A's slab
C_BATCH = [(3, 300), (4, 250), (5, 200), (6, 300)]  # larger than A's slab
FIRST_SAMPLE_CAP = 1 << 14                          # samples in a small problem's first stream buffers


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


@pytest.fixture(scope="module")
def c1():
    return scenarios.make_c1_planar(world_seed=1)


@pytest.fixture(scope="module")
def c2():
    return scenarios.make_c2(world_seed=1)


@pytest.fixture(scope="module")
def dyn_ref(L, ctx, oracle, c2):
    """(seed, max_vertices) -> (stats, tree) of the sequential planner in C2's dynamic space and the tree of a planner that
    solved the problem alone, in memory of its own (RKH_ARENA_CACHE=0)"""
    osc, sc = oracle.OracleScene(c2), L.Scene(ctx, c2)
    ref = {}
    with _env(RKH_ARENA_CACHE="0"):
        for seed, vertices in B_BATCH + C_BATCH:
            prm = c2.rrt_params(seed=seed, max_vertices=vertices)
            rc, rout, rtree = osc.rrt_dyn(prm)
            assert rc == 0 and rout.num_vertices == vertices + 1
            pl = L.RrtPlanner(sc, prm)
            pl.solve_planning_query()
            ref[seed, vertices] = (rout, rtree, pl.tree())
            pl.close()
    sc.close()
    return ref


@pytest.fixture(scope="module")
def qs_ref(oracle, c1):
    osc = oracle.OracleScene(c1)
    ref = {}
    for seed in (1, 2):
        rc, rout, rtree = osc.rrt_qs(c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"],
                                     c1.rrt_params(seed=seed, max_vertices=QS_VERTICES))
        assert rc == 0 and rout.num_vertices == QS_VERTICES + 1
        ref[seed] = (rout, rtree)
    return ref


def _same_integers(st, tree, rout, rtree):
    assert (st.num_vertices, st.iterations, st.edges_checked, st.num_solutions) == (
        rout.num_vertices, rout.iterations, rout.edges_checked, rout.num_solutions)
    assert np.array_equal(tree["parent"], rtree["parent"])
    assert np.array_equal(tree["nn_seq"], rtree["nn_seq"])
    assert np.array_equal(tree["accept"], rtree["accept"])


def _make(L, sc, c2, batch):
    return L.RrtPlanner(sc, [c2.rrt_params(seed=s, max_vertices=v) for s, v in batch])


def _check_trees(pl, batch, dyn_ref):
    """every problem of the (solved) batch planner is the oracle's and its alone-run's"""
    for i, key in enumerate(batch):
        st, tree = pl.all_stats[i], pl.tree(i)
        rout, rtree, alone = dyn_ref[key]
        _same_integers(st, tree, rout, rtree)
        assert np.allclose(tree["pos"], rtree["pos"], rtol=1e-10, atol=1e-12)
        assert np.array_equal(np.isinf(tree["goal_dist"]), np.isinf(rtree["goal_dist"]))
        assert np.array_equal(tree["pos"], alone["pos"]) and np.array_equal(tree["goal_dist"], alone["goal_dist"])


def _solve_and_check(pl, batch, dyn_ref):
    pl.solve_planning_query()
    _check_trees(pl, batch, dyn_ref)


def _leave_a_slab(L, sc, c2):
    """A solves and closes: its arena, full of A's trees, is what the next planner on this context finds"""
    a = _make(L, sc, c2, A_BATCH)
    a.solve_planning_query()
    assert all(int(st.num_vertices) == v + 1 for st, (_, v) in zip(a.all_stats, A_BATCH))
    a.close()


def test_recycled_slab(L, ctx, c2, dyn_ref):
    """A leaves its slab; B fits into it; C needs a larger one."""
    ctx.release_cached_memory()
    sc = L.Scene(ctx, c2)
    _leave_a_slab(L, sc, c2)
    b = _make(L, sc, c2, B_BATCH)
    _solve_and_check(b, B_BATCH, dyn_ref)
    b.close()
    c = _make(L, sc, c2, C_BATCH)
    _solve_and_check(c, C_BATCH, dyn_ref)
    c.close()
    sc.close()


def test_overlapping_planners(L, ctx, c2, dyn_ref):
    """A and B live together; A goes; C comes and takes what A left; B solves after that, then C: B's trees are B's."""
    ctx.release_cached_memory()
    sc = L.Scene(ctx, c2)
    a, b = _make(L, sc, c2, C_BATCH), _make(L, sc, c2, B_BATCH)
    a.solve_planning_query()
    a.close()
    c = _make(L, sc, c2, C_BATCH)
    _solve_and_check(b, B_BATCH, dyn_ref)
    _solve_and_check(c, C_BATCH, dyn_ref)
    _check_trees(b, B_BATCH, dyn_ref)  # B's memory is still B's after C ran
    b.close()
    c.close()
    sc.close()


def test_poisoned_memory(L, ctx, c2, dyn_ref):
    """RKH_ARENA_POISON=1 fills the slab with a non-zero pattern before anything is written: a first planner and a
    recycled one give the trees they give without it (nothing depends on zeroed memory)."""
    ctx.release_cached_memory()
    sc = L.Scene(ctx, c2)
    with _env(RKH_ARENA_POISON="1"):
        first = _make(L, sc, c2, B_BATCH)  # a new slab
        _solve_and_check(first, B_BATCH, dyn_ref)
        first.close()
        _leave_a_slab(L, sc, c2)
        again = _make(L, sc, c2, B_BATCH)  # A's slab
        _solve_and_check(again, B_BATCH, dyn_ref)
        again.close()
    sc.close()


def test_grown_stream_buffers(L, ctx, c2, dyn_ref):
    """A small problem's cursor is within 64 rounds' samples of the end of its first stream buffers at the first sync that
    finds it unfinished (here after two rounds): buffers of their own then supersede the arena's ranges, in a recycled
    slab as in a new one, and the rounds after that read and write those."""
    ctx.release_cached_memory()
    sc = L.Scene(ctx, c2)
    _leave_a_slab(L, sc, c2)
    b = _make(L, sc, c2, B_BATCH)
    assert all(b.sample_cap(i) == FIRST_SAMPLE_CAP for i in range(len(B_BATCH)))
    b.enqueue(2)
    b.sync()
    assert not b.done and any(b.sample_cap(i) > FIRST_SAMPLE_CAP for i in range(len(B_BATCH)))
    while not b.done:
        b.enqueue(2)
        b.sync()
    _check_trees(b, B_BATCH, dyn_ref)
    b.close()
    sc.close()


def test_release_cached_memory(L, ctx, c2, dyn_ref):
    """Releasing what the context keeps -- between two planners, and with nothing kept -- leaves the next planner right."""
    ctx.release_cached_memory()
    ctx.release_cached_memory()  # nothing kept
    sc = L.Scene(ctx, c2)
    _leave_a_slab(L, sc, c2)
    ctx.release_cached_memory()
    b = _make(L, sc, c2, B_BATCH)
    _solve_and_check(b, B_BATCH, dyn_ref)
    b.close()
    ctx.release_cached_memory()
    sc.close()


def test_quasi_static_batch_in_a_recycled_slab(L, ctx, c1, qs_ref):
    """C1's quasi-static space (no mirror, no two-lanes workspace): a batch that starts in the slab of the batch before it
    equals the oracle bit for bit, states included."""
    ctx.release_cached_memory()
    sc = L.Scene(ctx, c1)
    qs = L.make_qs_space(3, c1.meta["lower"][:3], c1.meta["upper"][:3], c1.meta["min_interval"])

    def make(seeds):
        return L.RrtPlanner(sc, [c1.rrt_params(seed=s, max_vertices=QS_VERTICES) for s in seeds], qs=qs)
    a = make([7, 8, 9])
    a.solve_planning_query()
    a.close()
    b = make([1, 2])
    b.solve_planning_query()
    for i, seed in enumerate((1, 2)):
        st, tree = b.all_stats[i], b.tree(i)
        rout, rtree = qs_ref[seed]
        _same_integers(st, tree, rout, rtree)
        assert np.array_equal(tree["pos"], rtree["pos"])
        assert np.array_equal(tree["goal_dist"], rtree["goal_dist"])
        assert st.best_cost == rout.best_cost
    b.close()
    sc.close()
