"""Handle lifetimes: a refused create leaves nothing behind that a later planner could notice, handles that overlap
in time own their device memory separately, and a scene can be built and torn down again and again.

Every planner here is compared with the sequential CPU oracle on the same seeded problem: integer work (parents, the
nearest-neighbour sequence, accept bits, counts) bit for bit; states bit for bit in the quasi-static space (pure IEEE
arithmetic) and within 1e-10 relative in the dynamic space (sin / cos are OCML on the device and glibc in the oracle),
where they are also compared bit for bit with a planner that ran alone.  No test looks at free device memory."""
import numpy as np
import pytest

from reak_amd import scenarios

pytestmark = pytest.mark.gpu

QS_VERTICES, DYN_VERTICES, STAR_VERTICES = 300, 200, 250


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


def _qs_space(L, c1, n_dof=3, min_interval=None):
    lo, hi = c1.meta["lower"], c1.meta["upper"]
    return L.make_qs_space(n_dof, lo[:n_dof], hi[:n_dof], c1.meta["min_interval"] if min_interval is None else min_interval)


@pytest.fixture(scope="module")
def qs_ref(oracle, c1):
    """seed -> (stats, tree) of the sequential planner in C1's quasi-static space"""
    osc = oracle.OracleScene(c1)
    ref = {}
    for seed in (1, 2):
        rc, rout, rtree = osc.rrt_qs(c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"],
                                     c1.rrt_params(seed=seed, max_vertices=QS_VERTICES))
        assert rc == 0 and rout.num_vertices == QS_VERTICES + 1
        ref[seed] = (rout, rtree)
    return ref


@pytest.fixture(scope="module")
def dyn_ref(L, ctx, oracle, c2):
    """seed -> (stats, tree) of the sequential planner in C2's dynamic space, and the tree of a planner that ran alone"""
    osc, sc = oracle.OracleScene(c2), L.Scene(ctx, c2)
    ref = {}
    for seed in (1, 2):
        prm = c2.rrt_params(seed=seed, max_vertices=DYN_VERTICES)
        rc, rout, rtree = osc.rrt_dyn(prm)
        assert rc == 0 and rout.num_vertices == DYN_VERTICES + 1
        pl = L.RrtPlanner(sc, prm)
        pl.solve_planning_query()
        ref[seed] = (rout, rtree, pl.tree())
        pl.close()
    sc.close()
    return ref


@pytest.fixture(scope="module")
def star_ref(oracle, c1):
    osc = oracle.OracleScene(c1)
    rc, rout, rg = osc.rrtstar_qs(c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"],
                                  c1.rrt_params(seed=1, max_vertices=STAR_VERTICES))
    assert rc == 0
    return rout, rg


def _same_integers(st, tree, rout, rtree):
    assert (st.num_vertices, st.iterations, st.edges_checked, st.num_solutions) == (
        rout.num_vertices, rout.iterations, rout.edges_checked, rout.num_solutions)
    assert np.array_equal(tree["parent"], rtree["parent"])
    assert np.array_equal(tree["nn_seq"], rtree["nn_seq"])
    assert np.array_equal(tree["accept"], rtree["accept"])


def _check_qs(pl, ref):
    st = pl.solve_planning_query()
    tree = pl.tree()
    rout, rtree = ref
    _same_integers(st, tree, rout, rtree)
    assert np.array_equal(tree["pos"], rtree["pos"])
    assert np.array_equal(tree["goal_dist"], rtree["goal_dist"])
    assert st.best_cost == rout.best_cost
    return st, tree


def _check_dyn(pl, ref):
    st = pl.solve_planning_query()
    tree = pl.tree()
    rout, rtree, alone = ref
    _same_integers(st, tree, rout, rtree)
    assert np.allclose(tree["pos"], rtree["pos"], rtol=1e-10, atol=1e-12)
    assert np.array_equal(np.isinf(tree["goal_dist"]), np.isinf(rtree["goal_dist"]))
    assert np.array_equal(tree["pos"], alone["pos"]) and np.array_equal(tree["goal_dist"], alone["goal_dist"])


def _check_star(ps, ref):
    st = ps.solve_planning_query()
    g = ps.graph()
    rout, rg = ref
    assert (st.num_vertices, st.samples, st.loop_iterations, st.num_solutions, st.rewires, st.edges_checked) == (
        rout.num_vertices, rout.samples, rout.loop_iterations, rout.num_solutions, rout.rewires, rout.edges_checked)
    assert np.array_equal(g["near_seq"], rg["near_seq"]) and np.array_equal(g["pred"], rg["pred"])
    assert np.array_equal(g["pos"], rg["pos"]) and np.array_equal(g["dist"], rg["dist"])


def test_refused_creates_leave_nothing_behind(L, ctx, c1, qs_ref):
    """Every refusal the arguments alone can reach raises; the planner created after all four is the oracle's."""
    sc = L.Scene(ctx, c1)
    prm = c1.rrt_params(seed=1, max_vertices=QS_VERTICES)
    with pytest.raises(L.RkhError):  # a quasi-static space whose edge walk has no step
        L.RrtPlanner(sc, prm, qs=_qs_space(L, c1, min_interval=0.0))
    with pytest.raises(L.RkhError):  # a space of another dimension than the scene
        L.RrtPlanner(sc, prm, qs=_qs_space(L, c1, n_dof=2))
    with pytest.raises(L.RkhError):  # no vertex budget
        L.RrtPlanner(sc, c1.rrt_params(seed=1, max_vertices=0), qs=_qs_space(L, c1))
    with pytest.raises(L.RkhError):  # the position-level planar chain has no dynamics
        L.RrtPlanner(sc, prm)
    pl = L.RrtPlanner(sc, prm, qs=_qs_space(L, c1))
    _check_qs(pl, qs_ref[1])
    pl.close()
    sc.close()


@pytest.mark.parametrize("space", ["quasi_static", "dynamic"])
def test_overlapping_planners_own_their_memory(L, ctx, c1, c2, qs_ref, dyn_ref, space):
    """A and B live together; A goes, B solves; C comes (where A's memory was) and solves: B and C are the oracle's."""
    qs = space == "quasi_static"
    scn, ref, check = (c1, qs_ref, _check_qs) if qs else (c2, dyn_ref, _check_dyn)
    vertices = QS_VERTICES if qs else DYN_VERTICES
    sc = L.Scene(ctx, scn)

    def make(seed):
        return L.RrtPlanner(sc, scn.rrt_params(seed=seed, max_vertices=vertices), qs=_qs_space(L, c1) if qs else None)
    a, b = make(1), make(2)
    a.close()
    check(b, ref[2])
    c = make(1)
    check(c, ref[1])
    check_again = b.tree()  # B's buffers are still B's after C was created and ran
    assert np.array_equal(check_again["parent"], ref[2][1]["parent"])
    b.close()
    c.close()
    sc.close()


def test_rrtstar_next_to_rrt(L, ctx, c1, qs_ref, star_ref):
    """A graph planner and a batch planner on one scene, created, solved and destroyed in interleaved order."""
    sc = L.Scene(ctx, c1)
    qspace = _qs_space(L, c1)
    star = L.RrtStarPlanner(sc, c1.rrt_params(seed=1, max_vertices=STAR_VERTICES), qspace)
    a = L.RrtPlanner(sc, c1.rrt_params(seed=1, max_vertices=QS_VERTICES), qs=qspace)
    b = L.RrtPlanner(sc, c1.rrt_params(seed=2, max_vertices=QS_VERTICES), qs=qspace)
    a.close()
    _check_star(star, star_ref)
    _check_qs(b, qs_ref[2])
    star.close()
    c = L.RrtPlanner(sc, c1.rrt_params(seed=1, max_vertices=QS_VERTICES), qs=qspace)
    star2 = L.RrtStarPlanner(sc, c1.rrt_params(seed=1, max_vertices=STAR_VERTICES), qspace)
    _check_qs(c, qs_ref[1])
    b.close()
    _check_star(star2, star_ref)
    c.close()
    star2.close()
    sc.close()


def test_solve_destroy_solve(L, ctx, c1, qs_ref):
    """Scene, planner, solve, planner gone, scene gone -- three times over: the same result every time."""
    trees = []
    for _ in range(3):
        sc = L.Scene(ctx, c1)
        pl = L.RrtPlanner(sc, c1.rrt_params(seed=2, max_vertices=QS_VERTICES), qs=_qs_space(L, c1))
        st, tree = _check_qs(pl, qs_ref[2])
        trees.append((st.num_vertices, st.iterations, tree))
        pl.close()
        sc.close()
    for nv, it, tree in trees[1:]:
        assert (nv, it) == trees[0][:2]
        for key in ("pos", "parent", "nn_seq", "accept", "goal_dist"):
            assert np.array_equal(tree[key], trees[0][2][key])
