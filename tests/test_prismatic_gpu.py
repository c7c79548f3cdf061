"""Prismatic joints in 3D chains on the GPU: scene acceptance and refusals, the HIP kernels (f-eval, distance query, RK4
steer, quasi-static edge walk) against the test-side restatement (tests/kte_ref.py: the oracle's KteChain does not know
prismatic_joint_3D) plus the oracle's closed-form pair distances, and every planner on the CRS A465 track scene."""
import ctypes as C

import numpy as np
import pytest

import kte_ref
from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


@pytest.fixture(scope="module")
def track():
    return scenarios.make_crs_a465_track()


def _rprp(seed=4, n_obstacles=16):
    """Random R-P-R-P chain with capsule links and a few obstacles (prismatic axes NOT unit length)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = scenarios.make_random_chain(4, seed=seed, n_obstacles=n_obstacles)
    axes = [tuple(v / np.linalg.norm(v)) for v in rng.normal(size=(4, 3))]
    axes[1] = tuple(0.7 * np.array(axes[1]))
    axes[3] = tuple(1.3 * np.array(axes[3]))
    for j, op in enumerate([o for o in base.ops if o.kind == T.KTE_REVOLUTE_JOINT_3D]):
        op.axis[:] = list(axes[j])
        if j % 2 == 1:
            op.kind = T.KTE_PRISMATIC_JOINT_3D
    base.name = "rprp"
    for j in (1, 3):
        base.dyn.lower[2 * j], base.dyn.upper[2 * j] = -0.5, 0.5
    return base


def _lone_track():
    ops = scenarios.serial_chain_ops([(0.0, 0.0, 1.5)], [(0.1, 0.0, 0.2)], [2.0], [(0.3, 0.01, 0.0, 0.2, 0.0, 0.1)], [0.5],
                                     [T.KTE_PRISMATIC_JOINT_3D])
    base = T.ChainBase()
    base.pose = T.make_pose((0.1, 0.2, 0.3), (0.9, 0.1, -0.3, 0.2))
    base.acceleration[:] = [0.0, 0.0, 9.81]
    return scenarios.Scenario(name="lone", ops=ops, base=base, shapes=[], dyn=T.DynSpace(), n_dof=1, n_frames=3,
                              start=np.zeros(2), goal=np.zeros(2))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(np.asarray(b)))))


def _random_states(scn, count, seed):
    rng = np.random.default_rng(seed)
    lo = np.array([scn.dyn.lower[i] for i in range(scn.D)]) if scn.dyn.n_dof else -np.ones(scn.D)
    hi = np.array([scn.dyn.upper[i] for i in range(scn.D)]) if scn.dyn.n_dof else np.ones(scn.D)
    return rng.uniform(lo, hi, size=(count, scn.D)), rng.uniform(-20, 20, size=(count, scn.n_dof))


def _status(L, ctx, scn):
    try:
        L.Scene(ctx, scn).close()
        return 0
    except L.RkhError as e:
        return e.status


def _with_mount(scn, offset):
    """The same chain behind a mount link from the chain base (rigid_link_3D 0 -> 1): frames shift by one."""
    ops = []
    mt = T.KteOp(kind=T.KTE_RIGID_LINK_3D, coord=-1, base_frame=0, end_frame=1, joint_op=-1)
    mt.offset = T.make_pose(offset)
    ops.append(mt)
    for o in scn.ops:
        c = T.KteOp()
        C.memmove(C.addressof(c), C.addressof(o), C.sizeof(T.KteOp))
        c.base_frame = o.base_frame + 1 if o.base_frame >= 0 else -1
        c.end_frame = o.end_frame + 1 if o.end_frame >= 0 else -1
        c.joint_op = o.joint_op + 1 if o.joint_op >= 0 else -1
        ops.append(c)
    shapes = []
    for s in scn.shapes:
        c = T.Shape(kind=s.kind, anchor=s.anchor + 1 if s.anchor >= 0 else -1)
        c.pose, c.dims[:] = s.pose, list(s.dims)
        shapes.append(c)
    return scenarios.Scenario(name=scn.name + "_mount", ops=ops, base=scn.base, shapes=shapes, dyn=scn.dyn, n_dof=scn.n_dof,
                              n_frames=scn.n_frames + 1, start=scn.start, goal=scn.goal, meta=dict(scn.meta))


# ---------------------------------------------------------------------------------------------- scene
def test_scene_accepts_prismatic_serial_chains(L, ctx, track):
    """The CRS A465 on its track, a random R-P-R-P chain and the track chain behind a mount link are scenes."""
    for scn in (track, _rprp(), _lone_track(), _with_mount(track, (0.2, 0.0, 0.0))):
        sc = L.Scene(ctx, scn)
        assert sc.num_pairs > 0 or not scn.shapes
        sc.close()


def test_scene_refuses_prismatic_joints_outside_serial_chains(L, ctx, track):
    """RKH_ERR_UNSUPPORTED (-5) for: a prismatic joint in a branching chain, with a flexible_beam_3D, with mesh shapes,
    a plane paired with a shape a prismatic joint carries, and a prismatic op in a planar chain."""
    # branching: the dual arm of C4 with a prismatic first joint
    c4 = scenarios.make_c4(world_seed=1, n_obstacles=10)
    next(o for o in c4.ops if o.kind == T.KTE_REVOLUTE_JOINT_3D).kind = T.KTE_PRISMATIC_JOINT_3D
    assert _status(L, ctx, c4) == -5
    # beam: the track with a tether from its tip to the world
    beam = scenarios.make_crs_a465_track(n_obstacles=5)
    beam.ops.append(scenarios.flexible_beam_op(2 * beam.n_dof, T.make_pose((0.0, -2.0, 1.5)), 0.3, 1e3, 10.0))
    assert _status(L, ctx, beam) == -5
    # mesh shapes
    mesh = scenarios.make_crs_a465_track(n_obstacles=5)
    verts = scenarios.box_as_mesh([0.2, 0.2, 0.2])
    s = T.Shape(kind=T.SHAPE_MESH, anchor=-1)
    s.pose = T.make_pose((1.0, -2.0, 0.5))
    s.dims[:] = [0.0, float(len(verts)), 0.0]
    mesh.shapes.append(s)
    mesh.mesh_vertices = np.asarray(verts, dtype=np.float64)
    assert _status(L, ctx, mesh) == -5
    # a floor plane under the track robot
    plane = scenarios.make_crs_a465_track(n_obstacles=5)
    s = T.Shape(kind=T.SHAPE_PLANE, anchor=-1)
    s.pose = T.make_pose((0.0, 0.0, 0.0))
    s.dims[:] = [20.0, 20.0, 0.0]
    plane.shapes.append(s)
    assert _status(L, ctx, plane) == -5
    # planar chain with a prismatic op in place of a revolute_joint_2D
    c1p = scenarios.make_c1_planar(world_seed=1)
    c1p.ops[0].kind = T.KTE_PRISMATIC_JOINT_3D
    assert _status(L, ctx, c1p) == -5
    c1p = scenarios.make_c1_planar(world_seed=1)
    c1p.ops[2].kind = T.KTE_PRISMATIC_JOINT_3D
    assert _status(L, ctx, c1p) == -5
    # and the same scenes without the prismatic joint stay what they were
    assert _status(L, ctx, scenarios.make_c4(world_seed=1, n_obstacles=10)) == 0


# ---------------------------------------------------------------------------------------------- f-eval
@pytest.mark.parametrize("which", ["track", "rprp", "lone"])
def test_state_derivative_matches_restatement(L, ctx, track, which):
    """rkh_state_derivative (pd, M, f) on 256 random states against the restatement, 1e-11 relative (sincos only)."""
    scn = {"track": track, "rprp": _rprp(), "lone": _lone_track()}[which]
    x, u = _random_states(scn, 256, 7)
    sc = L.Scene(ctx, scn)
    pd, M, f = sc.state_derivative(x, u)
    ch = kte_ref.Chain(scn)
    for i in range(len(x)):
        p2, M2, f2 = ch.state_derivative(x[i], u[i])
        assert _rel(pd[i], p2) <= 1e-11 and _rel(M[i], M2) <= 1e-11 and _rel(f[i], f2) <= 1e-11, i
    sc.close()


# ---------------------------------------------------------------------------------------------- distances
@pytest.mark.parametrize("which", ["track", "rprp"])
def test_min_distance_matches_restatement(L, ctx, oracle, track, which):
    """rkh_min_distance against the restatement's shape poses + the oracle's closed-form pair distances: 1e-12, and
    the same sign wherever |d| > 1e-9."""
    scn = {"track": track, "rprp": _rprp()}[which]
    x, _ = _random_states(scn, 48, 9)
    x[: len(x) // 2, 0] = np.linspace(-0.2, 2.5, len(x) // 2) if which == "track" else x[: len(x) // 2, 0]
    sc = L.Scene(ctx, scn)
    d = sc.min_distance(x)
    dist = kte_ref.Distances(kte_ref.Chain(scn), oracle)
    for i in range(len(x)):
        r = dist.min_distance(x[i])
        assert abs(d[i] - r) <= 1e-12 * max(1.0, abs(r)), (i, d[i], r)
        if abs(r) > 1e-9:
            assert np.sign(d[i]) == np.sign(r)
    sc.close()


def test_root_prismatic_equals_a_mount_link_on_the_oracle(L, ctx, oracle, track):
    """Independent of the restatement: the track robot at q0 is the 6-R arm behind a mount link with offset q0 a (then
    link_0's identity offset); the oracle's own scene gives the distance (orc_min_distance)."""
    sc = L.Scene(ctx, track)
    axes, _, offsets, masses, inertias, jin = scenarios.crs_like_chain()
    arm_ops = scenarios.serial_chain_ops(axes, offsets, masses, inertias, jin)
    rng = np.random.default_rng(3)
    for q0 in (-0.1, 0.4, 1.1, 2.0, 2.4):
        x = np.zeros(track.D)
        x[0] = q0
        x[2::2] = rng.uniform(-1.5, 1.5, size=6)
        arm = scenarios.Scenario(name="arm", ops=arm_ops, base=track.base, shapes=[], dyn=track.dyn, n_dof=6, n_frames=13,
                                 start=np.zeros(12), goal=np.zeros(12))
        arm.shapes = [s for s in track.shapes]
        arm = _with_mount(arm, (q0 * 1.0, 0.0, 0.0))
        for s in arm.shapes:  # track frames 2j+1 (joint j >= 1) -> arm frames 2(j-1)+1, shifted by the mount: 2j
            if s.anchor >= 0:
                s.anchor -= 2
        osc = oracle.OracleScene(arm)
        r = osc.min_distance(x[2:])[0]
        d = sc.min_distance(x)[0]
        assert abs(d - r) <= 1e-12 * max(1.0, abs(r)), (q0, d, r)
    sc.close()


# ---------------------------------------------------------------------------------------------- steer / walk
def test_propagate_matches_restatement_rk4_without_obstacles(L, ctx, track):
    """rkh_propagate with record on the obstacle-free track robot: states to 1e-10 relative, the same steps_free."""
    scn = scenarios.make_crs_a465_track(n_obstacles=0)
    scn.shapes = []
    sc = L.Scene(ctx, scn)
    a, _ = _random_states(scn, 6, 21)
    b, _ = _random_states(scn, 6, 22)
    a[:, 1::2] *= 0.3
    out, steps, rec = sc.steer_position_toward(a, b, 1.0, record=True)
    ch = kte_ref.Chain(scn)
    for i in range(len(a)):
        x, n_free, r, _ = kte_ref.steer(ch, _NoShapes(), scn.dyn, a[i], b[i])
        assert steps[i] == n_free, i
        assert _rel(out[i], x) <= 1e-10 and _rel(rec[i, : n_free + 1], r) <= 1e-10, i
    sc.close()


class _NoShapes:
    def min_distance(self, x):
        return np.inf


def test_propagate_with_obstacles_matches_restatement(L, ctx, oracle, track):
    """With obstacles: the same steps_free wherever no tested state comes within 1e-9 of contact."""
    sc = L.Scene(ctx, track)
    ch = kte_ref.Chain(track)
    dist = kte_ref.Distances(ch, oracle)
    rng = np.random.default_rng(31)
    a = np.zeros((6, track.D))
    b = np.zeros((6, track.D))
    a[:, 0::2] = rng.uniform([-0.2] + [-1.0] * 6, [2.5] + [1.0] * 6, size=(6, 7))
    b[:, 0::2] = rng.uniform([-0.2] + [-2.5] * 6, [2.5] + [2.5] * 6, size=(6, 7))
    out, steps, rec = sc.steer_position_toward(a, b, 1.0, record=True)
    compared = 0
    for i in range(len(a)):
        x, n_free, r, dmins = kte_ref.steer(ch, dist, track.dyn, a[i], b[i])
        if any(abs(d) <= 1e-9 for d in dmins):
            continue
        compared += 1
        assert steps[i] == n_free, i
        assert _rel(out[i], x) <= 1e-10
    assert compared >= 4
    sc.close()


def test_edge_check_matches_restatement_walk(L, ctx, oracle, track):
    """rkh_edge_check (the quasi-static walk) against the restatement's min_interval walk: the same points, the same
    number of is_free calls."""
    sc = L.Scene(ctx, track)
    ch = kte_ref.Chain(track)
    dist = kte_ref.Distances(ch, oracle)
    lo, hi, mi = track.meta["lower"], track.meta["upper"], track.meta["min_interval"]
    rng = np.random.default_rng(41)
    a = rng.uniform(lo, hi, size=(12, 7)) * np.array([1.0] + [0.4] * 6)
    b = rng.uniform(lo, hi, size=(12, 7))
    out, nchk = sc.move_position_toward(lo, hi, mi, a, b)
    for i in range(len(a)):
        r, n = kte_ref.qs_move(ch, dist, lo, hi, mi, a[i], b[i])
        assert np.array_equal(out[i], r) and nchk[i] == n, (i, nchk[i], n)
    sc.close()


# ---------------------------------------------------------------------------------------------- planners
def test_quasi_static_rrt_uses_the_track(L, ctx, oracle, track):
    """Quasi-static RRT on the track robot reaches the goal 2 m down the track: its path moves the track joint by more
    than 1.5 m, and every path vertex is free by the reference."""
    sc = L.Scene(ctx, track)
    lo, hi, mi = track.meta["lower"], track.meta["upper"], track.meta["min_interval"]
    prm = track.rrt_params(seed=1, max_vertices=20000, max_results=1)
    prm.start[:7] = [0.0] * 7
    prm.goal[:7] = list(track.goal[0::2])
    for i in range(7, len(prm.start)):
        prm.start[i] = prm.goal[i] = 0.0
    pl = L.RrtPlanner(sc, prm, qs=L.make_qs_space(7, lo, hi, mi))
    st = pl.solve_planning_query()
    assert st.num_solutions >= 1
    path, _ = pl.solution()
    pos = pl.tree()["pos"]
    q0 = np.append(pos[path, 0], track.goal[0])  # the tree's part of the path, then the goal it connects to
    assert q0.max() - q0.min() > 1.5
    dist = kte_ref.Distances(kte_ref.Chain(track), oracle)
    for v in path:
        x = np.zeros(14)
        x[0::2] = pos[v]
        assert kte_ref.in_bounds(pos[v], lo, hi) and dist.is_free(x)
    pl.close()


def _check_vertices(pos, scn, oracle):
    lo = [scn.dyn.lower[i] for i in range(scn.D)]
    hi = [scn.dyn.upper[i] for i in range(scn.D)]
    dist = kte_ref.Distances(kte_ref.Chain(scn), oracle)
    for p in pos:
        assert kte_ref.in_bounds(p, lo, hi) and dist.is_free(p)


def test_dynamic_rrt_on_the_track(L, ctx, oracle, track):
    """Dynamic RRT (2 000 vertices): every vertex in its box and free by the reference; two runs give identical trees;
    a batch of 8 problems equals the 8 single-problem runs bit for bit."""
    sc = L.Scene(ctx, track)
    prms = [track.rrt_params(seed=s, max_vertices=2000) for s in range(1, 9)]
    singles = []
    for p in prms:
        pl = L.RrtPlanner(sc, p)
        pl.solve_planning_query()
        singles.append(pl.tree())
        pl.close()
    assert len(singles[0]["pos"]) >= 2000
    pl = L.RrtPlanner(sc, prms[0])
    pl.solve_planning_query()
    again = pl.tree()
    pl.close()
    assert all(np.array_equal(again[k], singles[0][k]) for k in ("pos", "parent", "accept"))
    batch = L.RrtPlanner(sc, prms)
    batch.solve_planning_query()
    for i in range(8):
        t = batch.tree(i)
        assert all(np.array_equal(t[k], singles[i][k]) for k in ("pos", "parent", "nn_seq", "accept")), i
    batch.close()
    _check_vertices(singles[0]["pos"], track, oracle)
    sc.close()


def test_dynamic_rrtstar_and_prm_on_the_track(L, ctx, oracle, track):
    """RRT* and PRM over the dynamic space of the track robot: vertices in the box and free by the reference, runs
    repeat bit for bit, a batch of 8 equals the single runs.  Edge weights are Euclidean lengths of the travelled
    steer (planning_visitors.hpp:385-395: a connection may stop conn_tol short of its target): RRT*'s
    dist[v] - dist[pred] and PRM's weights lie in [|u - v| / (1 + tol), |u - v| / (1 - tol)]."""
    sc = L.Scene(ctx, track)
    prms = [track.rrt_params(seed=s, max_vertices=300) for s in range(1, 9)]
    tol = prms[0].conn_tol
    runs = []
    for p in prms:
        pl = L.RrtStarPlanner(sc, p, track.dyn)
        pl.solve_planning_query()
        runs.append(pl.graph())
        pl.close()
    pl = L.RrtStarPlanner(sc, prms[0], track.dyn)
    pl.solve_planning_query()
    g = pl.graph()
    pl.close()
    assert all(np.array_equal(g[k], runs[0][k]) for k in g)
    batch = L.RrtStarPlanner(sc, prms, track.dyn)
    batch.solve_planning_query()
    for i in range(8):
        gi = batch.graph(i)
        assert all(np.array_equal(gi[k], runs[i][k]) for k in gi), i
    batch.close()
    g = runs[0]
    conn = [v for v in range(1, len(g["pos"])) if g["pred"][v] != 0xFFFFFFFF]
    assert len(conn) > 100
    exact = 0
    for v in conn:
        p = g["pred"][v]
        seg, dw = kte_ref.euclid(g["pos"][v], g["pos"][p]), g["dist"][v] - g["dist"][p]
        assert seg / (1.0 + tol) - 1e-9 <= dw <= seg / (1.0 - tol) + 1e-9, v
        exact += g["dist"][v] == g["dist"][p] + seg
    assert exact > len(conn) // 2  # a vertex created by its nearest neighbour's steer: its end point, exactly
    _check_vertices(g["pos"], track, oracle)

    pprms = [track.prm_params(sampling_radius=1.0, seed=s, max_vertices=200) for s in range(1, 9)]
    runs = []
    for p in pprms:
        pl = L.PrmPlanner(sc, p, track.dyn)
        pl.solve_planning_query()
        runs.append(pl.graph())
        pl.close()
    pl = L.PrmPlanner(sc, pprms[0], track.dyn)
    pl.solve_planning_query()
    g = pl.graph()
    pl.close()
    assert all(np.array_equal(g[k], runs[0][k]) for k in g)
    batch = L.PrmPlanner(sc, pprms, track.dyn)
    batch.solve_planning_query()
    for i in range(8):
        gi = batch.graph(i)
        assert all(np.array_equal(gi[k], runs[i][k]) for k in gi), i
    batch.close()
    g = runs[0]
    assert len(g["edge_w"]) > 20
    for u, v, w in zip(g["edge_u"], g["edge_v"], g["edge_w"]):
        seg = kte_ref.euclid(g["pos"][u], g["pos"][v])
        assert seg / (1.0 + tol) - 1e-9 <= w <= seg / (1.0 - tol) + 1e-9
    _check_vertices(g["pos"], track, oracle)
    sc.close()
