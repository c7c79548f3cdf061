"""Chains with prismatic joints on the two-lanes-per-edge steer mapping (propagate_pair_prismatic.hip): the whole-edge
and the step-wise kernel against the one-wave prismatic form (bit for bit, the project's contract for mappings) and
against the test-side restatement (tests/kte_ref.py), the proximity-count probe, and the batch planner's steer plan on
the CRS A465 track robot.

Fixture chains: scenarios.make_random_chain(n, seed=4, n_obstacles=0) -- a capsule on every link, link 0 included --
with the listed joints turned prismatic (axis scaled by _SCALE[j]: not unit length; position bounds +-0.5) and, for
every prismatic joint j, two spheres of radius 0.06 where robot shape j sits with all coordinates 0 except q_j = +-0.35.
They cover a prismatic root carrying a shape, the prismatic Jacobian column on either lane of the edge, odd chains (the
spare axis row) and two prismatic columns on the same lane."""
import numpy as np
import pytest

import kte_ref
from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

_SCALE = [0.7, 1.3, 0.9, 1.1, 0.8, 1.2, 1.0]
_CHAINS = [(1, (0,)), (2, (0,)), (2, (1,)), (3, (0, 2)), (4, (1, 3)), (6, (0, 3))]
_EDGE_COUNTS = (1, 31, 32, 33, 65)  # the granularities of a 32-edge wave


def _chain(n, prism):
    scn = scenarios.make_random_chain(n, seed=4, n_obstacles=0)
    for j, op in enumerate([o for o in scn.ops if o.kind == T.KTE_REVOLUTE_JOINT_3D]):
        if j in prism:
            op.kind = T.KTE_PRISMATIC_JOINT_3D
            op.axis[:] = [_SCALE[j] * v for v in op.axis]
            scn.dyn.lower[2 * j], scn.dyn.upper[2 * j] = -0.5, 0.5
    ch = kte_ref.Chain(scn)
    spheres = []
    for j in prism:
        for t in (0.35, -0.35):
            x = np.zeros(2 * n)
            x[2 * j] = t
            robot, _ = ch.posed_shapes(x)
            s = T.Shape(kind=T.SHAPE_SPHERE, anchor=-1)
            s.pose = T.make_pose(tuple(robot[j].pose.pos))
            s.dims[:] = [0.06, 0.0, 0.0]
            spheres.append(s)
    scn.shapes = list(scn.shapes) + spheres
    scn.name = "p%d_%s" % (n, "".join(str(j) for j in prism))
    return scn


def _box(scn):
    return (np.array([scn.dyn.lower[i] for i in range(scn.D)]), np.array([scn.dyn.upper[i] for i in range(scn.D)]))


def _states(scn, count=96):
    lo, hi = _box(scn)
    return np.random.default_rng(100 + scn.n_dof).uniform(lo, hi, size=(count, scn.D))


def _edges(scn, count=65):
    lo, hi = _box(scn)
    rng = np.random.default_rng(200 + scn.n_dof)
    return rng.uniform(lo, hi, size=(count, scn.D)), rng.uniform(lo, hi, size=(count, scn.D))


def _rel(a, b):  # the _rel of tests/test_prismatic_gpu.py
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(np.asarray(b)))))


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


def _mapping(L):
    return L.steer_mapping_name()


def _scene_of(which, track):
    return track if which == "track" else _chain(*which)


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("which", _CHAINS + ["track"], ids=lambda w: w if isinstance(w, str) else "n%d_%s" % (w[0], "".join(map(str, w[1]))))
def test_pair_mapping_is_bit_identical_to_the_one_wave_form(L, ctx, track, monkeypatch, which):
    """rkh_propagate with record under RKH_LANES_PER_EDGE=2 (two lanes per edge, rkh::prismatic form) returns end
    states, steps_free and records bit-identical to the call with the variable unset (one wave per edge), for 1, 31, 32,
    33 and 65 edges; rkh_steer_mapping_name() says which mapping the plan chose."""
    scn = _scene_of(which, track)
    a, b = _edges(scn)
    sc = L.Scene(ctx, scn)
    for B in _EDGE_COUNTS:
        monkeypatch.delenv("RKH_LANES_PER_EDGE", raising=False)
        ref = sc.steer_position_toward(a[:B], b[:B], 1.0, record=True)
        assert _mapping(L) == "prismatic"
        monkeypatch.setenv("RKH_LANES_PER_EDGE", "2")
        got = sc.steer_position_toward(a[:B], b[:B], 1.0, record=True)
        assert _mapping(L) == "pair"
        for r, g, what in zip(ref, got, ("end state", "steps_free", "record")):
            assert np.array_equal(r, g), (B, what)
    sc.close()


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("which", [(2, (0,)), (3, (0, 2)), (4, (1, 3))], ids=lambda w: "n%d_%s" % (w[0], "".join(map(str, w[1]))))
def test_pair_mapping_matches_the_restatement(L, ctx, oracle, monkeypatch, which):
    """65 edges under RKH_LANES_PER_EDGE=2 against the restatement's RK4 + is_free: the same steps_free for EVERY edge
    (the restatement has no edge with a tested state within 1e-9 of contact, asserted here, so none is skipped), end
    states and records within 1e-10 relative.  The edges cover all three classes -- stopped in the first step, stopped
    on the way, all 20 steps free -- with at least 3 each (asserted from the restatement)."""
    scn = _chain(*which)
    a, b = _edges(scn)
    ch = kte_ref.Chain(scn)
    dist = kte_ref.Distances(ch, oracle)
    ref = [kte_ref.steer(ch, dist, scn.dyn, a[i], b[i]) for i in range(len(a))]
    steps_ref = np.array([r[1] for r in ref])
    n_steps = scn.dyn.steps_per_edge
    assert not any(abs(d) <= 1e-9 for r in ref for d in r[3])
    assert (steps_ref == 0).sum() >= 3 and ((steps_ref > 0) & (steps_ref < n_steps)).sum() >= 3 and (steps_ref == n_steps).sum() >= 3
    monkeypatch.setenv("RKH_LANES_PER_EDGE", "2")
    sc = L.Scene(ctx, scn)
    out, steps, rec = sc.steer_position_toward(a, b, 1.0, record=True)
    assert _mapping(L) == "pair"
    sc.close()
    print("steps_free: restatement", steps_ref.tolist(), "kernel", steps.tolist())
    assert np.array_equal(steps, steps_ref)
    for i, (x, n_free, r, _) in enumerate(ref):
        assert _rel(out[i], x) <= 1e-10 and _rel(rec[i, : n_free + 1], r) <= 1e-10, i


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("which", [(3, (0, 2)), (6, (0, 3))], ids=lambda w: "n%d_%s" % (w[0], "".join(map(str, w[1]))))
def test_proximity_counts_on_prismatic_chains(L, ctx, oracle, which):
    """rkh_diag_proximity_counts (the proximity test of the two-lanes kernels, prismatic form) on 96 states of the box:
    every state is tested, the states in collision are the ones the restatement's distance is negative for, and the
    host-side pair count is the scene's."""
    scn = _chain(*which)
    x = _states(scn)
    dist = kte_ref.Distances(kte_ref.Chain(scn), oracle)
    d = np.array([dist.min_distance(s) for s in x])
    assert 0 < (d < 0).sum() < len(x) and np.abs(d).min() > 1e-9
    sc = L.Scene(ctx, scn)
    c = sc.proximity_counts(x)
    assert c["states"] == 96
    assert c["states_in_collision"] == int((d < 0).sum())
    assert c["pairs_per_state"] == sc.num_pairs
    sc.close()


# ---------------------------------------------------------------------------------------------- 4
def _planner_run(L, ctx, scn, prms, monkeypatch, env):
    for k in ("RKH_LANES_PER_EDGE", "RKH_LANE_THRESHOLD", "RKH_STEER_SPLIT_MIN_EDGES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    # Auto alone fits each round's batch to whole passes of steer waves (RKH_WAVE_FIT): the same trees from another amount
    # of speculation.  Switched off, every mapping sees the same rounds and the executed-step counters can be compared.
    monkeypatch.setenv("RKH_WAVE_FIT", "0")
    sc = L.Scene(ctx, scn)
    pl = L.RrtPlanner(sc, prms)
    name = _mapping(L)
    pl.solve_planning_query()
    run = {"mapping": name,
           "stats": [(int(s.num_vertices), int(s.iterations), int(s.edges_checked), int(s.num_solutions), float(s.best_cost))
                     for s in pl.all_stats],
           "trees": [pl.tree(i) for i in range(len(prms))], "steps": pl.steer_steps(),
           "spec": sum(int(s.edges_speculated) for s in pl.all_stats)}
    pl.close()
    sc.close()
    return run


def _same_runs(runs):
    first = runs[0]
    for other in runs[1:]:
        assert other["stats"] == first["stats"]
        for i, (ta, tb) in enumerate(zip(first["trees"], other["trees"])):
            for key in ("pos", "parent", "nn_seq", "accept", "goal_dist"):
                assert np.array_equal(ta[key], tb[key]), (other["mapping"], i, key)
        assert other["steps"] == first["steps"]
    assert 0 < first["steps"] < 20 * 2 * first["spec"]
    assert all(s[0] >= 1500 for s in first["stats"])


# Round sizes of the runs below (8 problems, 1 500 vertices each): a problem offers clamp(4 sqrt(n), 8, b_max) candidates
# per round (batch factor 4 for at most 16 problems) plus a goal probe per vertex of the round before, so the first round
# has 8 x 8 = 64 edges and a late one (n ~ 1 400) 8 x ~150 candidates and as many probes, ~2 400 edges.  With
# RKH_LANE_THRESHOLD=512 the rounds up to n ~ 64 per problem stay on the one-wave form and the later ones -- most of the
# tree -- take the two-lanes form, step-wise at every size with RKH_STEER_SPLIT_MIN_EDGES=0.
_CROSSING = {"RKH_LANE_THRESHOLD": "512", "RKH_STEER_SPLIT_MIN_EDGES": "0"}


def test_batch_planner_on_the_track_robot_gives_the_same_trees_on_every_mapping(L, ctx, track, monkeypatch):
    """Eight dynamic RRT problems on the CRS A465 track robot (7 joints: one wave per edge when nothing is asked for),
    with RKH_LANES_PER_EDGE=2 (whole-edge two-lanes launches on every round) and with RKH_LANES_PER_EDGE=0 and the round
    sizes above (one-wave rounds, then step-wise two-lanes rounds): positions, parents, NN sequences, accept bits, goal
    probes, stats and the executed-step counter are identical, and the plan reports `prismatic`, `pair`, `auto`."""
    prms = [track.rrt_params(seed=s, max_vertices=1500) for s in range(1, 9)]
    runs = [_planner_run(L, ctx, track, prms, monkeypatch, env)
            for env in ({}, {"RKH_LANES_PER_EDGE": "2"}, dict(_CROSSING, RKH_LANES_PER_EDGE="0"))]
    assert [r["mapping"] for r in runs] == ["prismatic", "pair", "auto"]
    _same_runs(runs)


def test_batch_planner_default_on_a_six_joint_prismatic_chain(L, ctx, monkeypatch):
    """A chain of at most 6 joints takes Auto by default, prismatic or not: the (6, {0, 3}) chain with only
    RKH_LANE_THRESHOLD set (rounds cross from the one-wave form into the two-lanes form, whole-edge: they stay far below
    the step-wise form's default size) and with the step-wise form forced, against RKH_LANES_PER_EDGE=128, one wave per
    edge."""
    scn = _chain(6, (0, 3))
    prms = [scn.rrt_params(seed=s, max_vertices=1500) for s in range(1, 9)]
    runs = [_planner_run(L, ctx, scn, prms, monkeypatch, env)
            for env in ({"RKH_LANES_PER_EDGE": "128"}, {"RKH_LANE_THRESHOLD": "512"}, _CROSSING)]
    assert [r["mapping"] for r in runs] == ["prismatic", "auto", "auto"]
    _same_runs(runs)


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("lanes", [None, "2", "128"])
def test_feval_cycle_probe_still_refuses_prismatic_scenes(L, ctx, monkeypatch, lanes):
    scn = _chain(3, (0, 2))
    if lanes is None:
        monkeypatch.delenv("RKH_LANES_PER_EDGE", raising=False)
    else:
        monkeypatch.setenv("RKH_LANES_PER_EDGE", lanes)
    sc = L.Scene(ctx, scn)
    with pytest.raises(L.RkhError):
        sc.diag_feval_cycles(np.zeros((32, scn.D)), np.zeros((32, scn.n_dof)), iters=1)
    sc.close()
