"""The carried clearance of the two-lanes steer kernels (propagate_pair.hip) on the GPU: the bound the proximity test
returns is a lower bound on the oracle's distance, and steering with it -- skipping the tests it settles -- changes
nothing: end states, free-step counts, records and trees are bit-identical with RKH_STEER_CLEARANCE=0, which tests
every step, and equal to the oracle's.  Premises without a GPU: tests/test_steer_clearance_cpu.py."""
import numpy as np
import pytest

import steer_filter_scenes as S
from reak_amd import scenarios

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


def switch(monkeypatch, on):
    if on:
        monkeypatch.delenv("RKH_STEER_CLEARANCE", raising=False)
    else:
        monkeypatch.setenv("RKH_STEER_CLEARANCE", "0")


@pytest.mark.parametrize("M", (0.0, 1e5), ids=lambda M: "M%g" % M)
def test_clearance_is_a_lower_bound_on_the_distance(L, ctx, oracle, M):
    """C2 at the origin and moved by 1e5 m: the first 4 096 states of the 60 000-state sample and its near-hit and
    near-miss sets (within 5 mm of contact).  The clearance of the device code is at most the oracle's minimum distance
    wherever it is positive, not positive for any state the oracle finds in collision, and positive for at least half of
    the free states -- which are mostly more than 5 cm clear (premise, checked with the oracle)."""
    c2, x, d0 = S.far_sample(oracle)
    scn = S.far_world(c2, M)
    sc, osc = L.Scene(ctx, scn), oracle.OracleScene(scn)
    hits, misses = S.near_contact_sets(osc, x, d0, S.verdict_band(scn))
    assert len(hits) >= 120 and len(misses) >= 120
    states = np.concatenate([x[:4096], hits, misses])
    d = osc.min_distance(states)
    c = sc.proximity_clearance(states)
    sc.close()
    free, hit, pos = d > 0, d < 0, c > 0
    print("M=%g: %d states, %d free (%d more than 5 cm clear), %d in collision; clearance positive for %d of the free, "
          "largest clearance - distance where positive %.3g, largest clearance of a state in collision %.3g"
          % (M, len(states), free.sum(), (d > 0.05).sum(), hit.sum(), (pos & free).sum(),
             (c[pos] - d[pos]).max() if pos.any() else 0.0, c[hit].max() if hit.any() else 0.0))
    assert (d[free] > 0.05).sum() > 0.5 * free.sum()
    assert (c[pos] <= d[pos]).all()
    assert (c[hit] <= 0).all()
    assert (pos & free).sum() >= 0.5 * free.sum()


def test_steered_edges_are_bit_identical_with_the_switch_off(L, ctx, oracle, monkeypatch):
    """529 edges of C2, 209 of them starting within 5 mm of an obstacle, on the two-lanes mapping: end states, free-step
    counts and the recorded states of every step are identical with the clearance carried and with every step tested; the
    free-step counts are the oracle's; and the counters show that steps were settled by the bound and that tests ran."""
    c2 = S.far_sample(oracle)[0]
    a, b = S.far_edges(oracle)
    sc, osc = L.Scene(ctx, c2), oracle.OracleScene(c2)
    monkeypatch.setenv("RKH_LANES_PER_EDGE", "2")
    runs, counts = {}, {}
    for on in (True, False):
        switch(monkeypatch, on)
        before = sc.steer_clearance_counts()
        runs[on] = sc.steer_position_toward(a, b, record=True)
        assert L.steer_mapping_name() == "pair"
        after = sc.steer_clearance_counts()
        counts[on] = (after[0] - before[0], after[1] - before[1])
    sc.close()
    print("edge-steps settled by the bound / wave-steps tested: on", counts[True], "off", counts[False])
    for got, want in zip(runs[True], runs[False]):
        assert np.array_equal(got, want)
    _, _, rsteps, _ = osc.steer(a, b)
    assert np.array_equal(runs[True][1], rsteps)
    assert counts[True][0] > 0 and counts[True][1] > 0
    assert counts[False][0] == 0 and counts[False][1] > counts[True][1]


def test_stepwise_planner_is_bit_identical_with_the_switch_off(L, ctx, monkeypatch):
    """3 problems x 1 500 vertices on C2 with every round on the two-lanes mapping (RKH_LANE_THRESHOLD=1: rounds this
    small otherwise go to the one-wave kernels; 0 would size the one-wave launches' grids to nothing) and, with
    RKH_STEER_SPLIT_MIN_EDGES=0, through the step-wise launches: segment sizes are no multiples of 32, so both parts of the survivor lists end in partial waves.  Trees and counters
    are identical with the clearance carried and with every step tested, and identical to the whole-edge launches'
    (test_stepwise_and_whole_edge_steer_launches_do_not_change_results's other form); both counters move."""
    c2 = scenarios.make_c2(world_seed=1)
    prms = [c2.rrt_params(seed=170 + i, max_vertices=1500) for i in range(3)]
    monkeypatch.setenv("RKH_LANE_THRESHOLD", "1")
    runs = {}
    for name, split_min_edges, on in (("stepwise", "0", True), ("stepwise, every step tested", "0", False),
                                      ("whole", "1000000000", True)):
        monkeypatch.setenv("RKH_STEER_SPLIT_MIN_EDGES", split_min_edges)
        switch(monkeypatch, on)
        sc = L.Scene(ctx, c2)
        pl = L.RrtPlanner(sc, prms)
        pl.solve_planning_query()
        runs[name] = {"stats": [(int(s.num_vertices), int(s.iterations), int(s.edges_checked), int(s.num_solutions),
                                 float(s.best_cost)) for s in pl.all_stats],
                      "trees": [pl.tree(i) for i in range(3)], "steps": pl.steer_steps(),
                      "counts": sc.steer_clearance_counts()}
        pl.close()
        sc.close()
        print(name, "executed edge-steps", runs[name]["steps"], "settled by the bound / wave-steps tested", runs[name]["counts"])
    ref = runs["stepwise"]
    for name in ("stepwise, every step tested", "whole"):
        assert runs[name]["stats"] == ref["stats"], name
        assert runs[name]["steps"] == ref["steps"], name
        for t, r in zip(runs[name]["trees"], ref["trees"]):
            for key in ("parent", "nn_seq", "accept", "pos", "goal_dist"):
                assert np.array_equal(t[key], r[key]), (name, key)
    assert ref["counts"][0] > 0 and ref["counts"][1] > 0
    assert runs["whole"]["counts"][0] > 0 and runs["whole"]["counts"][1] > 0
    assert runs["stepwise, every step tested"]["counts"][0] == 0


@pytest.mark.parametrize("kind", ("plane", "prismatic"))
def test_scenes_the_bound_does_not_cover_test_every_step(L, ctx, monkeypatch, kind):
    """C2 above a floor plane (no finite bounding radius) and a 6-joint chain with two prismatic joints (no lever arm):
    has_clearance = 0.  96 steered edges on the two-lanes mapping settle no step by the bound, the diagnostic clearance
    is 0, and the switch changes nothing."""
    scn = scenarios.make_c2(world_seed=1, floor=-0.45) if kind == "plane" else S.prismatic_chain6()
    a, b = S.random_states(scn, 96, 51), S.random_states(scn, 96, 52)
    sc = L.Scene(ctx, scn)
    monkeypatch.setenv("RKH_LANES_PER_EDGE", "2")
    runs = {}
    for on in (True, False):
        switch(monkeypatch, on)
        runs[on] = sc.steer_position_toward(a, b, record=True)
        assert L.steer_mapping_name() == "pair"
    settled, tested = sc.steer_clearance_counts()
    assert (sc.proximity_clearance(a) == 0).all()
    sc.close()
    print(kind, "free steps", runs[True][1].sum(), "settled by the bound", settled, "wave-steps tested", tested)
    for got, want in zip(runs[True], runs[False]):
        assert np.array_equal(got, want)
    assert runs[True][1].sum() > 0 and settled == 0
