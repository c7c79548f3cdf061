"""The collision filters of the two-lanes steer kernels (propagate_pair.hip: pair_proximity_free, behind
propagate_pair_kernel, propagate_pair_step_kernel and their rkh::prismatic forms) at their edges, against the oracle,
which has none of them: the static reach prefix, the fp32 bounding cull, the two LDS queues and the separating-axis
screen.  Each can only fail by letting a collision go unnoticed, and a missed collision is usually caught a step later,
so trees and totals do not show it: here every state is settled on its own (check_verdicts), every steered edge has the
oracle's free-step count on every mapping (check_steer), and the scenes (tests/steer_filter_scenes.py; premises in
tests/test_steer_filters_cpu.py) sit where each filter decides."""
import numpy as np
import pytest

import steer_filter_scenes as S

pytestmark = pytest.mark.gpu

MAPPINGS = ("64", "128", "16", "2")


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


def check_verdicts(sc, osc, x, band, what=""):
    """Every state of x the reference osc puts more than `band` inside an obstacle is one the two-lanes kernels' proximity
    test (rkh_diag_proximity_counts) finds in collision, and every state more than `band` clear is one it finds free:
    the two groups are counted apart, so a missed and a false collision cannot cancel.  Returns the counts."""
    hit, free, excluded = S.split_by_band(osc, x, band)
    found = sc.proximity_counts(hit)["states_in_collision"] if len(hit) else 0
    false = sc.proximity_counts(free)["states_in_collision"] if len(free) else 0
    print("%s: %d states, %d in collision of which the kernel finds %d (missed %d); %d free of which it stops %d; "
          "%d within %.2g of contact left out" % (what, len(x), len(hit), found, len(hit) - found, len(free), false, excluded, band))
    assert found == len(hit), "%s: %d of %d collisions missed" % (what, len(hit) - found, len(hit))
    assert false == 0, "%s: %d of %d free states stopped" % (what, false, len(free))
    return {"hit": len(hit), "free": len(free), "excluded": excluded}


def check_steer(L, sc, osc, a, b, monkeypatch, osc_origin=None, what=""):
    """On every mapping of the steer kernel -- one wave per edge, two waves, 16 lanes, two lanes -- the free-step counts
    of the edges a -> b are the reference's and the end states match within rtol 1e-10 and atol 1e-12.  In a shifted world
    (osc_origin = the reference of the same scene at the origin) atol is 10 times the largest difference between the two
    references' end states on these edges, at least 1e-12.  RKH_LANES_PER_EDGE=2 must report the pair mapping."""
    _, rout, rsteps, _ = osc.steer(a, b)
    atol = 1e-12
    if osc_origin is not None:
        _, oout, osteps, _ = osc_origin.steer(a, b)
        assert np.array_equal(osteps, rsteps), "%s: the reference itself stops elsewhere in the shifted world" % what
        atol = max(1e-12, 10.0 * float(np.abs(rout - oout).max()))
    for lanes in MAPPINGS:
        monkeypatch.setenv("RKH_LANES_PER_EDGE", lanes)
        out, steps, _ = sc.steer_position_toward(a, b)
        if lanes == "2":
            assert L.steer_mapping_name() == "pair"
        wrong = np.flatnonzero(steps != rsteps)
        print("%s, %s lanes: %d edges, %d with another free-step count than the reference (%d run further), atol %.3g"
              % (what, lanes, len(a), len(wrong), int((steps > rsteps).sum()), atol))
        assert len(wrong) == 0, (what, lanes, wrong[:8].tolist(), steps[wrong[:8]].tolist(), rsteps[wrong[:8]].tolist())
        assert np.allclose(out, rout, rtol=1e-10, atol=atol), (what, lanes)
    monkeypatch.delenv("RKH_LANES_PER_EDGE")
    return rsteps


def check_distances(sc, osc, scn, x):
    band = S.verdict_band(scn)
    assert np.allclose(sc.min_distance(x), osc.min_distance(x), rtol=0, atol=band)


# ---------------------------------------------------------------------------------------------- 1. far world
@pytest.mark.parametrize("M", S.FAR_OFFSETS, ids=lambda M: "M%g" % M)
def test_far_world_verdicts(L, ctx, oracle, M):
    """C2 moved by M (1, 0.75, 0.1): the states of a 60 000-state sample within 5 mm of contact on either side (191
    near-hits, 209 near-misses: picked from all 60 000), and the first 20 000 states of the sample as they come (the
    oracle at each offset is what takes the time here; the near-contact states of the other 40 000 are in the two sets
    above), each settled as the shifted oracle settles it; distances within the band.  Before the cull ran on
    base-relative coordinates it rounded absolute ones to fp32 (ulp at 1e5 m: 8 mm against a 1 mm margin), and at
    M = 1e5 the two-lanes kernels missed 3 of the 191 near-hits and 2 of the 321 collisions among the first 8192 random
    states (the slice this test settled when it found the bug; it is 20 000 now); at M = 0 and 1e3 they missed none."""
    c2, x, d0 = S.far_sample(oracle)
    scn = S.far_world(c2, M)
    sc, osc, band = L.Scene(ctx, scn), oracle.OracleScene(scn), S.verdict_band(scn)
    hits, misses = S.near_contact_sets(osc, x, d0, band)
    assert len(hits) >= 120 and len(misses) >= 120
    failed = []
    for what, states in (("near-hits", hits), ("near-misses", misses), ("all states", x[:20000])):
        try:
            check_verdicts(sc, osc, states, band, "M=%g %s" % (M, what))
        except AssertionError as e:  # every group is counted and printed before the test fails
            failed.append(str(e))
    assert not failed, failed
    check_distances(sc, osc, scn, x[:2048])
    sc.close()


@pytest.mark.parametrize("M", S.FAR_OFFSETS, ids=lambda M: "M%g" % M)
def test_far_world_steer(L, ctx, oracle, monkeypatch, M):
    """529 edges of the moved C2 world, 209 of them starting within 5 mm of an obstacle, on every mapping.  Before the
    fix the two-lanes mapping alone differed at M = 1e5 (the other mappings cull in fp64): 3 of the 529 edges ran past the
    step at which the oracle stops them."""
    c2 = S.far_sample(oracle)[0]
    a, b = S.far_edges(oracle)
    scn = S.far_world(c2, M)
    sc, osc = L.Scene(ctx, scn), oracle.OracleScene(scn)
    steps = check_steer(L, sc, osc, a, b, monkeypatch, oracle.OracleScene(c2) if M else None, "M=%g" % M)
    assert ((steps > 0) & (steps < 20)).sum() >= 20 and (steps == 20).sum() >= 20
    sc.close()


@pytest.mark.parametrize("M", S.FAR_OFFSETS, ids=lambda M: "M%g" % M)
def test_grazing_spheres(L, ctx, oracle, monkeypatch, M):
    """Contacts inside the cull's 1 mm margin, at the origin and in the moved world: 64 states, each with a sphere whose
    surface is 0.1, 1 or 5 mm inside its capsule k = i mod 6 (twin scene: outside), where the cull's lower bound equals the
    pair's distance.  All spheres together: verdicts, steered edges and distances as the oracle has them.  Then each
    sphere alone with the arm, at its own state: the one contact of that scene, 0.1 .. 5 mm deep, is found (twin: the
    state is free).  Before the fix the two-lanes kernels missed 11 of the 64 lone contacts at M = 1e5 (ten of 0.1 mm, one
    of 1 mm); with all spheres present every state has a second, deeper contact (a sphere beside the base capsule
    touches the arm in every state) and nothing showed."""
    for gap in (False, True):
        base, x = S.grazing_spheres(oracle, gap=gap)
        scn = S.far_world(base, M)
        sc, osc, band = L.Scene(ctx, scn), oracle.OracleScene(scn), S.verdict_band(scn)
        what = "M=%g %s" % (M, scn.name)
        n = check_verdicts(sc, osc, x, band, what)
        assert n["free"] >= 20 if gap else n["hit"] >= 60
        check_steer(L, sc, osc, x, S.random_states(scn, len(x), 20), monkeypatch, oracle.OracleScene(base) if M else None, what)
        check_distances(sc, osc, scn, x)
        sc.close()
        missed = []
        for i, sphere in enumerate(s for s in scn.shapes if s.anchor < 0):
            alone = S.with_shapes(scn, S.robot_shapes(scn) + [sphere], "alone")
            d = oracle.OracleScene(alone).min_distance(x[i])[0]
            assert abs(abs(d) - S.PENETRATIONS[(i // 6) % 3]) <= 1e-8 and (d > 0) == gap
            sc1 = L.Scene(ctx, alone)
            if sc1.proximity_counts(x[i])["states_in_collision"] != (0 if gap else 1):
                missed.append((i, d))
            sc1.close()
        print(what, "spheres alone: %d wrong verdicts" % len(missed), missed)
        assert not missed, missed


def test_far_world_rrt(L, ctx, oracle, monkeypatch):
    """A 700-vertex RRT (seed 3) in the C2 world 1e5 m from the origin, with the steer plan left to itself and with two
    lanes per edge on every round: vertices, iterations, edges checked, parents, accept bits and NN sequence are the
    sequential oracle's in the same world."""
    scn = S.far_world(S.far_sample(oracle)[0], 1e5)
    osc = oracle.OracleScene(scn)
    prm = scn.rrt_params(seed=3, max_vertices=700)
    rc, ro, rtree = osc.rrt_dyn(prm)
    assert rc == 0
    for lanes in (None, "2"):
        if lanes is None:
            monkeypatch.delenv("RKH_LANES_PER_EDGE", raising=False)
        else:
            monkeypatch.setenv("RKH_LANES_PER_EDGE", lanes)
        sc = L.Scene(ctx, scn)
        pl = L.RrtPlanner(sc, prm)
        st, tree = pl.solve_planning_query(), pl.tree()
        assert (st.num_vertices, st.iterations, st.edges_checked) == (ro.num_vertices, ro.iterations, ro.edges_checked), lanes
        for key in ("parent", "accept", "nn_seq"):
            assert np.array_equal(tree[key], rtree[key]), (lanes, key)
        pl.close()
        sc.close()


def test_far_world_track_robot(L, ctx, oracle, monkeypatch):
    """The prismatic pair form 1e5 m from the origin: 512 steered edges of the CRS A465 on its track, on every mapping.
    The oracle's chain does not know prismatic joints, so the reference is the test-side restatement (tests/kte_ref.py),
    recorded at both offsets (tests/golden/steer_filters_track.npz; tests/test_steer_filters_cpu.py recomputes a few
    edges).  Before the edges, pair_proximity_free<7> of the prismatic form state by state: 384 random states (4 in
    collision) and 96 recorded triples (in collision, and within 5 mm of contact on either side), each settled as the
    restatement settles it."""
    scn, ref, x = S.track_states(oracle)
    sc = L.Scene(ctx, scn)
    n = check_verdicts(sc, ref, x, S.verdict_band(scn), "track")
    assert n["hit"] >= 100 and n["free"] >= 100 and n["excluded"] <= 0.005 * len(x)
    a, b = S.track_edges()
    rec = S.track_recorded()
    steps = check_steer(L, sc, rec[S.TRACK_OFFSET], a, b, monkeypatch, rec[0.0], "track")
    assert (steps < 20).sum() >= 10 and (steps == 20).sum() >= 10
    sc.close()


def test_far_world_prismatic_chain_verdicts(L, ctx, oracle):
    """The proximity test of the rkh::prismatic two-lanes forms 1e5 m from the origin: 1500 random states of a 6-joint
    chain with two prismatic joints and 12 obstacles (406 in collision, 19 of them by less than 5 mm), each settled as
    the restatement settles it."""
    scn = S.far_world(S.prismatic_chain6(), 1e5)
    sc, ref = L.Scene(ctx, scn), S.RestatedScene(scn, oracle)
    n = check_verdicts(sc, ref, S.random_states(scn, 1500, 33), S.verdict_band(scn), "prismatic chain")
    assert n["hit"] >= 100 and n["free"] >= 100 and n["excluded"] <= 7
    sc.close()


# ---------------------------------------------------------------------------------------------- 3. crowded
def test_crowded_scene_overflows_the_first_queue(L, ctx, oracle, monkeypatch):
    """144 thin obstacles around the arm.  A wave holds 32 states and the first queue 128 entries, so 4 pairs past the
    cull per state fill it; asked for here: at least 8 per free state.  Measured: 270 per free state (107 607 pairs
    of 398 states).  The
    lanes whose entries do not fit write placeholders, keep their mask and come back after a drain: verdicts of all 1024
    states, 333 steered edges (ten whole waves and a ragged one) on every mapping, distances."""
    scn, x, a, b = S.crowded_edges(oracle)
    sc, osc, band = L.Scene(ctx, scn), oracle.OracleScene(scn), S.verdict_band(scn)
    free = S.split_by_band(osc, x, band)[1]
    c = sc.proximity_counts(free)
    print("crowded: pairs past the cull per free state", c["pairs_past_cull"] / len(free), c)
    assert len(free) >= 0.3 * len(x) and c["pairs_past_cull"] / c["states"] >= 8
    check_verdicts(sc, osc, x, band, "crowded")
    steps = check_steer(L, sc, osc, a, b, monkeypatch, None, "crowded")
    assert (steps < 20).sum() >= 10 and (steps == 20).sum() >= 10
    check_distances(sc, osc, scn, x)
    sc.close()


# ---------------------------------------------------------------------------------------------- 4. box cage
def test_box_cage_overflows_the_second_queue(L, ctx, oracle, monkeypatch):
    """Four cubes set diagonally beside every capsule: the separating-axis screen passes every (capsule, cube) pair on to
    the golden-section search.  The second queue holds 64 entries for a wave's 32 states, so 2 searches per state fill
    it; asked for here: at least 4.  Measured: 23.8 per state (24 360 searches of 1024 states; with the cubes' bounding
    spheres 2 cm clear of the capsules the bounding cull left 0.13 per state and the queue never filled, so they
    reach 4 mm into the cull's range).  The queue is then drained from inside the first
    queue's drain and the lanes that did not fit try again: verdicts of 1024 free states (they come within 1.5 um of a
    cube) and of 2048 states as they are drawn, most of them inside a cube; 512 steered edges on every mapping,
    distances."""
    scn, kept, x, b = S.cage_edges(oracle)
    assert kept >= 20
    sc, osc, band = L.Scene(ctx, scn), oracle.OracleScene(scn), S.verdict_band(scn)
    c = sc.proximity_counts(x)
    print("box cage: golden-section searches per state", c["golden_section"] / len(x), c)
    assert c["golden_section"] / c["states"] >= 4
    n = check_verdicts(sc, osc, x, band, "box cage")
    assert n["free"] == len(x)
    n = check_verdicts(sc, osc, S.cage_draws(), band, "box cage, states as drawn")
    assert n["hit"] >= 1024
    steps = check_steer(L, sc, osc, x[: len(b)], b, monkeypatch, None, "box cage")
    assert (steps < 20).sum() >= 10 and (steps == 20).sum() >= 10
    check_distances(sc, osc, scn, x)
    sc.close()


# ---------------------------------------------------------------------------------------------- 5. reach boundary
@pytest.mark.parametrize("k", S.REACH_LINKS)
def test_reach_boundary(L, ctx, oracle, monkeypatch, k):
    """A sphere delta = 1e-4 or 1e-7 inside, or outside, the static reach of robot shape k, the outermost shape of the
    scene: the arm standing straight up touches the inner one by delta.  Verdicts of q = 0 and 63 states within 0.02 rad
    of it, the edges from them on every mapping, distances; and the prefix really leaves something out
    (pairs_in_static_reach < pairs_per_state: 1 of 4 (k + 1) proxy pairs -- shape k with the near sphere -- and 0 with
    the sphere 1e-4 outside; the three far spheres are beyond every shape's reach)."""
    x = S.reach_states()
    for delta in S.REACH_DELTAS:
        for inside in (True, False):
            scn = S.reach_boundary(k, delta, inside)
            sc, osc, band = L.Scene(ctx, scn), oracle.OracleScene(scn), S.verdict_band(scn)
            n = check_verdicts(sc, osc, x, band, scn.name)
            assert (n["hit"] >= 1) == inside
            c = sc.proximity_counts(x)
            print(scn.name, "pairs in static reach", c["pairs_in_static_reach"], "of", c["pairs_per_state"])
            assert c["pairs_in_static_reach"] < c["pairs_per_state"] == sc.num_pairs
            assert c["pairs_in_static_reach"] >= 1 or not inside
            check_steer(L, sc, osc, x, S.near_states(len(x), 14, np.zeros(6), 0.3, 1.0), monkeypatch, None, scn.name)
            check_distances(sc, osc, scn, x)
            sc.close()
