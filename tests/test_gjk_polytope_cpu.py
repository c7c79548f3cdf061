"""The oracle's support-map query (oracle/reak_gjk.hpp, the CPU twin of reak_amd/csrc/gjk_device.h) against the exact
polytope distance of tests/polytope_ref.py -- a reference that is no GJK, so a fault of the algorithm itself shows.

Bounds: free pairs 1e-10 absolute (the project's bound for GJK against the closed forms; the reference's own error at
these sizes is about 1e-16), colliding pairs exactly -(rA + rB) - 1e-9.  No case is excluded."""
import numpy as np
import pytest

import polytope_ref as P

TOL = 1e-10


def _report(cs, got):
    bad = cs.check(got, TOL)
    return "%d of %d wrong (index, case, reference, got):\n" % (len(bad), len(cs)) + "\n".join(map(str, bad[:20]))


@pytest.fixture(scope="module")
def families():
    return {"gap": P.gap_placed_cases(), "penetrating": P.penetrating_cases(), "edge": P.edge_cases(),
            "partner": P.partner_cases(), "capsule_box": P.capsule_box_cases()}


def test_the_two_reference_formulations_agree(families):
    """Hull features against all vertex triples and pairs, to 1e-13, on every hand-built free case, a spread of the
    gap-placed and partner cases, and ten pairs of 32 x 32 vertices.  The witness certifies each value from below."""
    sub = [(families["edge"], i) for i in np.nonzero(families["edge"].free())[0]]
    sub += [(families["gap"], i) for i in range(0, len(families["gap"]), 40)]
    sub += [(families["partner"], i) for i in range(0, len(families["partner"]), 45)]
    worst = 0.0
    for cs, i in sub:
        (WA, _), (WB, _) = cs.core(cs.A[i]), cs.core(cs.B[i])
        d, pa, pb, ax = P.polytope_distance(WA, WB, with_axis=True)
        d2, _, _ = P.polytope_distance_all(WA, WB)
        scale = max(1.0, float(np.max(np.abs(WA))), float(np.max(np.abs(WB))))
        worst = max(worst, abs(d - d2) / scale)
        assert abs(d - d2) <= 1e-13 * scale, (cs.label[i], d, d2)
        assert abs(np.linalg.norm(pb - pa) - d) <= 1e-13 * scale
        assert 0.0 < P.separation(WA, WB, pa, pb, ax) <= d + 1e-13 * scale, cs.label[i]
    rng = np.random.default_rng(5)
    for _ in range(10):
        VA, VB = (P.scenarios.random_convex_mesh(rng, 32, 0.2) for _ in range(2))
        WA = VA @ P.quat_rotmat(P._rand_quat(rng)).T
        WB = VB @ P.quat_rotmat(P._rand_quat(rng)).T + rng.uniform(0.41, 0.6) * np.array([0.6, -0.64, 0.48])  # apart
        d, d2 = P.polytope_distance(WA, WB)[0], P.polytope_distance_all(WA, WB)[0]
        worst = max(worst, abs(d - d2))
        assert abs(d - d2) <= 1e-13
    print("hull features vs all triples and pairs: worst |difference| = %.3g" % worst)


def test_the_reference_knows_which_pairs_intersect(families):
    """No LP: a pair is free exactly if some direction separates the vertex sets.  Every gap-placed and partner case is
    free by construction and every penetrating case shares a point by construction; the verdict must say so, and for the
    penetrating cases so must the direction-free check that the shared point lies inside both hulls."""
    for name in ("gap", "partner"):
        cs = families[name]
        assert all(free for _, _, free in cs.cert), name
        assert np.all(cs.free())
        assert max(abs(d - s) for d, s, _ in cs.cert) <= 1e-8   # the witness direction of a 1e-8 gap is good to ~1e-8 rad
    cs = families["penetrating"]
    assert len(cs) == 300
    for i in range(len(cs)):
        (WA, _), (WB, _) = cs.core(cs.A[i]), cs.core(cs.B[i])
        d, pa, pb, ax = P.polytope_distance(WA, WB, cs.features(cs.A[i]), cs.features(cs.B[i]), with_axis=True)
        assert P.separation(WA, WB, pa, pb, ax) <= 0.0, cs.label[i]
        assert P.inside_hull(WA, cs.shared[i]) and P.inside_hull(WB, cs.shared[i], 1e-12), cs.label[i]


def test_the_reference_reproduces_the_closed_forms(oracle):
    """Sphere / box, sphere / capped cylinder and capped cylinder pairs through their cores (1, 2 and 8 points) against
    the restated reference closed forms: 1e-12 (the box enters as the mesh of its eight corners).  The reference has no
    box / box routine (proxy_query_model.cpp:366-369); boxes with a known gap are among the hand-built cases."""
    from test_oracle_kat import gjk_pair_sets

    rng = np.random.default_rng(77)
    n = 0
    for (ka, kb), (A, B) in gjk_pair_sets(rng, 150).items():
        if (ka, kb) == ("ccyl", "box"):      # the reference's own routine is a golden-section search to 1e-3 L/2
            continue
        for a, b in zip(A, B):
            (WA, ra), (WB, rb) = P.core_world(a), P.core_world(b)
            d, pa, pb, free = P.cores_distance(WA, WB)
            if free:
                assert abs(d - ra - rb - oracle.pair_distance(a, b)) <= 1e-12, (ka, kb)
                n += 1
            else:
                assert oracle.pair_distance(a, b) < 0.0
    assert n > 500


@pytest.mark.parametrize("family", ["gap", "penetrating", "edge", "partner", "capsule_box"])
def test_oracle_gjk_matches_the_exact_polytope_distance(oracle, families, family):
    """oracle.gjk_distance on every case of the family.

    gap: mesh / mesh pairs of 4-32 vertices placed 1e-2, 1e-4, 1e-6 and 1e-8 apart along the witness of a comfortable
      placement (seed 13, 360 pairs; seed 14, 120 pairs: 1920 cases).  The GJK before the certified exit got three of
      them wrong -- seed 13 pair 73 at 1e-4 (a collision), seed 13 pair 358 at 1e-4 (2.3e-4) and seed 14 pair 118 at
      1e-2 (0.0425): at the optimal face the relative stop 1e-14 |v|^2 lay below the rounding of v.(v - w), a coplanar
      fourth support point went in, and the side tests of the flat tetrahedron ran on the sign of rounding noise.
    penetrating: pairs that share a point by construction, 1e-2, 1e-4 and 1e-6 deep: exactly -(rA + rB) - 1e-9.
    edge: hand-built face / face, parallel and crossed edges, vertex / vertex, 1-4 coplanar vertices, duplicated and
      interior vertices, offsets to 1e6, scales 1e-6 to 1e3, at gaps from 1 down to 1e-12 and touching (collision).
    partner: mesh against sphere, capped cylinder and box, gap-placed, both argument orders.
    capsule_box: pairs 7500-7599 of the 10 000 random capped cylinder / box poses of test_gjk_reproduces_the_closed_forms.
      The GJK before the certified exit returned -r - 1e-9 = -0.03642 (crossing cores) for pair 7561, whose cores are
      0.0123 apart (exact value -0.02415); that test reads a value below -r as a collision on both sides and let it by."""
    cs = families[family]
    got = oracle.gjk_distance(cs.A, cs.B, cs.pool)
    free = cs.free()
    err = np.abs(got - np.array(cs.expect))
    print("%s: %d cases, %d free; worst free error %.3g" % (family, len(cs), free.sum(), err[free].max() if free.any() else 0.0))
    assert not cs.check(got, TOL), _report(cs, got)


def test_a_mesh_scene_sees_the_same_gaps(oracle):
    """The scene path (pair list, to_gjk, minimum over the pairs) on the scene of the GPU test: a capped cylinder on a
    one-link chain among mesh obstacles placed 1e-6 clear of it or 1e-6 into it, one per configuration."""
    scn, x, expect = P.gap_scene()
    d = oracle.OracleScene(scn).min_distance(x)
    assert np.array_equal(d < 0.0, expect < 0.0), (d, expect)
    assert np.max(np.abs(d - expect)) <= TOL, (d, expect)
    # each configuration's nearest obstacle is its own: three gaps of +1e-6, three of -1e-6, one pair of crossing cores
    assert np.max(np.abs(expect - np.array([1e-6, -1e-6, 1e-6, -1e-6, 1e-6, -1e-6, -0.05 - 1e-9]))) <= 1e-12
