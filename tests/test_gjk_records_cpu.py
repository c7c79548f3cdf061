"""The record of a support-map (GJK) pair -- gjk_record of reak_amd/csrc/gjk_device.h through pair_record<true> of
proximity_record_device.h, compiled for the host (tests/cpp/gjk_record_host.cpp) -- on the case families of
tests/polytope_ref.py, held against the certificate of tests/gjk_records.py (1e-12 throughout, measured against the exact
polytope distance and never against the query).  No GPU.

Families: edge (118 hand-built degenerate pairs: parallel faces and edges, flat and one-point sets, offsets to 2^20,
touching pairs), penetrating (300), partner (1440: mesh against sphere, capped cylinder, box, both orders), gap (1440:
mesh / mesh at gaps of 1e-2 .. 1e-8, seed 13) and capsule_box (100 capped cylinder / box pairs)."""
import numpy as np
import pytest

import gjk_records as G
import polytope_ref as P

FAMILIES = ["edge", "penetrating", "partner", "gap", "capsule_box"]
UNIQUE = ("gap", "partner")   # random attitudes: the closest pair is unique, the points themselves can be compared


@pytest.fixture(scope="module")
def families():
    return {"edge": P.edge_cases(), "penetrating": P.penetrating_cases(), "partner": P.partner_cases(),
            "gap": P.gap_placed_cases(seeds=P.GAP_SEEDS[:1]), "capsule_box": P.capsule_box_cases()}


@pytest.fixture(scope="module")
def records(families):
    return {k: G.host_records(cs.A, cs.B, cs.pool) for k, cs in families.items()}


def test_the_families_have_the_sizes_the_figures_were_taken_on(families):
    assert [len(families[k]) for k in FAMILIES] == [118, 300, 1440, 1440, 100]


@pytest.mark.parametrize("family", FAMILIES)
def test_host_records_hold_the_certificate(families, records, family):
    """Every case: the certificate; dist bit-equal to gjk_distance of the same build; on the families with a unique
    closest pair the points are the reference's to 1e-10 max(1, |p|inf) as well."""
    cs, rec = families[family], records[family]
    w = G.certify_family(cs, rec, family)
    same = np.array_equal(rec["dist"].view(np.uint64), rec["gjk"].view(np.uint64))
    print("%s: dist bit-equal to gjk_distance: %s" % (family, same))
    if family in UNIQUE:
        r1, r2 = G.reference_points(cs)
        e1, e2 = G.point_error(rec["point1"], r1), G.point_error(rec["point2"], r2)
        print("%s: points against the reference's: point1 %.3g point2 %.3g" % (family, e1, e2))
    assert not w.bad, "%d of %d miss the certificate:\n" % (len(w.bad), w.n) + "\n".join(map(str, w.bad[:10]))
    assert same
    assert w.n_apart == int(np.sum(cs.free()))  # the reference's verdict here is the families' own
    if family in UNIQUE:
        assert e1 <= G.POINT_TOL and e2 <= G.POINT_TOL


@pytest.mark.parametrize("family", FAMILIES)
def test_swapping_the_arguments_swaps_the_points(families, records, family):
    """gjk_record(B, A): the certificate holds that way round too and the distances agree to 1e-12 (crossing cores:
    exactly); where the closest pair is unique the points are the swapped points to 1e-10 max(1, |p|inf)."""
    cs, rec = families[family], records[family]
    back = G.host_records(cs.B, cs.A, cs.pool)
    w = G.certify_family(cs, back, family + " swapped", swap=True)
    e_d = float(np.max(np.abs(back["dist"] - rec["dist"])))
    crossing = ~cs.free()
    print("%s: |dist(B, A) - dist(A, B)| max %.3g" % (family, e_d))
    if family in UNIQUE:
        e1, e2 = G.point_error(back["point2"], rec["point1"]), G.point_error(back["point1"], rec["point2"])
        print("%s: swapped points against the points: %.3g %.3g" % (family, e1, e2))
    assert not w.bad, "%d of %d miss the certificate:\n" % (len(w.bad), w.n) + "\n".join(map(str, w.bad[:10]))
    assert e_d <= G.TOL and np.array_equal(back["dist"][crossing], rec["dist"][crossing])
    if family in UNIQUE:
        assert e1 <= G.POINT_TOL and e2 <= G.POINT_TOL


def test_the_closed_form_form_still_has_no_record_for_a_mesh_pair(families):
    """pair_record<false> with a vertex pool is pair_record(routine, s1, s2): +inf for PR_GJK."""
    cs = families["edge"]
    a, b = (G.T.Shape * 1)(cs.A[0]), (G.T.Shape * 1)(cs.B[0])
    pool = np.ascontiguousarray(cs.pool)
    assert G.host_lib().grh_no_record(a, b, G.T.dptr(pool)) == np.inf
