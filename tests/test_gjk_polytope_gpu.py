"""The device's support-map query (reak_amd/csrc/gjk_device.h) against the exact polytope distance of
tests/polytope_ref.py -- a reference that is no GJK -- on the case families of tests/test_gjk_polytope_cpu.py, one launch
per family, and against the oracle's twin on the same cases.

Bounds: free pairs 1e-10 absolute against the reference (the project's bound for GJK against the closed forms; the
reference's own error at these sizes is about 1e-16), colliding pairs exactly -(rA + rB) - 1e-9, device against oracle
1e-12.  No case is excluded."""
import numpy as np
import pytest

import polytope_ref as P

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


@pytest.fixture(scope="module")
def families():
    return {"gap": P.gap_placed_cases(), "penetrating": P.penetrating_cases(), "edge": P.edge_cases(),
            "partner": P.partner_cases(), "capsule_box": P.capsule_box_cases()}


@pytest.mark.parametrize("family", ["gap", "penetrating", "edge", "partner", "capsule_box"])
def test_device_gjk_matches_the_exact_polytope_distance(L, ctx, oracle, families, family):
    """L.gjk_distance on every case of the family (the families: test_oracle_gjk_matches_the_exact_polytope_distance)."""
    cs = families[family]
    got = L.gjk_distance(ctx, cs.A, cs.B, cs.pool)
    twin = oracle.gjk_distance(cs.A, cs.B, cs.pool)
    free = cs.free()
    err = np.abs(got - np.array(cs.expect))
    print("%s: %d cases, %d free; worst free error against the reference %.3g, worst |device - oracle| %.3g"
          % (family, len(cs), free.sum(), err[free].max() if free.any() else 0.0, np.max(np.abs(got - twin))))
    bad = cs.check(got, TOL)
    assert not bad, "%d of %d wrong (index, case, reference, got):\n" % (len(bad), len(cs)) + "\n".join(map(str, bad[:20]))
    assert np.max(np.abs(got - twin)) <= 1e-12


def test_a_mesh_scene_sees_the_same_gaps(L, ctx, oracle):
    """Scene.min_distance (pair list, to_gjk, minimum over the pairs) for a capped cylinder on a one-link chain among
    mesh obstacles placed 1e-6 clear of it or 1e-6 into it, one per configuration, and one across its axis: the sign is
    the reference's, and so is the value, to 1e-10 (the cores of the -1e-6 pairs are apart, so those values are exact
    too; crossing cores give -radius - 1e-9)."""
    scn, x, expect = P.gap_scene()
    d = L.Scene(ctx, scn).min_distance(x)
    assert np.array_equal(d < 0.0, expect < 0.0), (d, expect)
    assert np.max(np.abs(d - expect)) <= TOL, (d, expect)
    assert np.max(np.abs(d - oracle.OracleScene(scn).min_distance(x))) <= 1e-12
