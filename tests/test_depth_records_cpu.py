"""The depth records of support-map pairs -- gjk_depth_record / gjk_depth_distance of reak_amd/csrc/epa_device.h through
pair_record_depth / pair_distance_depth of proximity_record_device.h, compiled for the host (tests/cpp/epa_record_host.cpp)
-- on the case families of tests/penetration_ref.py, held against its certificate: 1e-12 throughout, measured against the
separating-axis depth and the exact polytope distance, never against the code under test.  No GPU.

Families: shallow (polytope_ref.penetrating_cases: 300), deep (60 mesh pairs moved 1e-6 .. 0.2 into each other), partners
(60: mesh against sphere / capped cylinder / box with crossing cores, both orders), hand (20 hand-built dyadic pairs, half
of them at an offset of 2^20), continuity (a capped cylinder 1e-6 clear of a mesh and 1e-6 into it), and edge
(polytope_ref.edge_cases: 118 pairs, 100 of them apart) for the exits with the cores apart.

Worst figures of the host build over all of them, as first measured: unit 2.2e-16, depth 1.0e-16, width 1.7e-16, point1 /
point2 off their cores 4.2e-16 / 2.5e-16, |qa - qb - depth n| 5.6e-17; apart: normal 2.2e-16.  The largest polytope has 27
vertices (deep) of the 64 the cap allows."""
import subprocess

import numpy as np
import pytest

import gjk_records as G
import penetration_ref as R
import polytope_ref as P
from reak_amd import types as T

FAMILIES = ["shallow", "deep", "partners", "hand", "continuity", "edge"]


@pytest.fixture(scope="module")
def families():
    f = dict(R.families())
    f["edge"] = P.edge_cases()
    return f


@pytest.fixture(scope="module")
def records(families):
    return {k: R.host_records(cs.A, cs.B, cs.pool) for k, cs in families.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _report(w):
    return "%d of %d miss the certificate:\n" % (len(w.bad), w.n) + "\n".join(map(str, w.bad[:10]))


def test_the_families_are_what_the_figures_were_taken_on(families):
    assert [len(families[k]) for k in FAMILIES] == [300, 60, 60, 20, 2, 118]
    cross = {k: int(np.sum(R.crossing(families[k]))) for k in FAMILIES}
    print("crossing cases:", cross)
    assert cross["shallow"] == 300 and cross["partners"] == 60 and cross["hand"] == 20 and cross["continuity"] == 1
    assert 30 <= cross["deep"] < 60           # at least half cross, and the apart branch is in
    assert cross["edge"] == 18


def test_the_reference_on_cases_with_known_depths(families):
    """The hand-built depths, and the 18 colliding edge cases: exactly 0, 0.375 and 1 (touching pairs; the sphere's centre
    0.375 inside the cube's face; the point 0.375 inside; identical unit cubes)."""
    cs = families["hand"]
    for exact, ref, label in zip(cs.exact, R.family_references(cs), cs.label):
        assert not ref[4][0], label
        if exact is not None:
            assert ref[5] == exact, (label, ref[5], exact)
    cs = families["edge"]
    depths = sorted(set(r[5] for r in R.family_references(cs) if not r[4][0]))
    assert depths == [0.0, 0.375, 1.0], depths
    shallow = [r[5] for r in R.family_references(families["shallow"])]
    print("shallow depths: %.3g .. %.3g" % (min(shallow), max(shallow)))
    assert 1e-9 < min(shallow) and max(shallow) < 2e-3


@pytest.mark.parametrize("family", FAMILIES)
def test_host_records_hold_the_certificate(families, records, family):
    """Every case: the certificate; gjk_depth_distance bit-equal to the record's dist; where the cores are apart dist and
    the points are gjk_record's (the host build of tests/gjk_records.py) bit for bit."""
    cs, rec = families[family], records[family]
    w = R.certify_family(cs, rec, family)
    cap = R.host_lib().erh_max_verts_cap()
    print("%s: largest polytope %d vertices of %d" % (family, int(rec["verts"].max()), cap))
    assert not w.bad, _report(w)
    assert int(rec["verts"].max()) * 2 <= cap    # the margin the header claims
    assert np.array_equal(_bits(rec["dist"]), _bits(rec["depth_dist"]))
    apart = ~R.crossing(cs)
    assert w.n_apart == int(np.sum(apart))
    old = G.host_records(cs.A, cs.B, cs.pool)
    for k in ("dist", "point1", "point2"):
        assert np.array_equal(_bits(old[k][apart]), _bits(rec[k][apart])), k
    # crossing: the collision mark is kept, and the distance never lies above the sentinel of the plain query
    assert np.all(rec["dist"][~apart] <= old["dist"][~apart]) and np.all(rec["dist"][~apart] < 0.0)
    assert np.array_equal(old["dist"] < 0.0, rec["dist"] < 0.0)


@pytest.mark.parametrize("family", ["deep", "partners", "hand"])
def test_swapping_the_arguments_turns_the_normal(families, records, family):
    """gjk_depth_record(B, A): the certificate holds that way round, and the depth is the same to 1e-12."""
    cs, rec = families[family], records[family]
    back = R.host_records(cs.B, cs.A, cs.pool)
    w = R.certify_family(cs, back, family + " swapped", swap=True)
    e_d = float(np.max(np.abs(back["dist"] - rec["dist"])))
    print("%s: |dist(B, A) - dist(A, B)| max %.3g" % (family, e_d))
    assert not w.bad, _report(w)
    assert e_d <= R.TOL


def test_hand_built_cases_in_detail(families, records):
    cs, rec = families["hand"], records["hand"]
    by = {lab: i for i, lab in enumerate(cs.label)}
    for tag in ("", " at offset 2^20"):
        i = by["cube in cube, offset along x" + tag]      # the unique facet
        assert rec["dist"][i] == -0.625 - 1e-9 and rec["normal"][i].tolist() == [1.0, 0.0, 0.0]
        i = by["cube in cube, centred" + tag]             # six facets tie: any axis, either sign
        assert rec["dist"][i] == -0.75 - 1e-9 and sorted(np.abs(rec["normal"][i]).tolist()) == [0.0, 0.0, 1.0]
        for lab in ("touching face / face", "touching edge / edge", "touching corner / corner", "overlapping coplanar squares"):
            assert rec["dist"][by[lab + tag]] == -1e-9, lab      # depth 0: the sentinel itself
        i = by["overlapping coplanar squares" + tag]      # flat: the plane's normal, one common point
        assert np.abs(rec["normal"][i]).tolist() == [0.0, 0.0, 1.0]
        assert np.array_equal(rec["point1"][i], rec["point2"][i]) and rec["verts"][i] == 3


def test_continuity_across_touching(families, records):
    """1e-6 apart and 1e-6 deep along the same facet normal: the two distances differ by 2e-6 + 1e-9, and the normals agree."""
    rec = records["continuity"]
    step = rec["dist"][0] - rec["dist"][1]
    print("continuity: dist %.17g -> %.17g, step - (2e-6 + 1e-9) = %.3g, |n - n| %.3g"
          % (rec["dist"][0], rec["dist"][1], step - (2e-6 + 1e-9), np.max(np.abs(rec["normal"][0] - rec["normal"][1]))))
    assert abs(step - (2e-6 + 1e-9)) <= R.TOL
    assert np.max(np.abs(rec["normal"][0] - rec["normal"][1])) <= R.TOL


def test_closed_form_pairs_keep_their_records_and_gain_a_normal():
    """pair_record_depth of a closed-form routine: dist and the points are pair_record's bit for bit, the normal is
    (point2 - point1) / dist componentwise; zeros where dist is 0."""
    rng = np.random.default_rng(7)
    a, b = [], []
    for _ in range(50):
        ka, kb = rng.choice([T.SHAPE_SPHERE, T.SHAPE_CCYLINDER, T.SHAPE_BOX], 2)
        if ka == T.SHAPE_BOX and kb == T.SHAPE_BOX:
            kb = T.SHAPE_SPHERE
        dims = lambda k: (rng.uniform(0.1, 0.4), rng.uniform(0.05, 0.2), rng.uniform(0.1, 0.3))
        a.append(P.make_shape(int(ka), rng.uniform(-0.4, 0.4, 3), dims(ka), P._rand_quat(rng)))
        b.append(P.make_shape(int(kb), rng.uniform(-0.4, 0.4, 3), dims(kb), P._rand_quat(rng)))
    # two spheres that touch exactly: dist == 0
    a.append(P.make_shape(T.SHAPE_SPHERE, (0, 0, 0), (0.25, 0, 0)))
    b.append(P.make_shape(T.SHAPE_SPHERE, (0.5, 0, 0), (0.25, 0, 0)))
    r = R.host_routine_records(a, b, np.zeros((1, 3)))
    for k in ("dist", "point1", "point2"):
        assert np.array_equal(_bits(r[k]), _bits(r["plain_" + k])), k
    assert np.any(r["dist"] < 0.0) and np.any(r["dist"] > 0.0) and r["dist"][-1] == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        expect = (r["point2"] - r["point1"]) / r["dist"][:, None]
    expect[r["dist"] == 0.0] = 0.0
    assert np.array_equal(_bits(r["normal"]), _bits(expect))


def test_the_host_build_under_the_sanitizers(families, tmp_path):
    """The same source as a program of its own (its own main), built with -fsanitize=address,undefined, once over the
    shallow and the hand-built families: every array index of the expansion, checked."""
    exe = R.host_program()
    for name in ("shallow", "hand"):
        cs = families[name]
        path = tmp_path / (name + ".bin")
        R.write_pairs(path, cs.A, cs.B, cs.pool)
        run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
        print(name, run.stdout.strip())
        assert run.returncode == 0, run.stdout + run.stderr
        assert run.stdout.startswith("%d pairs" % len(cs)) and "runtime error" not in run.stderr
