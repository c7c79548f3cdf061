"""Planar proximity records on the GPU: rkh_min_distance_records_2d and rkh_collision_records_2d against the reference
side (tests/cpp/prox_record_ref_2d.cpp over the oracle's planar closed forms), and the C++ planar proximity socket.

Tolerances are the project's own (tests/prox_records.py): distances 1e-12, points 1e-10 max(1, |p|inf).  The device's
record is held against the record of the finder it named; that finder must be the min_i of the reference's replayed loop
wherever every decision of the replay had 1e-9 of margin (at most 20 % of the states may fall outside: the CPU test holds
that for these very states).  Points are compared where the reference defines them (prox_records_2d.MIN_SEPARATION)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import prox_records_2d as PR2
from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 8


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


def _assert_worst(worst):
    assert worst["d"] <= PR2.DIST_TOL and worst["p1"] <= PR2.POINT_TOL and worst["p2"] <= PR2.POINT_TOL, worst


# ------------------------------------------------------------------------------- (a) minimum records, scene by scene
_SCENES = {label: (make, seed) for label, make, seed in PR2.gpu_scenes()}


@pytest.mark.parametrize("B", PR2.GPU_BATCHES)
@pytest.mark.parametrize("label", sorted(_SCENES))
def test_min_distance_records_2d_against_the_reference_side(L, ctx, label, B):
    """The planar C1 arm, the mixed arms of 2, 4 and 7 joints, the CRS A465 analog (prismatic root) and a mixed revolute /
    prismatic chain of 7 joints, at B = 1, 65 and 1000: dist bit-equal to rkh_min_distance, every (shape1, shape2) a finder
    of the scene, points and distance of the named finder's record, the finder the replayed min_i wherever it is clear."""
    make, seed = _SCENES[label]
    scn = make()
    x = PR2.random_states(scn, B, seed)
    sc = L.Scene(ctx, scn)
    PR2.check_min_records_2d(sc, PR2.RefRecords2D(scn), PR2.restated_frames(scn, x), x, f"{label} B={B}")
    sc.close()


# ------------------------------------------------------------------------------- (b) the order decides
def _one_joint(shapes, link=0.2):
    ops = [T.KteOp(kind=T.KTE_REVOLUTE_JOINT_2D, coord=0, base_frame=0, end_frame=1, joint_op=-1),
           T.KteOp(kind=T.KTE_RIGID_LINK_2D, coord=-1, base_frame=1, end_frame=2, joint_op=-1)]
    ops[1].offset = T.make_pose_2d((link, 0.0))
    base = T.ChainBase()
    base.pose = T.make_pose_2d()
    return scenarios.Scenario(name="one_joint", ops=ops, base=base, shapes=list(shapes), dyn=T.DynSpace(), n_dof=1, n_frames=3,
                              start=np.zeros(1), goal=np.zeros(1), meta={"lower": np.array([-np.pi]), "upper": np.array([np.pi])})


def _shape(kind, pos, dims, angle=0.0, anchor=-1):
    s = T.Shape(kind=kind, anchor=anchor)
    s.pose = T.make_pose_2d(pos, angle)
    s.dims[:] = [float(dims[0]), float(dims[1]) if len(dims) > 1 else 0.0, 0.0]
    return s


def test_the_finder_order_decides_the_record(L, ctx):
    """The three shapes of test_planar_cull_order_is_the_references: a wide capped rectangle whose caps reach beyond its
    bounding radius, a circle 0.01 off one cap and a circle 0.05 inside the other.  With [link, far, near] the cull
    against the running minimum skips the penetrating pair and the record names `far` at 0.01; with [link, near, far] it
    names `near` at -0.05.  A kernel that reports the lowest distance fails the first."""
    link = _shape(T.SHAPE_CRECT, (0.1, 0.0), (0.2, 6.0), anchor=1)
    far, near = _shape(T.SHAPE_CIRCLE, (0.1, 3.11), (0.1,)), _shape(T.SHAPE_CIRCLE, (3.2, 0.0), (0.05,))
    x = np.zeros((1, 2))
    for shapes, expect, who in (([link, far, near], 0.01, 1), ([link, near, far], -0.05, 1)):
        scn = _one_joint(shapes)
        sc = L.Scene(ctx, scn)
        R = PR2.check_min_records_2d(sc, PR2.RefRecords2D(scn), PR2.restated_frames(scn, x), x, f"order, expect {expect}")
        rec = sc.min_distance_records_2d(x)
        sc.close()
        assert rec["dist"][0] == pytest.approx(expect, rel=1e-9)
        assert (int(rec["shape1"][0]), int(rec["shape2"][0])) == (who, 0)  # the circle is shape1, the link shape2
        assert R["winner"][0] == 0 and R["margin"][0] > 1e-3
    # (in the first order the lowest distance over all finders is the skipped pair's)
    assert R["dist"][0].min() == pytest.approx(-0.05, rel=1e-9)


# ------------------------------------------------------------------------------- (c) tile edges
@pytest.mark.parametrize("placement", ["last", "first", "descending"])
@pytest.mark.parametrize("n_env", [1, 63, 64, 65, 129])
def test_tile_edges(L, ctx, n_env, placement):
    """One joint, one robot circle, n_env environment circles around the lanes-per-tile count of 64.  `last`: the fillers
    recede, so each is culled by the first one's distance, and the last finder penetrates and wins.  `first`: finder 0
    is the nearest, with its bounding circles apart (it is computed regardless), and every later finder is culled.
    `descending`: every finder is nearer than the one before, so the minimum is taken over n_env - 1 times."""
    robot = _shape(T.SHAPE_CIRCLE, (0.3, 0.0), (0.1,), anchor=1)
    ring = lambda k, radius: (0.3 + radius * np.cos(0.37 * k), radius * np.sin(0.37 * k))
    env = []
    for k in range(n_env):
        if placement == "last":
            env.append(_shape(T.SHAPE_CIRCLE, ring(k, 4.0 + 0.01 * k), (0.05,)) if k < n_env - 1
                       else _shape(T.SHAPE_CIRCLE, (0.3, 0.13), (0.05,)))
        elif placement == "first":
            env.append(_shape(T.SHAPE_CIRCLE, ring(k, 4.0 + 0.01 * k), (0.05,)) if k > 0
                       else _shape(T.SHAPE_CIRCLE, (0.3, 0.5), (0.05,)))
        else:
            env.append(_shape(T.SHAPE_CIRCLE, ring(k, 4.0 - 0.01 * k), (0.05,)))
    scn = _one_joint([robot] + env)
    x = np.zeros((3, 2))
    x[:, 0] = [0.0, 0.4, -1.1]
    ref = PR2.RefRecords2D(scn)
    frames = PR2.restated_frames(scn, x)
    sc = L.Scene(ctx, scn)
    R = PR2.check_min_records_2d(sc, ref, frames, x, f"tile n_env={n_env} {placement}")
    rec = sc.min_distance_records_2d(x[:1])
    col = sc.collision_records_2d(x, CAP)
    sc.close()
    want = 0 if placement == "first" else n_env - 1
    assert R["winner"][0] == want and int(rec["shape1"][0]) == 0 and int(rec["shape2"][0]) == 1 + want
    if placement == "first":
        assert R["gap"][0, 0] > 0.1 and rec["dist"][0] == pytest.approx(0.35, rel=1e-9)
    if placement == "last":
        assert rec["dist"][0] == pytest.approx(-0.02, rel=1e-9) and int(col["n_found"][0]) == 1
    n_coll, _, worst, _, _ = PR2.check_collision_rows_2d(col, R, range(len(x)), CAP)
    _assert_worst(worst)
    assert (n_coll > 0) == (placement == "last")  # (only `last` places a circle within the robot's reach)


# ------------------------------------------------------------------------------- (d) every routine, both roles
def _pair_cases():
    cases = []
    for routine, (k1, k2) in sorted(PR2.ROUTINE_KINDS.items()):
        cases.append((routine, True))  # the robot's shape is shape1
        if k1 != k2:
            cases.append((routine, False))  # the environment's shape is shape1
    return cases


_PAIR_DIMS = {T.SHAPE_CIRCLE: (0.09,), T.SHAPE_CRECT: (0.3, 0.1), T.SHAPE_RECTANGLE: (0.3, 0.16)}


@pytest.mark.parametrize("routine,robot_first", _pair_cases())
def test_every_routine_one_pair_at_a_time(L, ctx, routine, robot_first):
    """A one-joint chain that carries one shape past one obstacle, 256 joint angles: every routine with the robot's shape
    as the finder's shape1 and (kinds differing) as its shape2.  One finder: its record, its ids in the finder's order."""
    k1, k2 = PR2.ROUTINE_KINDS[routine]
    k_robot, k_env = (k1, k2) if robot_first else (k2, k1)
    robot = _shape(k_robot, (0.25, 0.02), _PAIR_DIMS[k_robot], angle=0.15, anchor=1)
    env = _shape(k_env, (0.28, 0.21), _PAIR_DIMS[k_env], angle=-0.4)
    scn = _one_joint([env, robot])  # the obstacle first: the ids are the caller's indices, not robot-then-environment
    x = PR2.random_states(scn, 256, 300 + routine)
    sc = L.Scene(ctx, scn)
    R = PR2.check_min_records_2d(sc, PR2.RefRecords2D(scn), PR2.restated_frames(scn, x), x, f"routine {routine} robot_first={robot_first}")
    rec = sc.min_distance_records_2d(x)
    col = sc.collision_records_2d(x, 2)
    sc.close()
    assert list(R["routine"]) == [routine]
    assert np.all(rec["shape1"] == (1 if robot_first else 0)) and np.all(rec["shape2"] == (0 if robot_first else 1))
    n_coll, _, worst, _, _ = PR2.check_collision_rows_2d(col, R, range(len(x)), 2)
    _assert_worst(worst)
    if routine != 16:  # (rectangle / rectangle has no sign)
        assert 10 <= n_coll <= 246 and 10 <= int(np.sum(R["dist"][:, 0] < 0.0)) <= 246


# ------------------------------------------------------------------------------- (e) collision records
def test_collision_records_2d_match_gather_collision_points(L, ctx):
    """cap = 8 on 1000 states of the mixed 4-joint arm among 60 obstacles: n_found and the records in finder order are
    the reference's list -- finders whose bounding circles are not apart (> 0.0 skips) with d < 0.0 -- except finders
    within 1e-12 of either threshold."""
    scn = scenarios.make_planar_mixed(n=4, n_obstacles=60)
    x = PR2.random_states(scn, 1000, 21)
    R = PR2.RefRecords2D(scn).records(PR2.restated_frames(scn, x))
    sc = L.Scene(ctx, scn)
    rec = sc.collision_records_2d(x, CAP)
    sc.close()
    assert rec["point1"].shape == (1000, CAP, 2)
    n_coll, n_edge, worst, n_rec, n_undef = PR2.check_collision_rows_2d(rec, R, range(len(x)), CAP)
    print(f"mixed4/60: {n_coll} states with a collision, max n_found {int(rec['n_found'].max())}, {n_edge} states at the "
          f"verdict bar, {n_rec} records ({n_undef} with undefined points), dist err {worst['d']:.3e} point1 err "
          f"{worst['p1']:.3e} point2 err {worst['p2']:.3e}")
    assert n_coll >= 50 and int(rec["n_found"].max()) >= 2
    assert n_undef <= PR2.MAX_UNDEFINED * n_rec
    _assert_worst(worst)


def _crowded(n_env_extra, per_link=1):
    """The mixed 7-joint arm with circles strung along its links at one configuration (they collide there)."""
    scn = scenarios.make_planar_mixed(n=7, n_obstacles=24)
    x = np.zeros((1, 14))
    x[0, 0::2] = [0.4, 0.9, -1.3, 0.6, 1.1, -0.7, 0.5]
    fr = PR2.restated_frames(scn, x)[0]
    rng = np.random.default_rng(31)
    for k in range(n_env_extra):
        c = fr[1 + 2 * (1 + k % 6), :2] + rng.uniform(-0.05, 0.05, size=2)  # around the moving joints: each touches two links' shapes
        scn.shapes.append(_shape(T.SHAPE_CIRCLE, c, (0.11,)))
    return scn, x


def test_collision_records_2d_beyond_the_capacity(L, ctx):
    """More finders collide than cap = 8 holds: n_found is the true count, the first 8 records are the list's first 8 and
    the slots behind read +inf / 0xFFFFFFFF / 0; with cap = n_found the whole list comes back; cap = 0 still counts."""
    scn, x = _crowded(14)
    R = PR2.RefRecords2D(scn).records(PR2.restated_frames(scn, x))
    sure, maybe = PR2.PR.reference_collisions(R, 0)
    assert len(sure) > CAP and len(maybe) == 0, (len(sure), len(maybe))
    sc = L.Scene(ctx, scn)
    rec = sc.collision_records_2d(x, CAP)
    full = sc.collision_records_2d(x, len(sure) + 3)
    none = sc.collision_records_2d(x, 0)
    sc.close()
    assert int(rec["n_found"][0]) == len(sure) == int(full["n_found"][0]) == int(none["n_found"][0])
    assert none["dist"].shape == (1, 0)
    _, _, worst, _, _ = PR2.check_collision_rows_2d(rec, R, [0], CAP)
    _, _, worst2, n_rec, _ = PR2.check_collision_rows_2d(full, R, [0], len(sure) + 3)
    print(f"{len(sure)} collisions at cap {CAP}: errors {worst} / full list {worst2}")
    assert n_rec == len(sure)
    _assert_worst(worst)
    _assert_worst(worst2)


def test_collision_records_2d_on_more_than_4096_pairs(L, ctx):
    """21 robot shapes (three per link of the 7-joint arm) against 200 obstacles: 4200 finders, 66 tiles of 64.  Both
    queries against the reference side on 6 states (only the _2d entries are called on this scene)."""
    scn = scenarios.make_planar_mixed(n=7, n_obstacles=200)
    robot = [s for s in scn.shapes if s.anchor >= 0]
    for s in robot:
        for off, r in ((0.08, 0.045), (0.2, 0.035)):
            scn.shapes.append(_shape(T.SHAPE_CIRCLE, (off, 0.01), (r,), anchor=s.anchor))
    ref = PR2.RefRecords2D(scn)
    assert ref.nf == 21 * 200 > 4096
    x = PR2.random_states(scn, 6, 41)
    R = ref.records(PR2.restated_frames(scn, x))
    sc = L.Scene(ctx, scn)
    assert sc.num_pairs == 4200
    col = sc.collision_records_2d(x, 64)
    rec = sc.min_distance_records_2d(x)
    sc.close()
    n_coll, n_edge, worst, n_rec, n_undef = PR2.check_collision_rows_2d(col, R, range(len(x)), 64)
    print(f"4200 pairs: n_found {col['n_found'].tolist()}, {n_rec} records ({n_undef} undefined), errors {worst}")
    assert n_coll >= 3 and n_rec >= 20 and int(col["n_found"].max()) <= 64
    _assert_worst(worst)
    finder_of = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(R["s1"], R["s2"]))}
    for b in range(len(x)):
        fi = finder_of[(int(rec["shape1"][b]), int(rec["shape2"][b]))]
        assert abs(rec["dist"][b] - R["dist"][b, fi]) <= PR2.DIST_TOL
        if R["margin"][b] >= PR2.CLEAR_MARGIN:
            assert fi == R["winner"][b]
        if R["sep"][b, fi] >= PR2.MIN_SEPARATION:
            assert PR2.point_error(rec["point1"][b], R["p1"][b, fi]) <= PR2.POINT_TOL
            assert PR2.point_error(rec["point2"][b], R["p2"][b, fi]) <= PR2.POINT_TOL
    assert np.sum(R["margin"] >= PR2.CLEAR_MARGIN) >= 5


# ------------------------------------------------------------------------------- (f) refusals and edges
def test_refusals_and_edge_cases_2d(L, ctx):
    lib = L.load()
    dz, uz = (C.c_double * 64)(), (C.c_uint32 * 64)()
    # a 3D scene: its records come from the 3D entries, and the text says so
    sc = L.Scene(ctx, scenarios.make_c2())
    x = np.zeros((1, sc.D))
    for call in (lambda: sc.min_distance_records_2d(x), lambda: sc.collision_records_2d(x, 4)):
        with pytest.raises(L.RkhError) as e:
            call()
        assert e.value.status == -5 and "not supported" in str(e.value) and "rkh_min_distance_records" in str(e.value)
    sc.close()
    # a planar scene without environment shapes: no finders
    c1 = scenarios.make_c1_planar()
    c1.shapes = [s for s in c1.shapes if s.anchor >= 0]
    sc = L.Scene(ctx, c1)
    assert sc.num_pairs == 0
    x = np.full((5, sc.D), 0.25)
    rec = sc.min_distance_records_2d(x)
    assert np.all(np.isposinf(rec["dist"])) and np.all(rec["shape1"] == PR2.NO_SHAPE) and np.all(rec["shape2"] == PR2.NO_SHAPE)
    assert not rec["point1"].any() and not rec["point2"].any()
    col = sc.collision_records_2d(x, 3)
    assert not col["n_found"].any() and np.all(col["shape1"] == PR2.NO_SHAPE) and np.all(np.isposinf(col["dist"]))
    assert not col["point1"].any() and not col["point2"].any()
    # NULL pointers and B = 0
    xs = np.zeros(sc.D)
    args = [sc.h, T.dptr(xs), 1, dz, dz, dz, uz, uz]
    for i in (0, 1, 3, 4, 5, 6, 7):
        bad = list(args)
        bad[i] = None
        assert lib.rkh_min_distance_records_2d(*bad) == -1, i
    assert lib.rkh_min_distance_records_2d(sc.h, T.dptr(xs), 0, dz, dz, dz, uz, uz) == 0
    args = [sc.h, T.dptr(xs), 1, 2, uz, dz, dz, dz, uz, uz]
    for i in (0, 1, 4, 5, 6, 7, 8, 9):
        bad = list(args)
        bad[i] = None
        assert lib.rkh_collision_records_2d(*bad) == -1, i
    assert lib.rkh_collision_records_2d(sc.h, T.dptr(xs), 0, 2, uz, dz, dz, dz, uz, uz) == 0
    sc.close()


# ------------------------------------------------------------------------------- (g) the adaptor
def test_the_cpp_planar_proximity_socket_returns_the_records(L, ctx, tmp_path):
    """tests/cpp/prox_records_2d_smoke.cpp (g++ against librkh.so, built like prox_records_smoke.cpp):
    findMinimumDistance() and gatherCollisionPoints of hip_proxy_query_pair_2D on states of the crowded 7-joint arm -- 16
    colliding and 8 free ones -- are the C-ABI's own answers bit for bit, gatherCollisionPoints growing its capacity."""
    scn, x0 = _crowded(14)
    x = np.concatenate([x0, PR2.random_states(scn, 255, 51)])
    sc = L.Scene(ctx, scn)
    d = sc.min_distance(x)
    pick = np.concatenate([[0], np.flatnonzero(d < -1e-6)[1:16], np.flatnonzero(d > 1e-3)[:8]])
    xs = np.ascontiguousarray(x[pick])
    src, exe = os.path.join(ROOT, "tests", "cpp", "prox_records_2d_smoke.cpp"), os.path.join(ROOT, "tests", "cpp", "prox_records_2d_smoke")
    newer = [src, os.path.join(ROOT, "include", "rkh_adaptors.hpp"), os.path.join(ROOT, "include", "rkh.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(f) for f in newer)):
        lib_dir = os.path.join(ROOT, "reak_amd")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                        "-L", lib_dir, "-lrkh", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    blob = tmp_path / "scene.bin"
    with open(blob, "wb") as f:
        f.write(np.int32(len(scn.ops)).tobytes())
        f.write(bytes(scn.ops_array()))
        f.write(bytes(scn.base))
        f.write(np.int32(len(scn.shapes)).tobytes())
        f.write(bytes(scn.shapes_array()))
        f.write(np.int32(len(xs)).tobytes())
        f.write(xs.tobytes())
    run = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = json.loads(run.stdout.strip().splitlines()[-1])["states"]
    rec = sc.min_distance_records_2d(xs)
    col = sc.collision_records_2d(xs, 64)
    sc.close()
    assert len(out) == len(xs) == 24 and CAP < int(col["n_found"].max()) <= 64
    n_hits = 0
    for b, o in enumerate(out):
        assert o["dist"] == rec["dist"][b] and o["p1"] == rec["point1"][b].tolist() and o["p2"] == rec["point2"][b].tolist()
        assert (o["s1"], o["s2"]) == (int(rec["shape1"][b]), int(rec["shape2"][b]))
        n = int(col["n_found"][b])
        assert len(o["hits"]) == n
        for i, h in enumerate(o["hits"]):
            assert h["dist"] == col["dist"][b, i] and h["p1"] == col["point1"][b, i].tolist()
            assert h["p2"] == col["point2"][b, i].tolist()
            assert (h["s1"], h["s2"]) == (int(col["shape1"][b, i]), int(col["shape2"][b, i]))
        n_hits += n
    assert n_hits >= 16
