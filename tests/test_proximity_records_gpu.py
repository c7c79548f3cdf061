"""Proximity records on the GPU: rkh_min_distance_records and rkh_collision_records against the reference side
(tests/cpp/prox_record_ref.cpp over the oracle's closed forms), and the C++ proximity socket over them.

Tolerances: distances 1e-12 against the oracle, points 1e-10 max(1, |p|inf).  The winner's pair is
not stable where two finders tie -- adjacent link capsules share a cap at the joint, and 12-13 % of random C2 states
have two finders within 1e-12 of the minimum -- so: the device's points are held against the record of the finder the
device named, that finder's oracle distance must be the oracle's minimum to 1e-12, and the named pair must be the
oracle's winner wherever the oracle's runner-up is more than 1e-9 behind; at most 20 % of the states may fall outside
that last comparison."""
import copy
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import prox_records as PR
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


def _c2_scene(which):
    return scenarios.make_c2() if which == "c2" else scenarios.make_c2(floor=-0.45, n_cylinders=6, tool_sphere=0.06)


@pytest.fixture(scope="module")
def c2_cases(oracle):
    """(a)'s two scenes with 2048 random states each, their frames and the reference side, computed once."""
    out = {}
    for which in ("c2", "c2_full"):
        scn = _c2_scene(which)
        x = PR.random_states(scn, 2048, 5)
        out[which] = (scn, x, oracle.OracleScene(scn).fk(x), PR.RefRecords(scn))
    return out


# ------------------------------------------------------------------------------------------ (a) C2 and the full C2
def test_min_distance_records_on_c2_and_the_full_c2(L, ctx, c2_cases):
    """2048 random states each of C2 and of C2 with a floor plane, six cylinders and a spherical tool: dist bit-equal to
    rkh_min_distance, points and pair ids by the module's rules; both signs occur; together the winners cover the
    routines 1, 2, 3, 4, 5, 7, 8 and 11."""
    seen = set()
    for which in ("c2", "c2_full"):
        scn, x, frames, ref = c2_cases[which]
        sc = L.Scene(ctx, scn)
        routines, R = PR.check_min_records(sc, ref, frames, x, which)
        sc.close()
        seen |= set(int(r) for r in routines)
        n_hit = int(np.sum(R["dist"].min(axis=1) < 0.0))
        assert 0.02 * len(x) <= n_hit <= 0.15 * len(x), n_hit
    print("winning routines:", sorted(seen))
    assert seen >= {1, 2, 3, 4, 5, 7, 8, 11}


# ------------------------------------------------------------------------------------------ (b) one pair at a time
def _pair_cases():
    cases = []
    for routine, (k1, k2) in sorted(PR.ROUTINE_KINDS.items()):
        cases.append((routine, True))  # the robot's shape is shape1
        if k1 != k2:
            cases.append((routine, False))  # the environment's shape is shape1
    return cases


@pytest.mark.parametrize("routine,robot_first", _pair_cases())
def test_every_routine_one_pair_at_a_time(L, ctx, oracle, routine, robot_first):
    """A one-joint chain (make_pendulum) carrying one shape against one environment shape, for every routine and, where
    the cascade of kinds allows, both roles: 8 random placements x 32 joint angles = 256 poses, and one axis-aligned
    placement at the angle 0 (parallel and perpendicular axes; sin and cos of 0 are exact on both sides).  Axis-aligned
    placements at other angles are left to the CPU test of the closed forms: a capped cylinder that stays parallel to a
    box face has a whole stretch of closest points, and which of them the golden-section search ends on turns on the
    last bit of the joint's sine.  n_pairs = 1.  Planes are 8 m x 8 m, as the scene-creation rule wants them."""
    rng = np.random.default_rng(1000 + 10 * routine + int(robot_first))
    k1, k2 = PR.ROUTINE_KINDS[routine]
    k_robot, k_env = (k1, k2) if robot_first else (k2, k1)
    worst = {"p1": 0.0, "p2": 0.0, "d": 0.0}
    n_hit = 0
    for placement in range(9):
        scn = scenarios.make_pendulum()
        mode = 0 if placement == 8 else 2
        rs = T.Shape(kind=k_robot, anchor=1)
        rs.pose = T.make_pose(rng.uniform(-0.3, 0.3, size=3), PR._quat(rng, mode))
        rs.dims[:] = [float(v) for v in PR.random_dims(rng, k_robot, big_plane=True)]
        es = T.Shape(kind=k_env, anchor=-1)
        es.pose = T.make_pose(rng.uniform(-0.4, 0.4, size=3), PR._quat(rng, mode))
        es.dims[:] = [float(v) for v in PR.random_dims(rng, k_env, big_plane=True)]
        scn.shapes = [rs, es]
        x = np.zeros((32, 2))
        x[:, 0] = rng.uniform(-np.pi, np.pi, size=32)
        if mode == 0:
            x = np.zeros((1, 2))
        sc = L.Scene(ctx, scn)
        assert sc.num_pairs == 1
        rec, d_plain = sc.min_distance_records(x), sc.min_distance(x)
        sc.close()
        R = PR.RefRecords(scn).records(oracle.OracleScene(scn).fk(x))
        assert R["routine"].tolist() == [routine]
        want = (0, 1) if robot_first else (1, 0)
        assert (int(R["s1"][0]), int(R["s2"][0])) == want
        assert np.all(rec["shape1"] == want[0]) and np.all(rec["shape2"] == want[1])
        assert np.array_equal(rec["dist"].view(np.uint64), d_plain.view(np.uint64))
        worst["d"] = max(worst["d"], float(np.max(np.abs(rec["dist"] - R["dist"][:, 0]))))
        worst["p1"] = max(worst["p1"], PR.point_error(rec["point1"], R["p1"][:, 0]))
        worst["p2"] = max(worst["p2"], PR.point_error(rec["point2"], R["p2"][:, 0]))
        n_hit += int(np.sum(R["dist"][:, 0] < 0.0))
    print(f"routine {routine} robot_first={robot_first}: dist err {worst['d']:.3e} point1 err {worst['p1']:.3e} "
          f"point2 err {worst['p2']:.3e} penetrating {n_hit}/257")
    assert worst["d"] <= PR.DIST_TOL and worst["p1"] <= PR.POINT_TOL and worst["p2"] <= PR.POINT_TOL


# ------------------------------------------------------------------------------------------ (c) exact ties
@pytest.mark.parametrize("where", ["after", "before"])
def test_lowest_finder_wins_an_exact_tie(L, ctx, c2_cases, where):
    """C2 with the obstacle that wins most often listed twice: the twins' distances are bit-equal by construction, and the
    reference keeps the earlier finder (a new minimum only on a strictly smaller distance).  The copy goes once behind
    all shapes and once in front of the environment shapes, so the lower index is once the original's and once the
    copy's."""
    scn, x, frames, ref = c2_cases["c2"]
    R = ref.records(frames[:512])
    env_of = np.where(R["s1"] >= 6, R["s1"], R["s2"])  # C2: shapes 0..5 are the robot's capsules
    top = int(np.bincount(env_of[R["winner"]]).argmax())
    twin = copy.deepcopy(scn)
    dup = T.Shape(kind=scn.shapes[top].kind, anchor=-1)
    dup.pose, dup.dims[:] = scn.shapes[top].pose, list(scn.shapes[top].dims)
    if where == "after":
        twin.shapes = list(scn.shapes) + [dup]
        low, high = top, len(scn.shapes)
    else:
        twin.shapes = list(scn.shapes[:6]) + [dup] + list(scn.shapes[6:])
        low, high = 6, top + 1
    sc = L.Scene(ctx, twin)
    rec = sc.min_distance_records(x[:512])
    sc.close()
    R2 = PR.RefRecords(twin).records(frames[:512])
    w1, w2 = R2["s1"][R2["winner"]], R2["s2"][R2["winner"]]
    tie = (w1 == low) | (w2 == low)  # the oracle's winner is the lower twin: an exact tie with the higher one
    assert int(np.sum(tie)) >= 20, int(np.sum(tie))
    got_env = np.where(rec["shape1"] >= 6, rec["shape1"], rec["shape2"])  # (the robot's capsules stay shapes 0..5)
    d_sorted = np.sort(R2["dist"], axis=1)
    clear = d_sorted[:, 2] - d_sorted[:, 0] > 1e-9  # nobody else near the twins
    n = int(np.sum(tie & clear))
    print(f"twin {where}: {int(np.sum(tie))} states won by the twins, {n} of them clear of third finders; "
          f"device named the higher twin in {int(np.sum(got_env[tie & clear] == high))}")
    assert n >= 20
    assert np.all(got_env[tie & clear] == low)
    assert np.array_equal(rec["shape1"][tie & clear], w1[tie & clear].astype(np.uint32))
    assert np.array_equal(rec["shape2"][tie & clear], w2[tie & clear].astype(np.uint32))


# ------------------------------------------------------------------------------------------ (d) (e) (f) other chains
def test_min_distance_records_with_a_prismatic_root(L, ctx):
    """make_crs_a465_track (7 joints, prismatic root), 512 states; the frames come from tests/kte_ref.py.  Served by the
    one record kernel of the revolute translation unit.  On these states the oracle alone puts two finders within 1e-12 of
    the minimum in 26.8 % of them (nothing between 1e-12 and 1e-9; 12-13 % on C2): the ceiling on the share left out
    of the pair comparison is this scene's own, 30 %."""
    scn = scenarios.make_crs_a465_track()
    x = PR.random_states(scn, 512, 6)
    sc = L.Scene(ctx, scn)
    PR.check_min_records(sc, PR.RefRecords(scn), PR.restated_frames(scn, x), x, "track", max_excluded=0.30)
    sc.close()


def test_min_distance_records_on_a_branching_chain_of_12_joints(L, ctx, oracle):
    """make_c4(meshes=False): 12 joints in two branches, 200 obstacles (2400 finders: several strides per lane), 256
    states.  Two arms tie at twice as many joints: the oracle alone puts two finders within 1e-12 of the minimum in
    22.3 % of these states (nothing between 1e-12 and 1e-9), so the ceiling on the share left out of the pair comparison
    is this scene's own, 25 %."""
    scn = scenarios.make_c4(meshes=False)
    x = PR.random_states(scn, 256, 7)
    sc = L.Scene(ctx, scn)
    PR.check_min_records(sc, PR.RefRecords(scn), oracle.OracleScene(scn).fk(x), x, "c4", max_excluded=0.25)
    sc.close()


def test_points_stay_inside_the_relative_bar_far_from_the_origin(L, ctx, oracle):
    """C2 moved by (1e5, 0.75e5, 1e4) m (the translated world of tests/test_steer_filters_gpu.py), 512 states.  Points:
    1e-10 max(1, |p|inf) as everywhere.  Distances are differences of coordinates of size 1e5, whose unit in the last
    place is 1.5e-11, yet the 1e-12 bar holds there too: device and oracle round every sum alike and differ by sin/cos
    roundings only."""
    import steer_filter_scenes as S

    scn = S.far_world(scenarios.make_c2(), 1e5)
    x = PR.random_states(scn, 512, 8)
    sc = L.Scene(ctx, scn)
    PR.check_min_records(sc, PR.RefRecords(scn), oracle.OracleScene(scn).fk(x), x, "c2 at 1e5 m")
    sc.close()


# ------------------------------------------------------------------------------------------ (g) collision records
def _check_collision_rows(rec, R, rows, cap):
    """Device rows against the reference's list (cull at 0, then d < 0, finder order).  Returns (states with a collision,
    states left to the verdict bar)."""
    finder_of = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(R["s1"], R["s2"]))}
    n_coll = n_edge = 0
    worst = {"d": 0.0, "p1": 0.0, "p2": 0.0}
    for b in rows:
        sure, maybe = PR.reference_collisions(R, b)
        n = int(rec["n_found"][b])
        k = min(n, cap)
        ids = [finder_of[(int(rec["shape1"][b, i]), int(rec["shape2"][b, i]))] for i in range(k)]
        assert ids == sorted(ids) and len(set(ids)) == len(ids), (b, ids)
        assert np.all(rec["shape1"][b, k:] == PR.NO_SHAPE) and np.all(np.isinf(rec["dist"][b, k:]))
        if len(maybe):  # a finder within 1e-12 of 0 (distance or cull): either verdict is right
            n_edge += 1
            assert set(ids) <= set(sure) | set(maybe) and len(sure) <= n <= len(sure) + len(maybe), (b, ids, sure, maybe)
        else:
            assert n == len(sure) and ids == list(sure[:cap]), (b, n, ids, sure)
        n_coll += 1 if len(sure) else 0
        for i, fi in enumerate(ids):
            worst["d"] = max(worst["d"], abs(rec["dist"][b, i] - R["dist"][b, fi]))
            worst["p1"] = max(worst["p1"], PR.point_error(rec["point1"][b, i], R["p1"][b, fi]))
            worst["p2"] = max(worst["p2"], PR.point_error(rec["point2"][b, i], R["p2"][b, fi]))
    return n_coll, n_edge, worst


@pytest.mark.parametrize("which", ["c2", "c2_full"])
def test_collision_records_match_gather_collision_points(L, ctx, c2_cases, which):
    """cap = 8 on (a)'s states: n_found and the records in finder order are the reference's list -- finders whose
    bounding spheres are not apart (> 0.0 skips) with d < 0.0 -- except finders within 1e-12 of either threshold."""
    scn, x, frames, ref = c2_cases[which]
    sc = L.Scene(ctx, scn)
    rec = sc.collision_records(x, CAP)
    sc.close()
    R = ref.records(frames)
    n_coll, n_edge, worst = _check_collision_rows(rec, R, range(len(x)), CAP)
    print(f"{which}: {n_coll} states with a collision, max n_found {int(rec['n_found'].max())}, {n_edge} states at the "
          f"verdict bar, dist err {worst['d']:.3e} point1 err {worst['p1']:.3e} point2 err {worst['p2']:.3e}")
    assert n_coll >= 50
    assert worst["d"] <= PR.DIST_TOL and worst["p1"] <= PR.POINT_TOL and worst["p2"] <= PR.POINT_TOL


def test_collision_records_beyond_the_capacity(L, ctx, oracle):
    """The arm folded into a cluster of overlapping obstacles: C2's world plus twelve spheres strung along the folded
    arm.  More finders collide than cap = 8 holds: n_found is the true count, the first 8 records are the list's first 8,
    and with cap = n_found the whole list comes back."""
    scn = scenarios.make_c2()
    x = np.zeros((1, scn.D))
    x[0, 0::2] = [0.4, 1.2, -2.2, 0.3, 1.5, 0.0]
    fr = oracle.OracleScene(scn).fk(x)[0]
    rng = np.random.default_rng(12)
    for k in range(12):
        s = T.Shape(kind=T.SHAPE_SPHERE, anchor=-1)
        c = fr[1 + 2 * (k % 6), :3] + rng.uniform(-0.06, 0.06, size=3)  # around the joints: each touches two capsules
        s.pose = T.make_pose(c)
        s.dims[:] = [0.12, 0.0, 0.0]
        scn.shapes.append(s)
    R = PR.RefRecords(scn).records(oracle.OracleScene(scn).fk(x))
    sure, maybe = PR.reference_collisions(R, 0)
    assert len(sure) > CAP and len(maybe) == 0, (len(sure), len(maybe))
    sc = L.Scene(ctx, scn)
    rec = sc.collision_records(x, CAP)
    assert int(rec["n_found"][0]) == len(sure)
    n_coll, _, worst = _check_collision_rows(rec, R, [0], CAP)
    full = sc.collision_records(x, len(sure))
    _, _, worst2 = _check_collision_rows(full, R, [0], len(sure))
    none = sc.collision_records(x, 0)
    sc.close()
    assert int(none["n_found"][0]) == len(sure)
    print(f"{len(sure)} collisions at cap {CAP}: errors {worst} / full list {worst2}")
    for w in (worst, worst2):
        assert w["d"] <= PR.DIST_TOL and w["p1"] <= PR.POINT_TOL and w["p2"] <= PR.POINT_TOL


# ------------------------------------------------------------------------------------------ (h) refusals and edges
def test_refusals_and_edge_cases(L, ctx):
    lib = L.load()
    dz, uz = (C.c_double * 64)(), (C.c_uint32 * 64)()
    # scenes whose records are not built: meshes (the support-map query yields no points), planar chains
    for scn in (scenarios.make_c4(n_obstacles=10, meshes=True), scenarios.make_c1_planar()):
        sc = L.Scene(ctx, scn)
        x = np.zeros((1, sc.D))
        for call in (lambda: sc.min_distance_records(x), lambda: sc.collision_records(x, 4)):
            with pytest.raises(L.RkhError) as e:
                call()
            assert e.value.status == -5 and "not supported" in str(e.value)
        assert np.isfinite(sc.min_distance(x)[0])  # the distance query still serves them
        sc.close()
    # an empty pair list
    sc = L.Scene(ctx, scenarios.make_hidim(3))
    assert sc.num_pairs == 0
    x = np.full((5, sc.D), 0.25)
    rec = sc.min_distance_records(x)
    assert np.all(np.isposinf(rec["dist"])) and np.all(rec["shape1"] == PR.NO_SHAPE) and np.all(rec["shape2"] == PR.NO_SHAPE)
    assert not rec["point1"].any() and not rec["point2"].any()
    col = sc.collision_records(x, 3)
    assert not col["n_found"].any() and np.all(col["shape1"] == PR.NO_SHAPE) and np.all(np.isposinf(col["dist"]))
    # NULL pointers and B = 0
    xs = np.zeros(sc.D)
    args = [sc.h, T.dptr(xs), 1, dz, dz, dz, uz, uz]
    for i in (0, 1, 3, 4, 5, 6, 7):
        bad = list(args)
        bad[i] = None
        assert lib.rkh_min_distance_records(*bad) == -1, i
    assert lib.rkh_min_distance_records(sc.h, T.dptr(xs), 0, dz, dz, dz, uz, uz) == 0
    args = [sc.h, T.dptr(xs), 1, 2, uz, dz, dz, dz, uz, uz]
    for i in (0, 1, 4, 5, 6, 7, 8, 9):
        bad = list(args)
        bad[i] = None
        assert lib.rkh_collision_records(*bad) == -1, i
    assert lib.rkh_collision_records(sc.h, T.dptr(xs), 0, 2, uz, dz, dz, dz, uz, uz) == 0
    sc.close()


# ------------------------------------------------------------------------------------------ (i) the adaptor
def test_the_cpp_proximity_socket_returns_the_records(L, ctx, tmp_path, c2_cases):
    """tests/cpp/prox_records_smoke.cpp (g++ against librkh.so, built like abi_smoke.cpp): findMinimumDistance() and
    gatherCollisionPoints of hip_proxy_query_pair on C2 states -- the first 24 colliding ones and 8 free ones of (a) --
    are the C-ABI's own answers bit for bit, gatherCollisionPoints growing its capacity where needed."""
    scn, x, frames, ref = c2_cases["c2"]
    d = ref.records(frames)["dist"].min(axis=1)
    pick = np.concatenate([np.flatnonzero(d < -1e-6)[:24], np.flatnonzero(d > 1e-3)[:8]])
    xs = np.ascontiguousarray(x[pick])
    src, exe = os.path.join(ROOT, "tests", "cpp", "prox_records_smoke.cpp"), os.path.join(ROOT, "tests", "cpp", "prox_records_smoke")
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
    sc = L.Scene(ctx, scn)
    rec = sc.min_distance_records(xs)
    col = sc.collision_records(xs, 64)
    sc.close()
    assert len(out) == len(xs) and int(col["n_found"].max()) <= 64
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
    assert n_hits >= 24
