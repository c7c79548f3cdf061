"""Depth records on the GPU: gjk_depth_record pair by pair (rkh_diag_gjk_depth_records), the depth forms of the two record
kernels (rkh_min_distance_records_depth, rkh_collision_records_depth) and the C++ proximity socket with its depth switch.

A record is held against the CERTIFICATE of tests/penetration_ref.py -- 1e-12 throughout, measured against the
separating-axis depth and the exact polytope distance, never against the code under test -- and against the host build
of the same header (required: dist 1e-12, points 1e-10 max(1, |p|inf), normals 1e-12; expected: bit-equal)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import gjk_records as G
import penetration_ref as R
import polytope_ref as P
import prox_records as PR
from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("dist", "point1", "point2")


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _report(w):
    return "%d of %d miss the certificate:\n" % (len(w.bad), w.n) + "\n".join(map(str, w.bad[:10]))


# ------------------------------------------------------------------------------------------ 1. one pair at a time
@pytest.fixture(scope="module")
def families():
    return dict(R.families())


@pytest.mark.parametrize("family", ["shallow", "deep", "partners", "hand", "continuity"])
def test_device_records_hold_the_certificate(L, ctx, families, family):
    cs = families[family]
    rec = L.gjk_depth_records(ctx, cs.A, cs.B, cs.pool)
    host = R.host_records(cs.A, cs.B, cs.pool)
    w = R.certify_family(cs, rec, family)
    e_d = float(np.max(np.abs(rec["dist"] - host["dist"])))
    e1, e2 = G.point_error(rec["point1"], host["point1"]), G.point_error(rec["point2"], host["point2"])
    e_n = float(np.max(np.abs(rec["normal"] - host["normal"])))
    same = all(np.array_equal(_bits(rec[k]), _bits(host[k])) for k in KEYS + ("normal",))
    print("%s: against the host build's: bit-equal %s; dist %.3g point1 %.3g point2 %.3g normal %.3g"
          % (family, same, e_d, e1, e2, e_n))
    assert not w.bad, _report(w)
    assert e_d <= G.TOL and e1 <= G.POINT_TOL and e2 <= G.POINT_TOL and e_n <= 1e-12
    if family == "continuity":
        assert abs((rec["dist"][0] - rec["dist"][1]) - (2e-6 + 1e-9)) <= G.TOL


# ------------------------------------------------------------------------------------------ 2. the gap scene
def test_records_of_the_gap_scene(L, ctx, oracle):
    """polytope_ref.gap_scene(): 7 finders, so 57 idle lanes carry +inf into the butterfly.  States 0-5 (cores apart) are
    the _meshes entry's bit for bit; state 6 (the mesh across the cylinder's axis) holds the certificate below the sentinel."""
    scn, x, expect = P.gap_scene()
    radius = scn.shapes[0].dims[1]
    frames = oracle.OracleScene(scn).fk(x)
    sc = L.Scene(ctx, scn)
    rec, old = sc.min_distance_records_depth(x), sc.min_distance_records_meshes(x)
    col, col_old = sc.collision_records_depth(x, 4), sc.collision_records_meshes(x, 4)
    sc.close()
    print("dist", rec["dist"], "normal", rec["normal"])
    for k in KEYS + ("shape1", "shape2"):
        assert rec[k][:6].tobytes() == old[k][:6].tobytes(), k
    assert rec["shape1"].tolist() == [0] * 7 and rec["shape2"].tolist() == list(range(1, 8))
    w = R.Worst()
    for i in range(7):
        c = R.certify_scene_record(scn, frames[i], 0, 1 + i, rec["point1"][i], rec["point2"][i], rec["normal"][i], rec["dist"][i])
        assert c["apart"] == (i != 6)
        w.add(c, i)
    print("gap scene: %s" % w)
    assert not w.bad, _report(w)
    assert old["dist"][6] == -radius - 1e-9 and rec["dist"][6] < old["dist"][6]
    assert col["n_found"].tolist() == col_old["n_found"].tolist() == (expect < 0.0).astype(int).tolist()
    for k in ("shape1", "shape2"):
        assert col[k].tobytes() == col_old[k].tobytes()
    for i in range(7):
        k = int(col["n_found"][i])
        if k:  # the one colliding finder is the closest one: the same record from both kernels
            for key in KEYS + ("normal",):
                assert np.array_equal(_bits(col[key][i, 0]), _bits(rec[key][i])), (i, key)
        assert np.all(np.isposinf(col["dist"][i, k:])) and not col["normal"][i, k:].any() and not col["point1"][i, k:].any()


# ------------------------------------------------------------------------------------------ 3. two depths
def two_depths_scene(seed=3, radius=0.05, length=0.5, q=0.3):
    """A one-link chain carrying a capped cylinder (polytope_ref.gap_scene's), and two convex meshes across its axis at
    configuration q: the first in finder order off the axis (shallow), the second centred on it (deep).  States: q, and
    q + 2 (free)."""
    rng = np.random.default_rng(seed)
    scn = scenarios.make_pendulum(length=length)
    cap = T.Shape(kind=T.SHAPE_CCYLINDER, anchor=1)
    cap.pose = T.make_pose((0.5 * length, 0.0, 0.0), (np.cos(np.pi / 4), 0.0, np.sin(np.pi / 4), 0.0))
    cap.dims[:] = [length, radius, 0.0]
    tip = np.array([length * np.cos(q), 0.0, length * np.sin(q)])
    side = np.array([-np.sin(q), 0.0, np.cos(q)])
    shapes, pool = [cap], []
    for at, off in ((0.4, 0.045), (0.8, 0.0)):
        V = scenarios.random_convex_mesh(rng, 16, 0.08)
        s = T.Shape(kind=T.SHAPE_MESH, anchor=-1)
        s.pose = T.make_pose(tuple(at * tip + off * side), P._rand_quat(rng))
        s.dims[:] = [float(sum(len(v) for v in pool)), float(len(V)), 0.0]
        pool.append(V)
        shapes.append(s)
    scn.shapes = shapes
    scn.mesh_vertices = np.concatenate(pool)
    x = np.zeros((2, 2))
    x[:, 0] = [q, q + 2.0]
    return scn, x


def _scene_depths(scn, frames):
    """The reference's (cores apart, depth_ref) of the cylinder against each mesh at one state."""
    out = []
    a = G.shape_world(scn, frames, 0)
    WA = P.core_world(a, scn.mesh_vertices)[0]
    for j in range(1, len(scn.shapes)):
        WB = P.core_world(G.shape_world(scn, frames, j), scn.mesh_vertices)[0]
        out.append((G.reference(WA, WB)[0], R.depth_ref(WA, WB)[0]))
    return out


def test_the_deeper_of_two_crossing_meshes_wins(L, ctx, oracle):
    scn, x = two_depths_scene()
    frames = oracle.OracleScene(scn).fk(x)
    (ap1, d1), (ap2, d2) = _scene_depths(scn, frames[0])
    print("reference depths at the colliding state: %.6g (first), %.6g (second)" % (d1, d2))
    assert not ap1 and not ap2 and d1 > 1e-3 and d2 > d1 + 1e-3       # both cross, the second deeper
    assert all(ap for ap, _ in _scene_depths(scn, frames[1]))
    sc = L.Scene(ctx, scn)
    rec, old = sc.min_distance_records_depth(x), sc.min_distance_records_meshes(x)
    cols = {cap: (sc.collision_records_depth(x, cap), sc.collision_records_meshes(x, cap)) for cap in (1, 2, 3)}
    sc.close()
    assert (int(rec["shape1"][0]), int(rec["shape2"][0])) == (0, 2)    # the deeper
    assert (int(old["shape1"][0]), int(old["shape2"][0])) == (0, 1)    # the first at the sentinel
    for k in KEYS + ("shape1", "shape2"):                              # the free state: the _meshes record
        assert rec[k][1].tobytes() == old[k][1].tobytes(), k
    w = R.Worst()
    w.add(R.certify_scene_record(scn, frames[0], 0, 2, rec["point1"][0], rec["point2"][0], rec["normal"][0], rec["dist"][0]), "min")
    w.add(R.certify_scene_record(scn, frames[1], rec["shape1"][1], rec["shape2"][1], rec["point1"][1], rec["point2"][1],
                                 rec["normal"][1], rec["dist"][1]), "free")
    for cap, (col, col_old) in cols.items():
        assert col["n_found"].tolist() == col_old["n_found"].tolist() == [2, 0], cap
        k = min(2, cap)
        assert col["shape1"][0, :k].tolist() == [0] * k and col["shape2"][0, :k].tolist() == [1, 2][:k]    # finder order
        for k2 in ("shape1", "shape2"):
            assert col[k2].tobytes() == col_old[k2].tobytes()
        for i in range(k):
            w.add(R.certify_scene_record(scn, frames[0], 0, 1 + i, col["point1"][0, i], col["point2"][0, i], col["normal"][0, i],
                                         col["dist"][0, i]), (cap, i))
        if cap >= 2:
            for key in KEYS + ("normal",):
                assert np.array_equal(_bits(col[key][0, 1]), _bits(rec[key][0])), key
            assert col["dist"][0, 1] < col["dist"][0, 0] < 0.0
        for b, used in ((0, k), (1, 0)):    # unused slots
            assert np.all(np.isposinf(col["dist"][b, used:])) and not col["point1"][b, used:].any()
            assert not col["point2"][b, used:].any() and not col["normal"][b, used:].any()
            assert np.all(col["shape1"][b, used:] == PR.NO_SHAPE) and np.all(col["shape2"][b, used:] == PR.NO_SHAPE)
    print("two depths: %s" % w)
    assert not w.bad, _report(w)


# ------------------------------------------------------------------------------------------ 4. C4 with ten meshes
@pytest.fixture(scope="module")
def c4_case(oracle):
    """make_c4(n_obstacles=10, meshes=True) and the 64 random states of tests/test_gjk_records_gpu.py's c4_case (4 collide)."""
    scn = scenarios.make_c4(n_obstacles=10, meshes=True)
    x = PR.random_states(scn, 64, 5)
    return scn, x, oracle.OracleScene(scn).fk(x)


def test_c4_with_meshes_against_the_meshes_entries(L, ctx, c4_case):
    scn, x, frames = c4_case
    sc = L.Scene(ctx, scn)
    rec, old = sc.min_distance_records_depth(x), sc.min_distance_records_meshes(x)
    cap = 4
    col, col_old = sc.collision_records_depth(x, cap), sc.collision_records_meshes(x, cap)
    sc.close()
    assert col["n_found"].tolist() == col_old["n_found"].tolist()
    assert int(np.sum(col["n_found"] > 0)) == 4 and int(col["n_found"].max()) <= cap
    for k in ("shape1", "shape2"):
        assert col[k].tobytes() == col_old[k].tobytes(), k
    w = R.Worst()
    n_cross = 0
    for b in range(len(x)):
        for i in range(int(col["n_found"][b])):
            c = R.certify_scene_record(scn, frames[b], col["shape1"][b, i], col["shape2"][b, i], col["point1"][b, i],
                                       col["point2"][b, i], col["normal"][b, i], col["dist"][b, i])
            w.add(c, (b, i))
            if c["apart"]:     # swept shapes overlap, cores apart: gjk_record's values
                for k in KEYS:
                    assert np.array_equal(_bits(col[k][b, i]), _bits(col_old[k][b, i])), (b, i, k)
            else:
                n_cross += 1
                assert col["dist"][b, i] <= col_old["dist"][b, i]
        k = int(col["n_found"][b])
        assert np.all(np.isposinf(col["dist"][b, k:])) and not col["normal"][b, k:].any()
    # the minimum-distance records: the _meshes entry's wherever its winner's cores are apart
    for b in range(len(x)):
        c = R.certify_scene_record(scn, frames[b], rec["shape1"][b], rec["shape2"][b], rec["point1"][b], rec["point2"][b],
                                   rec["normal"][b], rec["dist"][b])
        w.add(c, ("min", b))
        old_apart = G.certify_scene_record(scn, frames[b], old["shape1"][b], old["shape2"][b], old["point1"][b], old["point2"][b],
                                           old["dist"][b])["apart"]
        if old_apart and c["apart"]:
            for k in KEYS + ("shape1", "shape2"):
                assert rec[k][b].tobytes() == old[k][b].tobytes(), (b, k)
        assert rec["dist"][b] <= old["dist"][b]
    print("c4 meshes: %d collision records (%d with crossing cores); %s" % (int(col["n_found"].sum()), n_cross, w))
    assert not w.bad, _report(w)     # (counted on the CPU: all 8 collision records of these states have their cores apart)


# ------------------------------------------------------------------------------------------ 5. scenes without meshes
def test_scenes_without_meshes_and_the_argument_rules(L, ctx):
    lib = L.load()
    scn = scenarios.make_c2()
    x = PR.random_states(scn, 32, 5)
    sc = L.Scene(ctx, scn)
    a, b = sc.min_distance_records(x), sc.min_distance_records_depth(x)
    for k in KEYS + ("shape1", "shape2"):
        assert a[k].tobytes() == b[k].tobytes(), k
    with np.errstate(divide="ignore", invalid="ignore"):
        expect = (a["point2"] - a["point1"]) / a["dist"][:, None]
    assert np.all(np.isfinite(a["dist"])) and np.all(a["dist"] != 0.0)
    # (the record's own distance divides, the reported one is the search's: they agree to rounding)
    assert float(np.max(np.abs(b["normal"] - expect))) <= 1e-12
    assert float(np.max(np.abs(np.linalg.norm(b["normal"], axis=1) - 1.0))) <= 1e-9
    a, b = sc.collision_records(x, 8), sc.collision_records_depth(x, 8)
    for k in ("n_found",) + KEYS + ("shape1", "shape2"):
        assert a[k].tobytes() == b[k].tobytes(), k
    unused = np.isposinf(a["dist"])
    assert not b["normal"][unused].any()
    sc.close()
    # planar scenes: refused, and the text says where their records come from
    sc = L.Scene(ctx, scenarios.make_c1_planar())
    xp = np.zeros((1, sc.D))
    for call in (lambda: sc.min_distance_records_depth(xp), lambda: sc.collision_records_depth(xp, 4)):
        with pytest.raises(L.RkhError) as e:
            call()
        assert e.value.status == -5 and "_2d" in str(e.value)
    sc.close()
    # an empty pair list
    sc = L.Scene(ctx, scenarios.make_hidim(3))
    assert sc.num_pairs == 0
    xh = np.full((5, sc.D), 0.25)
    rec = sc.min_distance_records_depth(xh)
    assert np.all(np.isposinf(rec["dist"])) and np.all(rec["shape1"] == PR.NO_SHAPE) and np.all(rec["shape2"] == PR.NO_SHAPE)
    assert not rec["point1"].any() and not rec["point2"].any() and not rec["normal"].any()
    col = sc.collision_records_depth(xh, 3)
    assert not col["n_found"].any() and np.all(col["shape1"] == PR.NO_SHAPE) and np.all(np.isposinf(col["dist"]))
    assert not col["normal"].any()
    # NULL pointers and B = 0
    dz, uz = (C.c_double * 64)(), (C.c_uint32 * 64)()
    xs = np.zeros(sc.D)
    args = [sc.h, T.dptr(xs), 1, dz, dz, dz, dz, uz, uz]
    for i in (0, 1, 3, 4, 5, 6, 7, 8):
        bad = list(args)
        bad[i] = None
        assert lib.rkh_min_distance_records_depth(*bad) == -1, i
    assert lib.rkh_min_distance_records_depth(sc.h, T.dptr(xs), 0, dz, dz, dz, dz, uz, uz) == 0
    args = [sc.h, T.dptr(xs), 1, 2, uz, dz, dz, dz, dz, uz, uz]
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 10):
        bad = list(args)
        bad[i] = None
        assert lib.rkh_collision_records_depth(*bad) == -1, i
    assert lib.rkh_collision_records_depth(sc.h, T.dptr(xs), 0, 2, uz, dz, dz, dz, dz, uz, uz) == 0
    sc.close()
    # the diagnostic entry
    one = (T.Shape * 1)(P.make_shape(T.SHAPE_SPHERE, (0, 0, 0), (0.1, 0, 0)))
    args = [ctx.h, one, one, 1, None, 0, dz, dz, dz, dz]
    for i in (0, 1, 2, 6, 7, 8, 9):
        bad = list(args)
        bad[i] = None
        assert lib.rkh_diag_gjk_depth_records(*bad) == -1, i
    assert lib.rkh_diag_gjk_depth_records(ctx.h, one, one, 0, None, 0, dz, dz, dz, dz) == 0


# ------------------------------------------------------------------------------------------ 6. the adaptor
def test_the_cpp_proximity_socket_with_depth_records(L, ctx, tmp_path):
    """tests/cpp/prox_records_depth_smoke.cpp (g++ against librkh.so) on the scene of (3): hip_proxy_query_pair with the
    depth switch on returns the C-ABI's depth records bit for bit, normals included; with the switch off, the _meshes
    entry's distance and no normal (the program exits with 5 otherwise)."""
    scn, xs = two_depths_scene()
    src = os.path.join(ROOT, "tests", "cpp", "prox_records_depth_smoke.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "prox_records_depth_smoke")
    newer = [src, os.path.join(ROOT, "include", "rkh_adaptors.hpp"), os.path.join(ROOT, "include", "rkh.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(f) for f in newer)):
        lib_dir = os.path.join(ROOT, "reak_amd")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                        "-L", lib_dir, "-lrkh", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    verts = np.ascontiguousarray(scn.mesh_vertices, dtype=np.float64).reshape(-1, 3)
    blob = tmp_path / "scene.bin"
    with open(blob, "wb") as f:
        f.write(np.int32(len(scn.ops)).tobytes())
        f.write(bytes(scn.ops_array()))
        f.write(bytes(scn.base))
        f.write(np.int32(len(scn.shapes)).tobytes())
        f.write(bytes(scn.shapes_array()))
        f.write(np.int32(len(verts)).tobytes())
        f.write(verts.tobytes())
        f.write(np.int32(len(xs)).tobytes())
        f.write(np.ascontiguousarray(xs).tobytes())
    run = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    out = json.loads(run.stdout.strip().splitlines()[-1])["states"]
    sc = L.Scene(ctx, scn)
    rec, old = sc.min_distance_records_depth(xs), sc.min_distance_records_meshes(xs)
    col = sc.collision_records_depth(xs, 8)
    sc.close()
    assert len(out) == 2 and col["n_found"].tolist() == [2, 0]
    for b, o in enumerate(out):
        assert o["dist"] == rec["dist"][b] and o["p1"] == rec["point1"][b].tolist() and o["p2"] == rec["point2"][b].tolist()
        assert o["n"] == rec["normal"][b].tolist() and o["plain_dist"] == old["dist"][b]
        assert (o["s1"], o["s2"]) == (int(rec["shape1"][b]), int(rec["shape2"][b]))
        assert len(o["hits"]) == int(col["n_found"][b])
        for i, h in enumerate(o["hits"]):
            assert h["dist"] == col["dist"][b, i] and h["p1"] == col["point1"][b, i].tolist()
            assert h["p2"] == col["point2"][b, i].tolist() and h["n"] == col["normal"][b, i].tolist()
            assert (h["s1"], h["s2"]) == (int(col["shape1"][b, i]), int(col["shape2"][b, i]))
    assert out[0]["dist"] < out[0]["plain_dist"] and (out[0]["s1"], out[0]["s2"]) == (0, 2)
