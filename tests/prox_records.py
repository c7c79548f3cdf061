"""Shared by the proximity-record tests: the reference side (tests/cpp/prox_record_ref.cpp: every finder's record and the
winner, from the oracle's closed forms), the device's closed forms compiled for the host (tests/cpp/prox_record_host.cpp),
random pairs for every routine, and the comparison rules of the GPU tests."""
import ctypes as C
import os
import subprocess

import numpy as np

from reak_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
DIST_TOL = 1e-12   # distances against the oracle (the project's verdict bar)
POINT_TOL = 1e-10  # points: POINT_TOL * max(1, |p|inf) (the project's bar on propagated quantities)
NO_SHAPE = 0xFFFFFFFF

# routine -> (kind of shape1, kind of shape2), createProxFinderList's cascade
ROUTINE_KINDS = {1: (T.SHAPE_SPHERE, T.SHAPE_SPHERE), 2: (T.SHAPE_SPHERE, T.SHAPE_CCYLINDER), 3: (T.SHAPE_SPHERE, T.SHAPE_BOX),
                 4: (T.SHAPE_CCYLINDER, T.SHAPE_CCYLINDER), 5: (T.SHAPE_CCYLINDER, T.SHAPE_BOX),
                 6: (T.SHAPE_PLANE, T.SHAPE_PLANE), 7: (T.SHAPE_PLANE, T.SHAPE_SPHERE), 8: (T.SHAPE_PLANE, T.SHAPE_CCYLINDER),
                 9: (T.SHAPE_PLANE, T.SHAPE_CYLINDER), 10: (T.SHAPE_PLANE, T.SHAPE_BOX), 11: (T.SHAPE_SPHERE, T.SHAPE_CYLINDER)}


def _build(src, out, includes):
    deps = [src, os.path.join(ROOT, "oracle", "reak_proximity.hpp"), os.path.join(ROOT, "oracle", "reak_math.hpp"),
            os.path.join(ROOT, "reak_amd", "csrc", "proximity_record_device.h"),
            os.path.join(ROOT, "reak_amd", "csrc", "proximity_device.h"), os.path.join(ROOT, "reak_amd", "csrc", "device_math.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(f) for f in deps):
        return out
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC"]
    for i in includes:
        cmd += ["-I", os.path.join(ROOT, i)]
    subprocess.run(cmd + [src, "-o", out], check=True)
    return out


_libs = {}


def ref_lib():
    if "ref" not in _libs:
        lib = C.CDLL(_build(os.path.join(CPP, "prox_record_ref.cpp"), os.path.join(CPP, "libprox_record_ref.so"),
                            ["oracle", "include"]))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        lib.prr_num_finders.argtypes = [C.POINTER(T.Shape), C.c_int]
        lib.prr_records.argtypes = [C.POINTER(T.Shape), C.c_int, dp, C.c_int, C.c_int, ip, ip, ip, dp, dp, dp, dp, ip]
        lib.prr_pair_records.argtypes = [C.POINTER(T.Shape), C.POINTER(T.Shape), C.c_int, C.c_int, dp]
        _libs["ref"] = lib
    return _libs["ref"]


def host_lib():
    if "host" not in _libs:
        lib = C.CDLL(_build(os.path.join(CPP, "prox_record_host.cpp"), os.path.join(CPP, "libprox_record_host.so"),
                            [os.path.join("tests", "cpp", "hip_host"), "include"]))
        lib.prh_pair_routine.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
        lib.prh_pair_records.argtypes = [C.POINTER(T.Shape), C.POINTER(T.Shape), C.c_int, C.c_int, C.POINTER(C.c_double)]
        _libs["host"] = lib
    return _libs["host"]


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


class RefRecords:
    """Every finder's record of a scenario's shapes at given chain frames, and findMinimumDistance's winner."""

    def __init__(self, scn):
        self.lib = ref_lib()
        self.n_shapes = len(scn.shapes)
        self._shapes = scn.shapes_array() if scn.shapes else (T.Shape * 1)()
        self.nf = self.lib.prr_num_finders(self._shapes, self.n_shapes)

    def records(self, frames):
        frames = np.ascontiguousarray(frames, dtype=np.float64)
        B, n_frames = frames.shape[0], frames.shape[1]
        nf = max(self.nf, 1)
        s1, s2, routine = (np.zeros(nf, dtype=np.int32) for _ in range(3))
        gap, dist = np.zeros((B, nf)), np.zeros((B, nf))
        p1, p2 = np.zeros((B, nf, 3)), np.zeros((B, nf, 3))
        winner = np.zeros(B, dtype=np.int32)
        got = self.lib.prr_records(self._shapes, self.n_shapes, T.dptr(frames), n_frames, B, _ip(s1), _ip(s2), _ip(routine),
                                   T.dptr(gap), T.dptr(dist), T.dptr(p1), T.dptr(p2), _ip(winner))
        assert got == self.nf
        n = self.nf
        return {"s1": s1[:n], "s2": s2[:n], "routine": routine[:n], "gap": gap[:, :n], "dist": dist[:, :n], "p1": p1[:, :n],
                "p2": p2[:, :n], "winner": winner}


def oracle_frames(oracle, scn, x):
    """[B][n_frames][7] from the oracle's chain (revolute chains)."""
    return oracle.OracleScene(scn).fk(x)


def restated_frames(scn, x):
    """The same from tests/kte_ref.py (chains with prismatic joints, which the oracle's chain does not know)."""
    import kte_ref

    ch = kte_ref.Chain(scn)
    return np.array([ch.frames(row) for row in np.atleast_2d(x)])


def random_states(scn, count, seed):
    rng = np.random.default_rng(seed)
    lo = np.array([scn.dyn.lower[i] for i in range(scn.D)])
    hi = np.array([scn.dyn.upper[i] for i in range(scn.D)])
    return rng.uniform(lo, hi, size=(count, scn.D))


def point_error(p, ref):
    """max over the points of |p - ref|inf / max(1, |ref|inf): to be held against POINT_TOL."""
    p, ref = np.asarray(p).reshape(-1, 3), np.asarray(ref).reshape(-1, 3)
    if len(p) == 0:
        return 0.0
    return float(np.max(np.max(np.abs(p - ref), axis=1) / np.maximum(1.0, np.max(np.abs(ref), axis=1))))


def check_min_records(sc, ref, frames, x, label, max_excluded=0.20):
    """The rules of rkh_min_distance_records against the reference side, on the states x (frames: their chain frames).
    Prints every figure before it asserts.  Returns the routines of the oracle's winners and the reference records."""
    rec = sc.min_distance_records(x)
    d_plain = sc.min_distance(x)
    R = ref.records(frames)
    B = len(x)
    finder_of = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(R["s1"], R["s2"]))}
    named = np.array([finder_of.get((int(a), int(b)), -1) for a, b in zip(rec["shape1"], rec["shape2"])])
    rows = np.arange(B)
    d_sorted = np.sort(R["dist"], axis=1)
    d_min = d_sorted[:, 0]
    clear = (d_sorted[:, 1] - d_min > 1e-9) if R["dist"].shape[1] > 1 else np.ones(B, dtype=bool)
    bit_equal = np.array_equal(rec["dist"].view(np.uint64), d_plain.view(np.uint64))
    unknown = int(np.sum(named < 0))
    nm = np.where(named < 0, 0, named)
    e_dist = float(np.max(np.abs(rec["dist"] - d_min)))
    e_named = float(np.max(np.abs(R["dist"][rows, nm] - d_min)))
    e_p1 = point_error(rec["point1"], R["p1"][rows, nm])
    e_p2 = point_error(rec["point2"], R["p2"][rows, nm])
    same_id = named == R["winner"]
    excluded = float(np.mean(~clear))
    print(f"{label}: B={B} finders={ref.nf} bit_equal={bit_equal} unknown_pairs={unknown} |d-oracle|max={e_dist:.3e} "
          f"named-finder excess max={e_named:.3e} point1 err={e_p1:.3e} point2 err={e_p2:.3e} "
          f"id mismatches where clear={int(np.sum(clear & ~same_id))} excluded from id check={excluded:.4f} "
          f"colliding={int(np.sum(d_min < 0))}")
    assert bit_equal, "dist differs from rkh_min_distance"
    assert unknown == 0, "a (shape1, shape2) that is no finder of the scene"
    assert e_dist <= DIST_TOL and e_named <= DIST_TOL
    assert e_p1 <= POINT_TOL and e_p2 <= POINT_TOL
    assert not np.any(clear & ~same_id)
    assert excluded <= max_excluded
    return R["routine"][R["winner"]], R


def reference_collisions(R, b):
    """(sure, maybe): finder indices of state b that gatherCollisionPoints reports -- not culled (gap > 0 skips) and
    d < 0 -- split at the verdict bar: a finder with |d| < 1e-12 or |gap| < 1e-12 may fall either way on the device."""
    gap, d = R["gap"][b], R["dist"][b]
    edge = (np.abs(d) < DIST_TOL) | (np.abs(gap) < DIST_TOL)
    hit = ~(gap > 0.0) & (d < 0.0)
    return np.flatnonzero(hit & ~edge), np.flatnonzero(edge)


# ---- one pair at a time ----------------------------------------------------------------------------------------------
def _quat(rng, mode):
    if mode == 0:
        return (1.0, 0.0, 0.0, 0.0)
    if mode == 1:  # a quarter turn about a coordinate axis: exactly parallel / perpendicular axes
        h = float(np.sqrt(0.5))
        return [(h, h, 0.0, 0.0), (h, 0.0, h, 0.0), (h, 0.0, 0.0, h)][int(rng.integers(0, 3))]
    q = rng.normal(size=4)
    return tuple(q / np.linalg.norm(q))


def random_dims(rng, kind, big_plane=False):
    """Sizes in the ranges of scenarios.make_c2 (planes: its 8 m floor if big_plane, else 0.5 .. 2 m)."""
    if kind == T.SHAPE_SPHERE:
        return [rng.uniform(0.05, 0.2), 0.0, 0.0]
    if kind == T.SHAPE_BOX:
        return list(rng.uniform(0.1, 0.4, size=3))
    if kind == T.SHAPE_CCYLINDER:
        return [rng.uniform(0.1, 0.4), rng.uniform(0.03, 0.1), 0.0]
    if kind == T.SHAPE_CYLINDER:
        return [rng.uniform(0.15, 0.4), rng.uniform(0.05, 0.15), 0.0]
    return [8.0, 8.0, 0.0] if big_plane else [rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0), 0.0]


def random_pairs(routine, count, seed):
    """`count` world-anchored (shape1, shape2) pairs of the routine's kinds, centres within 0.6 m so that a good share
    penetrates; a third with identity orientations, a third with quarter turns (parallel and perpendicular axes)."""
    rng = np.random.default_rng(seed)
    k1, k2 = ROUTINE_KINDS[routine]
    a, b = (T.Shape * count)(), (T.Shape * count)()
    for i in range(count):
        mode = i % 3
        for arr, kind in ((a, k1), (b, k2)):
            arr[i].kind, arr[i].anchor = kind, -1
            arr[i].pose = T.make_pose(rng.uniform(-0.3, 0.3, size=3), _quat(rng, mode))
            arr[i].dims[:] = [float(v) for v in random_dims(rng, kind)]
        if mode == 1 and i % 2 == 0:  # the same x: axes in one plane (never the same x AND y: the reference divides by
            b[i].pose.pos[0] = a[i].pose.pos[0]  # the lateral offset, coaxial shapes have no defined points)
    return a, b
