"""Shared by the planar proximity-record tests, beside tests/prox_records.py: the reference side
(tests/cpp/prox_record_ref_2d.cpp: every finder's proximity_record_2D, the min_i the reference's culled loop leaves and the
margin of its decisions, from the oracle's closed forms), the device's planar closed forms compiled for the host
(tests/cpp/prox_record_host_2d.cpp), chain frames, random pairs for every routine, the scenes and seeds of the GPU tests,
and their comparison rules."""
import ctypes as C
import os
import subprocess

import numpy as np

import prox_records as PR
from reak_amd import scenarios
from reak_amd import types as T

ROOT = PR.ROOT
CPP = PR.CPP
DIST_TOL, POINT_TOL, NO_SHAPE = PR.DIST_TOL, PR.POINT_TOL, PR.NO_SHAPE
CLEAR_MARGIN = 1e-9   # check_min_records' margin: below it a decision of the replay may go either way on the device
MAX_EXCLUDED = 0.20   # check_min_records' default cap on the share of states left out of the id check
# Where the reference's points are defined.  Every routine that has two curved or swept shapes forms its points as
# a + (r / s) v with s = |v| the separation of two centres (circle centres, an end-cap centre, the closest points of two
# centre lines) and r a radius or half width <= 0.2 m; s = mDistance + rad1 + rad2 with rad = radius (circle), half
# width (capped rectangle), 0 (rectangle).  Where two centre lines cross (an open set of configurations of two
# penetrating capped rectangles) s is the rounding noise of the operands and so is the direction v / s: the reference's
# own points are arbitrary there, like the coaxial shapes tests/prox_records.py keeps out of its pairs.  Two chains of
# sincos, products and sums that differ in the last place (OCML against glibc: device_math.h) give frames about
# 7 joints x 2 ulp x 2 m = 3e-15 m apart; that moves a point by r x 3e-15 / s, which stays within POINT_TOL = 1e-10 for
# s >= 0.2 x 3e-15 / 1e-10 = 6e-6.  Records below MIN_SEPARATION are left out of the point comparison (never out of the
# distance or id comparison).  MAX_UNDEFINED caps their share: like MAX_EXCLUDED a condition on the states a test draws,
# held from the reference side alone (an arm of capped rectangles deep inside capped-rectangle obstacles crosses centre
# lines on several percent of its colliding states).
MIN_SEPARATION = 1e-5
MAX_UNDEFINED = 0.15

# routine -> (kind of shape1, kind of shape2), createProxFinderList's 2D cascade (proxy_query_model.cpp:75-161)
ROUTINE_KINDS = {11: (T.SHAPE_CIRCLE, T.SHAPE_CIRCLE), 12: (T.SHAPE_CIRCLE, T.SHAPE_CRECT), 13: (T.SHAPE_CIRCLE, T.SHAPE_RECTANGLE),
                 14: (T.SHAPE_CRECT, T.SHAPE_CRECT), 15: (T.SHAPE_CRECT, T.SHAPE_RECTANGLE),
                 16: (T.SHAPE_RECTANGLE, T.SHAPE_RECTANGLE)}


def _build(src, out, includes):
    csrc = os.path.join(ROOT, "reak_amd", "csrc")
    deps = [src, os.path.join(ROOT, "oracle", "reak_planar.hpp"), os.path.join(ROOT, "include", "rkh_types.h"),
            os.path.join(csrc, "proximity_record_planar_device.h"), os.path.join(csrc, "proximity_planar_device.h"),
            os.path.join(csrc, "device_math.h")]
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
        lib = C.CDLL(_build(os.path.join(CPP, "prox_record_ref_2d.cpp"), os.path.join(CPP, "libprox_record_ref_2d.so"),
                            ["oracle", "include"]))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        lib.prr2_num_finders.argtypes = [C.POINTER(T.Shape), C.c_int]
        lib.prr2_records.argtypes = [C.POINTER(T.Shape), C.c_int, dp, C.c_int, C.c_int, ip, ip, ip, dp, dp, dp, dp, ip, dp]
        lib.prr2_pair_records.argtypes = [C.POINTER(T.Shape), C.POINTER(T.Shape), C.c_int, C.c_int, dp]
        _libs["ref"] = lib
    return _libs["ref"]


def host_lib():
    if "host" not in _libs:
        lib = C.CDLL(_build(os.path.join(CPP, "prox_record_host_2d.cpp"), os.path.join(CPP, "libprox_record_host_2d.so"),
                            [os.path.join("tests", "cpp", "hip_host"), "include"]))
        lib.prh2_pair_records.argtypes = [C.POINTER(T.Shape), C.POINTER(T.Shape), C.c_int, C.c_int, C.POINTER(C.c_double)]
        _libs["host"] = lib
    return _libs["host"]


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


class RefRecords2D:
    """Every finder's record of a planar scenario's shapes at given chain frames [B][n_frames][4], the min_i of
    findMinimumDistance's replayed loop and the smallest margin of its decisions."""

    def __init__(self, scn):
        self.lib = ref_lib()
        self.n_shapes = len(scn.shapes)
        self._shapes = scn.shapes_array() if scn.shapes else (T.Shape * 1)()
        self.nf = self.lib.prr2_num_finders(self._shapes, self.n_shapes)
        self.rad = np.array([s.dims[0] if s.kind == T.SHAPE_CIRCLE else (0.5 * s.dims[1] if s.kind == T.SHAPE_CRECT else 0.0)
                             for s in scn.shapes] + [0.0])

    def records(self, frames):
        frames = np.ascontiguousarray(frames, dtype=np.float64)
        B, n_frames = frames.shape[0], frames.shape[1]
        assert frames.shape[2] == 4
        nf = max(self.nf, 1)
        s1, s2, routine = (np.zeros(nf, dtype=np.int32) for _ in range(3))
        gap, dist = np.zeros((B, nf)), np.zeros((B, nf))
        p1, p2 = np.zeros((B, nf, 2)), np.zeros((B, nf, 2))
        winner, margin = np.zeros(B, dtype=np.int32), np.zeros(B)
        got = self.lib.prr2_records(self._shapes, self.n_shapes, T.dptr(frames), n_frames, B, _ip(s1), _ip(s2), _ip(routine),
                                    T.dptr(gap), T.dptr(dist), T.dptr(p1), T.dptr(p2), _ip(winner), T.dptr(margin))
        assert got == self.nf
        n = self.nf
        sep = np.abs(dist[:, :n] + self.rad[s1[:n]] + self.rad[s2[:n]])  # see MIN_SEPARATION
        return {"s1": s1[:n], "s2": s2[:n], "routine": routine[:n], "gap": gap[:, :n], "dist": dist[:, :n], "p1": p1[:, :n],
                "p2": p2[:, :n], "winner": winner, "margin": margin, "sep": sep}


def restated_frames(scn, x):
    """[B][n_frames][4] (position, (cos, sin)) from tests/kte_ref_planar.py: revolute and prismatic planar chains."""
    import kte_ref_planar

    ch = kte_ref_planar.Chain(scn)
    return np.array([ch.frames(row) for row in np.atleast_2d(x)])


def oracle_frames(oracle, scn, x):
    """The same from the oracle's chain (revolute planar chains only: it does not know prismatic_joint_2D)."""
    return np.ascontiguousarray(oracle.OracleScene(scn).fk(x)[:, :, [0, 1, 3, 4]])


def random_states(scn, count, seed):
    """`count` states (q, qd = 0) with q uniform in the scenario's joint box (meta lower / upper; rate-limited coordinates
    are scaled back to joint values)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(scn.meta["lower"], dtype=float), np.asarray(scn.meta["upper"], dtype=float)
    if "speed_limits" in scn.meta:
        lo, hi = lo * scn.meta["speed_limits"], hi * scn.meta["speed_limits"]
    x = np.zeros((count, 2 * scn.n_dof))
    x[:, 0::2] = rng.uniform(lo, hi, size=(count, scn.n_dof))
    return x


def point_error(p, ref):
    """max over the points of |p - ref|inf / max(1, |ref|inf): to be held against POINT_TOL."""
    p, ref = np.asarray(p).reshape(-1, 2), np.asarray(ref).reshape(-1, 2)
    if len(p) == 0:
        return 0.0
    return float(np.max(np.max(np.abs(p - ref), axis=1) / np.maximum(1.0, np.max(np.abs(ref), axis=1))))


# ---- the scenes and states of the GPU test (the CPU test holds their share of unclear states against MAX_EXCLUDED) -----
def gpu_scenes():
    """(label, scenario factory, seed of the states) of test_proximity_records_planar_gpu.py's minimum-record cases."""
    import planar_prismatic_scenes as PPS

    return [("c1_planar", scenarios.make_c1_planar, 11), ("mixed2", lambda: scenarios.make_planar_mixed(n=2), 12),
            ("mixed4", lambda: scenarios.make_planar_mixed(n=4), 13), ("mixed7", lambda: scenarios.make_planar_mixed(n=7), 14),
            ("crs_a465_2d", scenarios.make_crs_a465_2d, 15), ("seven_prismatic", PPS.seven, 16)]


GPU_BATCHES = (1, 65, 1000)


def excluded_share(R):
    """Share of states the id check leaves out: some decision of the replay (a gap or a distance against the running
    minimum) had less than CLEAR_MARGIN of margin."""
    return float(np.mean(R["margin"] < CLEAR_MARGIN))


def check_min_records_2d(sc, ref, frames, x, label):
    """The rules of rkh_min_distance_records_2d against the reference side, on the states x (frames: their chain frames).
    Prints every figure before it asserts.  Returns the reference records."""
    rec = sc.min_distance_records_2d(x)
    d_plain = sc.min_distance(x)
    R = ref.records(frames)
    B = len(x)
    assert rec["point1"].shape == (B, 2) and rec["point2"].shape == (B, 2)
    finder_of = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(R["s1"], R["s2"]))}
    named = np.array([finder_of.get((int(a), int(b)), -1) for a, b in zip(rec["shape1"], rec["shape2"])])
    rows = np.arange(B)
    clear = R["margin"] >= CLEAR_MARGIN
    bit_equal = np.array_equal(rec["dist"].view(np.uint64), d_plain.view(np.uint64))
    unknown = int(np.sum(named < 0))
    nm = np.where(named < 0, 0, named)
    e_named = float(np.max(np.abs(rec["dist"] - R["dist"][rows, nm])))
    defined = R["sep"][rows, nm] >= MIN_SEPARATION
    e_p1 = point_error(rec["point1"][defined], R["p1"][rows, nm][defined])
    e_p2 = point_error(rec["point2"][defined], R["p2"][rows, nm][defined])
    same_id = named == R["winner"]
    excluded, undefined = float(np.mean(~clear)), float(np.mean(~defined))
    d_won = R["dist"][rows, R["winner"]]
    print(f"{label}: B={B} finders={ref.nf} bit_equal={bit_equal} unknown_pairs={unknown} |d - named finder's|max={e_named:.3e} "
          f"point1 err={e_p1:.3e} point2 err={e_p2:.3e} id mismatches where clear={int(np.sum(clear & ~same_id))} "
          f"excluded from id check={excluded:.4f} points undefined={undefined:.4f} colliding={int(np.sum(d_won < 0))} "
          f"winner is not the lowest distance={int(np.sum(d_won > np.min(R['dist'], axis=1)))}")
    assert bit_equal, "dist differs from rkh_min_distance"
    assert unknown == 0, "a (shape1, shape2) that is no finder of the scene"
    assert e_named <= DIST_TOL
    assert e_p1 <= POINT_TOL and e_p2 <= POINT_TOL
    assert not np.any(clear & ~same_id)
    assert excluded <= MAX_EXCLUDED
    assert int(np.sum(~defined)) <= int(MAX_UNDEFINED * B)
    return R


def check_collision_rows_2d(rec, R, rows, cap):
    """Device rows of rkh_collision_records_2d against the reference's list (gap > 0.0 skips, then d < 0.0, finder order;
    prox_records.reference_collisions' band for finders within 1e-12 of either threshold).  Returns (states with a
    collision, states at the verdict bar, worst errors, records compared, records whose points are undefined)."""
    finder_of = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(R["s1"], R["s2"]))}
    n_coll = n_edge = n_rec = n_undef = 0
    worst = {"d": 0.0, "p1": 0.0, "p2": 0.0}
    for b in rows:
        sure, maybe = PR.reference_collisions(R, b)
        n = int(rec["n_found"][b])
        k = min(n, cap)
        ids = [finder_of[(int(rec["shape1"][b, i]), int(rec["shape2"][b, i]))] for i in range(k)]
        assert ids == sorted(ids) and len(set(ids)) == len(ids), (b, ids)
        assert np.all(rec["shape1"][b, k:] == NO_SHAPE) and np.all(rec["shape2"][b, k:] == NO_SHAPE)
        assert np.all(np.isposinf(rec["dist"][b, k:])) and not rec["point1"][b, k:].any() and not rec["point2"][b, k:].any()
        if len(maybe):  # a finder within 1e-12 of 0 (distance or cull): either verdict is right
            n_edge += 1
            assert set(ids) <= set(sure) | set(maybe) and len(sure) <= n <= len(sure) + len(maybe), (b, ids, sure, maybe)
        else:
            assert n == len(sure) and ids == list(sure[:cap]), (b, n, ids, sure)
        n_coll += 1 if len(sure) else 0
        for i, fi in enumerate(ids):
            n_rec += 1
            worst["d"] = max(worst["d"], abs(rec["dist"][b, i] - R["dist"][b, fi]))
            if R["sep"][b, fi] < MIN_SEPARATION:
                n_undef += 1
                continue
            worst["p1"] = max(worst["p1"], point_error(rec["point1"][b, i], R["p1"][b, fi]))
            worst["p2"] = max(worst["p2"], point_error(rec["point2"][b, i], R["p2"][b, fi]))
    return n_coll, n_edge, worst, n_rec, n_undef


# ---- one pair at a time ----------------------------------------------------------------------------------------------
def _rot(rng, mode):
    if mode == 0:
        return (1.0, 0.0)
    if mode == 1:  # a quarter turn, exactly: parallel and perpendicular axes
        return [(0.0, 1.0), (0.0, -1.0), (-1.0, 0.0)][int(rng.integers(0, 3))]
    a = rng.uniform(-np.pi, np.pi)
    return (float(np.cos(a)), float(np.sin(a)))


def random_dims_2d(rng, kind):
    """Sizes in the ranges of scenarios.make_planar_mixed's obstacles."""
    if kind == T.SHAPE_CIRCLE:
        return [rng.uniform(0.06, 0.18), 0.0, 0.0]
    if kind == T.SHAPE_RECTANGLE:
        return [rng.uniform(0.15, 0.4), rng.uniform(0.15, 0.4), 0.0]
    return [rng.uniform(0.15, 0.4), rng.uniform(0.06, 0.16), 0.0]


def _centre_lines_cross(s1, s2):
    """Whether the centre-line segments of two capped rectangles cross (both orientations strictly opposite)."""
    def ends(s):
        h = 0.5 * s.dims[0]
        c, n = np.array([s.pose.pos[0], s.pose.pos[1]]), np.array([s.pose.quat[0], s.pose.quat[1]])
        return c - h * n, c + h * n

    def side(p, q, r):
        return (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])

    p1, p2 = ends(s1)
    p3, p4 = ends(s2)
    return side(p1, p2, p3) * side(p1, p2, p4) < 0.0 and side(p3, p4, p1) * side(p3, p4, p2) < 0.0


def random_pairs_2d(routine, count, seed):
    """`count` world-anchored (shape1, shape2) pairs of the routine's kinds, centres within 0.6 m so that a good share
    penetrates; a third with identity rotations, a third with quarter turns (the parallel and perpendicular branches), a
    third random.  Two capped rectangles never with crossing centre lines: the reference divides by the distance between
    the lines' closest points, which is then 0 (exactly, with perpendicular lines: NaN points) or rounding noise -- it
    defines no points there (MIN_SEPARATION above)."""
    rng = np.random.default_rng(seed)
    k1, k2 = ROUTINE_KINDS[routine]
    a, b = (T.Shape * count)(), (T.Shape * count)()
    for i in range(count):
        mode = i % 3
        while True:
            for arr, kind in ((a, k1), (b, k2)):
                arr[i].kind, arr[i].anchor = kind, -1
                c, s = _rot(rng, mode)
                arr[i].pose.pos[:] = [float(v) for v in rng.uniform(-0.3, 0.3, size=2)] + [0.0]
                arr[i].pose.quat[:] = [c, s, 0.0, 0.0]
                arr[i].dims[:] = [float(v) for v in random_dims_2d(rng, kind)]
            if routine != 14 or not _centre_lines_cross(a[i], b[i]):
                break
    return a, b
