"""Shared by the tests of the support-map (GJK) records: gjk_record of reak_amd/csrc/gjk_device.h compiled for the host
(tests/cpp/gjk_record_host.cpp), and the CERTIFICATE of a record -- what makes two reported points a closest pair,
measured against the exact polytope distance of tests/polytope_ref.py and never against the code under test.

Where the closest pair of two polytopes is not unique (parallel faces, parallel edges) two correct answers can lie far
apart, so the points are certified, not compared.  With cores WA, WB (vertex sets), radii rA, rB, and the reference's
verdict on whether the cores are apart:

  cores apart     n_ref = the unit vector pb - pa of the reference's closest pair (the separating direction of two
                  disjoint convex sets is unique even where the points are not); qa = point1 - rA n_ref and
                  qb = point2 + rB n_ref must lie in conv(WA) and conv(WB) to 1e-12, and |qb - qa| must be
                  dist + rA + rB to 1e-12.  Two points of the two sets at the minimum distance ARE a closest pair.
  cores crossing  dist == -(rA + rB) - 1e-9 exactly; point1 in conv(WA) and point2 in conv(WB) to 1e-12;
                  |point1 - point2|inf <= 1e-12.

"In conv(W) to 1e-12": the distance of the point to all vertex triples and pairs of W (polytope_distance_all), which is
the distance to the set for a point on its boundary (witnesses of separated cores) and for any point of a segment or a
flat set; a point inside a full-dimensional core is on the inner side of every hull face (inside_hull)."""
import ctypes as C
import os
import subprocess

import numpy as np

import polytope_ref as P
from reak_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
TOL = 1e-12          # every figure of the certificate
POINT_TOL = 1e-10    # points against points: POINT_TOL * max(1, |p|inf) (tests/prox_records.py)

_lib = None


def host_lib():
    """tests/cpp/gjk_record_host.cpp as a shared library, built as prox_records._build does."""
    global _lib
    if _lib is None:
        src, out = os.path.join(CPP, "gjk_record_host.cpp"), os.path.join(CPP, "libgjk_record_host.so")
        csrc = os.path.join(ROOT, "reak_amd", "csrc")
        deps = [src] + [os.path.join(csrc, h) for h in ("gjk_device.h", "proximity_record_device.h", "proximity_device.h",
                                                        "device_math.h")]
        if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(f) for f in deps)):
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                            os.path.join(CPP, "hip_host"), "-I", os.path.join(ROOT, "include"), src, "-o", out], check=True)
        lib = C.CDLL(out)
        dp = C.POINTER(C.c_double)
        lib.grh_pair_records.argtypes = [C.POINTER(T.Shape), C.POINTER(T.Shape), C.c_int, dp, dp]
        lib.grh_no_record.argtypes = [C.POINTER(T.Shape), C.POINTER(T.Shape), dp]
        lib.grh_no_record.restype = C.c_double
        _lib = lib
    return _lib


def host_records(a, b, pool):
    """pair_record<true>(PR_GJK, a[i], b[i]) of the host build: {dist, point1, point2, gjk (gjk_distance of that build)}."""
    n = len(a)
    aa, bb = T.as_array(list(a), T.Shape), T.as_array(list(b), T.Shape)
    pool = np.ascontiguousarray(pool, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((n, 8))
    host_lib().grh_pair_records(aa, bb, n, T.dptr(pool), T.dptr(out))
    return {"point1": out[:, 0:3].copy(), "point2": out[:, 3:6].copy(), "dist": out[:, 6].copy(), "gjk": out[:, 7].copy()}


def to_core(W, q):
    """Distance of the point q to all vertex triples and pairs of W."""
    return P.polytope_distance_all(np.asarray(q, dtype=np.float64)[None], W)[0]


def outside_core(W, q):
    """How far q is from conv(W): 0.0 inside a full-dimensional core, else its distance to the triples and pairs."""
    d = to_core(W, q)
    if d > TOL and len(W) >= 4 and np.linalg.matrix_rank(W - W.mean(axis=0), tol=1e-9) == 3 and P.inside_hull(W, q, TOL):
        return 0.0
    return d


def reference(WA, WB, feat_a=None, feat_b=None):
    """(cores apart, core distance, pa, pb) of the reference."""
    d, pa, pb, ax = P.polytope_distance(WA, WB, feat_a, feat_b, with_axis=True)
    return P.separation(WA, WB, pa, pb, ax) > 0.0, d, pa, pb


def certificate(WA, ra, WB, rb, ref, point1, point2, dist):
    """The figures of one record, each to be held against TOL: {"apart": bool, "len", "in_a", "in_b", "same", "exact"}
    (len: cores apart only; same, exact: crossing cores only; the others 0.0 / True)."""
    apart, d_ref, pa, pb = ref
    point1, point2 = np.asarray(point1, dtype=np.float64), np.asarray(point2, dtype=np.float64)
    if apart:
        n_ref = (pb - pa) / np.linalg.norm(pb - pa)
        qa, qb = point1 - ra * n_ref, point2 + rb * n_ref
        return {"apart": True, "len": abs(float(np.linalg.norm(qb - qa)) - (dist + ra + rb)), "in_a": to_core(WA, qa),
                "in_b": to_core(WB, qb), "same": 0.0, "exact": True}
    return {"apart": False, "len": 0.0, "in_a": outside_core(WA, point1), "in_b": outside_core(WB, point2),
            "same": float(np.max(np.abs(point1 - point2))), "exact": dist == -(ra + rb) - P.OVERLAP}


def passes(c):
    return c["exact"] and max(c["len"], c["in_a"], c["in_b"], c["same"]) <= TOL


class Worst:
    """Running worst figures of many certificates, and the cases that miss."""

    def __init__(self):
        self.w = {"len": 0.0, "in_a": 0.0, "in_b": 0.0, "same": 0.0}
        self.n = self.n_apart = 0
        self.bad = []

    def add(self, c, label):
        self.n += 1
        self.n_apart += int(c["apart"])
        for k in self.w:
            self.w[k] = max(self.w[k], c[k])
        if not passes(c):
            self.bad.append((label, c))

    def __str__(self):
        return ("%d records (%d with the cores apart): | |qb - qa| - (dist + rA + rB) | max %.3g, point1 off its core %.3g, "
                "point2 off its core %.3g, crossing |point1 - point2|inf %.3g, %d miss" %
                (self.n, self.n_apart, self.w["len"], self.w["in_a"], self.w["in_b"], self.w["same"], len(self.bad)))


def family_references(cs, swap=False):
    """reference() of every case of a polytope_ref.Cases family (cached on the family), in either argument order."""
    key = "_gjk_record_refs_swapped" if swap else "_gjk_record_refs"
    if not hasattr(cs, key):
        refs = []
        for a, b in zip(cs.A, cs.B):
            a, b = (b, a) if swap else (a, b)
            (WA, ra), (WB, rb) = cs.core(a), cs.core(b)
            refs.append((WA, ra, WB, rb, reference(WA, WB, cs.features(a), cs.features(b))))
        setattr(cs, key, refs)
    return getattr(cs, key)


def certify_family(cs, rec, label, swap=False):
    """Certificate of rec = {dist, point1, point2} on every case of the family; prints the worst figures, returns Worst."""
    w = Worst()
    for i, (WA, ra, WB, rb, ref) in enumerate(family_references(cs, swap)):
        w.add(certificate(WA, ra, WB, rb, ref, rec["point1"][i], rec["point2"][i], float(rec["dist"][i])), (i, cs.label[i]))
    print("%s: %s" % (label, w))
    return w


def reference_points(cs):
    """([n][3], [n][3]): the reference's own closest points on the swept shapes, for families whose pairs are unique."""
    p1, p2 = [], []
    for WA, ra, WB, rb, (apart, d, pa, pb) in family_references(cs):
        n = (pb - pa) / np.linalg.norm(pb - pa)
        p1.append(pa + ra * n)
        p2.append(pb - rb * n)
    return np.array(p1), np.array(p2)


def point_error(p, ref):
    """max |p - ref|inf / max(1, |ref|inf)."""
    p, ref = np.asarray(p).reshape(-1, 3), np.asarray(ref).reshape(-1, 3)
    return float(np.max(np.max(np.abs(p - ref), axis=1) / np.maximum(1.0, np.max(np.abs(ref), axis=1)))) if len(p) else 0.0


# ---- scenes ----------------------------------------------------------------------------------------------------------
def shape_world(scn, frames, idx):
    """World-anchored copy of shape idx of the scenario at the chain frames [n_frames][7] (pos, quat) of one state."""
    s = scn.shapes[idx]
    if s.anchor < 0:
        return P.make_shape(s.kind, list(s.pose.pos), list(s.dims), list(s.pose.quat))
    f = frames[s.anchor]
    R = P.quat_rotmat(f[3:7])
    pos = f[:3] + R @ np.array(list(s.pose.pos))
    w1, x1, y1, z1 = f[3:7]
    w2, x2, y2, z2 = list(s.pose.quat)
    q = (w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
         w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2)
    return P.make_shape(s.kind, pos, list(s.dims), q)


def gjk_finders(scn):
    """(robot shape, environment shape) of every support-map finder of the scenario, in finder order (i-major over the
    anchored shapes, j-minor over the world's): the pairs with a mesh in them whose other shape the query knows.  The
    finder's shape1 is the robot's shape."""
    known = (T.SHAPE_SPHERE, T.SHAPE_CCYLINDER, T.SHAPE_BOX, T.SHAPE_MESH)
    robot = [i for i, s in enumerate(scn.shapes) if s.anchor >= 0]
    env = [i for i, s in enumerate(scn.shapes) if s.anchor < 0]
    return [(r, e) for r in robot for e in env
            if T.SHAPE_MESH in (scn.shapes[r].kind, scn.shapes[e].kind) and scn.shapes[r].kind in known and scn.shapes[e].kind in known]


def gjk_finder_distances(oracle, scn, frames, finders):
    """[B][len(finders)]: the oracle's gjk_distance of every finder at the chain frames [B][n_frames][7] of B states."""
    a, b = [], []
    for fr in frames:
        world = {i: shape_world(scn, fr, i) for i in set(r for r, _ in finders) | set(e for _, e in finders)}
        a += [world[r] for r, _ in finders]
        b += [world[e] for _, e in finders]
    return oracle.gjk_distance(a, b, scn.mesh_vertices).reshape(len(frames), len(finders))


def certify_scene_record(scn, frames, s1, s2, point1, point2, dist):
    """Certificate of one record of a scene: shapes s1, s2 of the scenario at one state's chain frames."""
    a, b = shape_world(scn, frames, int(s1)), shape_world(scn, frames, int(s2))
    (WA, ra), (WB, rb) = P.core_world(a, scn.mesh_vertices), P.core_world(b, scn.mesh_vertices)
    return certificate(WA, ra, WB, rb, reference(WA, WB), point1, point2, float(dist))
