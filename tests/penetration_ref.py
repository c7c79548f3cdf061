"""Reference, certificate and case families for the DEPTH records of support-map pairs (reak_amd/csrc/epa_device.h).
No EPA and no GJK in here.

The penetration depth of two crossing convex polytopes is the smallest overlap over the separating-axis candidates:

    depth_ref = min_n [ max_A n.a - min_B n.b ],

n over the unit face normals of A, those of B and the unit cross products of an edge of A with an edge of B, each with
both signs (faces and edges: polytope_ref.hull_features; a point core has neither, a segment core one edge).  The bracket
is the support function of D = A - B along n, the distance of the origin from D's supporting plane with that normal;
its minimum over all directions is attained at a facet normal of D, and every facet normal of A + (-B) is in the list.  A
candidate too many only adds a larger value.  depth_ref <= 0: the cores are apart or touching.

The CERTIFICATE of one record {dist, point1, point2, normal}, every figure held against gjk_records.TOL (1e-12):
  cores apart (gjk_records.reference)  gjk_records.certificate unchanged, and: | |n| - 1 |, and |n - n_ref|inf with n_ref
                  the reference's separating direction.  That direction is the unit normal of the reference's closest
                  feature pair where that normal separates the cores as widely as the witness pb - pa does (face /
                  vertex and edge / edge pairs: it does not degrade as the gap closes), else the unit witness.
  cores crossing  with qa = point1 - rA n, qb = point2 + rB n and depth = -dist - 1e-9 - rA - rB:
                  (i) | |n| - 1 |   (ii) |depth - depth_ref|   (iii) max_A n.a - min_B n.b - depth_ref (n is a minimising
                  direction; ties between facets are all right)   (iv) qa off conv(WA), qb off conv(WB)
                  (gjk_records.outside_core)   (v) |qa - qb - depth n|inf.
Nothing of it is taken from the code under test."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import gjk_records as G
import polytope_ref as P
from reak_amd import scenarios, types as T

TOL = G.TOL
CPP = G.CPP
ROOT = G.ROOT
_HEADERS = ("epa_device.h", "gjk_device.h", "proximity_record_device.h", "proximity_device.h", "device_math.h")


# ------------------------------------------------------------------ the reference
def _unit_rows(N):
    ln = np.sqrt(np.einsum("ij,ij->i", N, N))
    scale = float(np.max(ln)) if len(ln) else 0.0
    keep = ln > 1e-12 * max(scale, 1e-300)
    return N[keep] / ln[keep][:, None]


def _candidates(WA, WB, feat_a=None, feat_b=None):
    FA, EA = feat_a if feat_a is not None else P.hull_features(WA)
    FB, EB = feat_b if feat_b is not None else P.hull_features(WB)
    cand = []
    for W, F in ((WA, FA), (WB, FB)):
        if len(F):
            cand.append(_unit_rows(P._cross(W[F[:, 1]] - W[F[:, 0]], W[F[:, 2]] - W[F[:, 0]])))
    ea, eb = WA[EA[:, 1]] - WA[EA[:, 0]], WB[EB[:, 1]] - WB[EB[:, 0]]
    if len(ea) and len(eb):
        cand.append(_unit_rows(P._cross(ea[:, None, :], eb[None, :, :]).reshape(-1, 3)))
    cand = [c for c in cand if len(c)]
    return np.concatenate(cand) if cand else np.zeros((0, 3))


def width(WA, WB, n):
    """max_A n.a - min_B n.b: the support function of A - B along n.  Taken about A's first vertex, so that the rounding
    scales with the size of the cores and not with their distance from the world's origin."""
    return float(np.max((WA - WA[0]) @ n) - np.min((WB - WA[0]) @ n))


def depth_ref(WA, WB, feat_a=None, feat_b=None):
    """(depth_ref, a minimising unit direction).  Cores without any candidate (two points): (0.0, e_x) if they coincide."""
    WA, WB = np.atleast_2d(np.asarray(WA, dtype=np.float64)), np.atleast_2d(np.asarray(WB, dtype=np.float64))
    N = _candidates(WA, WB, feat_a, feat_b)
    if len(N) == 0:
        return float(-np.linalg.norm(WA[0] - WB[0])), np.array([1.0, 0.0, 0.0])
    pa, pb = (WA - WA[0]) @ N.T, (WB - WA[0]) @ N.T     # about A's first vertex, as in width()
    plus = pa.max(axis=0) - pb.min(axis=0)      # along +n
    minus = pb.max(axis=0) - pa.min(axis=0)     # along -n
    k, m = int(np.argmin(plus)), int(np.argmin(minus))
    return (float(plus[k]), N[k]) if plus[k] <= minus[m] else (float(minus[m]), -N[m])


def separating_direction(WA, WB, feat_a=None, feat_b=None):
    """The unit separating direction (from A towards B) of two cores that are apart; see the module docstring."""
    d, pa, pb, ax = P.polytope_distance(WA, WB, feat_a, feat_b, with_axis=True)
    wit = (pb - pa) / np.linalg.norm(pb - pa)
    la = float(np.sqrt(ax @ ax))
    if la > 0.0:
        n = ax / la
        n = n if n @ wit > 0.0 else -n
        gap = lambda v: float(np.min(WB @ v) - np.max(WA @ v))
        if gap(n) >= gap(wit) - 1e-15 * max(1.0, float(np.max(np.abs(WA))), float(np.max(np.abs(WB)))):
            return n
    return wit


def certificate(WA, ra, WB, rb, ref, dref, n_ref, point1, point2, normal, dist):
    """The figures of one depth record: {"apart", "unit", then apart: "len", "in_a", "in_b", "nrm"; crossing: "depth",
    "width", "in_a", "in_b", "same"} (the others 0.0)."""
    point1, point2, n = (np.asarray(v, dtype=np.float64) for v in (point1, point2, normal))
    c = {"apart": bool(ref[0]), "unit": abs(float(np.linalg.norm(n)) - 1.0), "len": 0.0, "nrm": 0.0, "depth": 0.0, "width": 0.0,
         "same": 0.0}
    if ref[0]:
        g = G.certificate(WA, ra, WB, rb, ref, point1, point2, dist)
        c.update(len=g["len"], in_a=g["in_a"], in_b=g["in_b"], nrm=float(np.max(np.abs(n - n_ref))))
        return c
    depth = -dist - P.OVERLAP - ra - rb
    qa, qb = point1 - ra * n, point2 + rb * n
    c.update(depth=abs(depth - dref), width=max(0.0, width(WA, WB, n) - dref), in_a=G.outside_core(WA, qa),
             in_b=G.outside_core(WB, qb), same=float(np.max(np.abs(qa - qb - depth * n))))
    return c


FIGURES = ("unit", "len", "nrm", "depth", "width", "in_a", "in_b", "same")


def passes(c, tol=TOL):
    return max(c[k] for k in FIGURES) <= tol


class Worst:
    def __init__(self):
        self.w = {k: 0.0 for k in FIGURES}
        self.n = self.n_apart = 0
        self.bad = []

    def add(self, c, label):
        self.n += 1
        self.n_apart += int(c["apart"])
        for k in FIGURES:
            self.w[k] = max(self.w[k], c[k])
        if not passes(c):
            self.bad.append((label, c))

    def __str__(self):
        return ("%d records (%d with the cores apart): " % (self.n, self.n_apart) +
                ", ".join("%s %.3g" % (k, self.w[k]) for k in FIGURES) + ", %d miss" % len(self.bad))


def family_references(cs, swap=False):
    """(WA, ra, WB, rb, gjk_records.reference, depth_ref, n_ref or None) of every case of a family, cached on it."""
    key = "_depth_refs_swapped" if swap else "_depth_refs"
    if not hasattr(cs, key):
        refs = []
        for a, b in zip(cs.A, cs.B):
            a, b = (b, a) if swap else (a, b)
            (WA, ra), (WB, rb) = cs.core(a), cs.core(b)
            fa, fb = cs.features(a), cs.features(b)
            ref = G.reference(WA, WB, fa, fb)
            refs.append((WA, ra, WB, rb, ref, depth_ref(WA, WB, fa, fb)[0],
                         separating_direction(WA, WB, fa, fb) if ref[0] else None))
        setattr(cs, key, refs)
    return getattr(cs, key)


def certify_family(cs, rec, label, swap=False):
    """Certificate of rec = {dist, point1, point2, normal} on every case of the family; prints and returns the Worst."""
    w = Worst()
    for i, (WA, ra, WB, rb, ref, dref, n_ref) in enumerate(family_references(cs, swap)):
        w.add(certificate(WA, ra, WB, rb, ref, dref, n_ref, rec["point1"][i], rec["point2"][i], rec["normal"][i],
                          float(rec["dist"][i])), (i, cs.label[i]))
    print("%s: %s" % (label, w))
    return w


def crossing(cs):
    """[n] bool: the reference's verdict on every case."""
    return np.array([not r[4][0] for r in family_references(cs)])


def certify_scene_record(scn, frames, s1, s2, point1, point2, normal, dist):
    """Certificate of one record of a scene: shapes s1, s2 of the scenario at one state's chain frames."""
    a, b = G.shape_world(scn, frames, int(s1)), G.shape_world(scn, frames, int(s2))
    (WA, ra), (WB, rb) = P.core_world(a, scn.mesh_vertices), P.core_world(b, scn.mesh_vertices)
    ref = G.reference(WA, WB)
    return certificate(WA, ra, WB, rb, ref, depth_ref(WA, WB)[0], separating_direction(WA, WB) if ref[0] else None, point1,
                       point2, normal, float(dist))


# ------------------------------------------------------------------ the host build
_lib = None


def _stale(out, deps):
    return not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(f) for f in deps))


def _deps():
    csrc = os.path.join(ROOT, "reak_amd", "csrc")
    return [os.path.join(CPP, "epa_record_host.cpp")] + [os.path.join(csrc, h) for h in _HEADERS]


def host_lib():
    """tests/cpp/epa_record_host.cpp as a shared library, built as gjk_records.host_lib does."""
    global _lib
    if _lib is None:
        out = os.path.join(CPP, "libepa_record_host.so")
        if _stale(out, _deps()):
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(CPP, "hip_host"),
                            "-I", os.path.join(ROOT, "include"), _deps()[0], "-o", out], check=True)
        lib = C.CDLL(out)
        dp = C.POINTER(C.c_double)
        lib.erh_pair_records.argtypes = [C.POINTER(T.Shape), C.POINTER(T.Shape), C.c_int, dp, dp]
        lib.erh_routine_records.argtypes = [C.POINTER(T.Shape), C.POINTER(T.Shape), C.c_int, dp, dp]
        lib.erh_max_verts_cap.restype = C.c_int
        _lib = lib
    return _lib


def host_program():
    """The same source with its own main, built with AddressSanitizer and UBSan: the path of the program."""
    out = os.path.join(CPP, "epa_record_host_asan")
    if _stale(out, _deps()):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-DERH_MAIN", "-I", os.path.join(CPP, "hip_host"), "-I",
                        os.path.join(ROOT, "include"), _deps()[0], "-o", out], check=True)
    return out


def write_pairs(path, a, b, pool):
    """The input file of host_program: int32 n, int32 pool vertices, the shapes of a, those of b, the pool."""
    pool = np.ascontiguousarray(pool, dtype=np.float64).reshape(-1, 3)
    with open(path, "wb") as f:
        f.write(np.array([len(a), len(pool)], dtype=np.int32).tobytes())
        f.write(bytes(T.as_array(list(a), T.Shape)))
        f.write(bytes(T.as_array(list(b), T.Shape)))
        f.write(pool.tobytes())


def host_records(a, b, pool):
    """pair_record_depth(PR_GJK, a[i], b[i]) of the host build: {dist, point1, point2, normal, depth_dist
    (pair_distance_depth of that build), verts (the polytope's vertex count; 0: EPA did not run)}."""
    n = len(a)
    aa, bb = T.as_array(list(a), T.Shape), T.as_array(list(b), T.Shape)
    pool = np.ascontiguousarray(pool, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((n, 12))
    host_lib().erh_pair_records(aa, bb, n, T.dptr(pool), T.dptr(out))
    return {"point1": out[:, 0:3].copy(), "point2": out[:, 3:6].copy(), "normal": out[:, 6:9].copy(), "dist": out[:, 9].copy(),
            "depth_dist": out[:, 10].copy(), "verts": out[:, 11].astype(int)}


def host_routine_records(a, b, pool):
    """pair_record_depth of the cascade's routine for (a[i], b[i]) beside the plain pair_record: {dist, point1, point2,
    normal, plain_dist, plain_point1, plain_point2}."""
    n = len(a)
    aa, bb = T.as_array(list(a), T.Shape), T.as_array(list(b), T.Shape)
    pool = np.ascontiguousarray(pool, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((n, 17))
    host_lib().erh_routine_records(aa, bb, n, T.dptr(pool), T.dptr(out))
    return {"point1": out[:, 0:3].copy(), "point2": out[:, 3:6].copy(), "normal": out[:, 6:9].copy(), "dist": out[:, 9].copy(),
            "plain_point1": out[:, 10:13].copy(), "plain_point2": out[:, 13:16].copy(), "plain_dist": out[:, 16].copy()}


# ------------------------------------------------------------------ case families
def shallow_cases():
    """(a) polytope_ref.penetrating_cases() as it is: 300 shallow mesh pairs."""
    return P.penetrating_cases()


DEEP_T = (1e-6, 1e-3, 0.05, 0.2)


@functools.lru_cache(maxsize=None)
def deep_cases(seed=47, count=15):
    """(b) count x len(DEEP_T) = 60 mesh pairs: B moved along the separated placement's witness by -(d + t).  Each case is
    classified by the reference; at t = 0.2 some come out apart again on the far side and stay in.  At least half cross."""
    cs = P.Cases()
    rng = np.random.default_rng(seed)
    for i in range(count):
        VA, VB, qa, qb, u = P._draw_mesh_pair(rng)
        WA, WB0 = VA @ P.quat_rotmat(qa).T, VB @ P.quat_rotmat(qb).T + u
        d, pa, pb = P.polytope_distance(WA, WB0, cs.features_of(VA), cs.features_of(VB))
        n = (pb - pa) / np.linalg.norm(pb - pa)
        a = cs.mesh(VA, (0, 0, 0), qa)
        for t in DEEP_T:
            cs.add_by_reference(a, cs.mesh(VB, u - n * (d + t), qb), f"seed {seed} pair {i} nv {len(VA)}/{len(VB)} t {t:g}")
    assert 2 * int(np.sum(crossing(cs))) >= len(cs), "deep_cases: fewer than half of the pairs cross"
    return cs


PARTNER_T = (0.05, 0.02, 1e-3)


@functools.lru_cache(maxsize=None)
def partner_cases(seed=43, count=10):
    """(c) Mesh against sphere / capped cylinder / box with crossing cores, in both argument orders: count draws per kind,
    2 x count cases each.  The partner is moved along the witness of the separated placement by -(d + t), t the first
    of PARTNER_T at which the reference finds the cores crossing (the sphere's centre inside the mesh, the capped
    cylinder's axis through it)."""
    cs = P.Cases()
    rng = np.random.default_rng(seed)
    for i in range(count):
        for kind in ("sphere", "ccyl", "box"):
            VA, _, qa, qb, u = P._draw_mesh_pair(rng)
            if kind == "sphere":
                k, dims = T.SHAPE_SPHERE, (rng.uniform(0.05, 0.2), 0, 0)
            elif kind == "ccyl":
                k, dims = T.SHAPE_CCYLINDER, (rng.uniform(0.1, 0.4), rng.uniform(0.03, 0.1), 0)
            else:
                k, dims = T.SHAPE_BOX, tuple(rng.uniform(0.1, 0.3, 3))
            a = cs.mesh(VA, (0, 0, 0), qa)
            (WA, _), (WB0, _) = cs.core(a), cs.core(P.make_shape(k, u, dims, qb))
            d, pa, pb = P.polytope_distance(WA, WB0, cs.features(a))
            n = (pb - pa) / np.linalg.norm(pb - pa)
            placed = None
            for t in PARTNER_T:
                b = P.make_shape(k, u - n * (d + t), dims, qb)
                WB = cs.core(b)[0]
                if not G.reference(WA, WB, cs.features(a))[0] and depth_ref(WA, WB, cs.features(a))[0] > 0.0:
                    placed = (b, t)
                    break
            assert placed is not None, "partner_cases: no crossing placement"
            b, t = placed
            lab = f"seed {seed} pair {i} mesh nv {len(VA)} / {kind} t {t:g}"
            cs.add_by_reference(a, b, lab)
            cs.add_by_reference(b, a, lab + " swapped")
    return cs


@functools.lru_cache(maxsize=None)
def hand_cases():
    """(d) Hand-built pairs with dyadic coordinates, each once more at an offset of 2^20 from the world's origin.
    cs.exact[i]: the exact depth where it is known by hand (else None)."""
    cs = P.Cases()
    cs.exact = []
    cube = scenarios.box_as_mesh([1.0, 1.0, 1.0])    # corners at +-0.5
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64) * 0.5
    roof_a = np.array([[0.5, 0, -1], [0.5, 0, 1], [-0.5, -0.5, 0], [-0.5, 0.5, 0]], dtype=np.float64)     # ridge along z at x = 0.5
    roof_b = np.array([[0, -1, 0], [0, 1, 0], [1, 0, -0.5], [1, 0, 0.5]], dtype=np.float64)               # ridge along y at x = 0
    square = np.array([[0.5, 0.5, 0], [-0.5, 0.5, 0], [-0.5, -0.5, 0], [0.5, -0.5, 0]], dtype=np.float64)
    for off in (0.0, 2.0 ** 20):
        o = np.array([off, -off, off])
        tag = "" if off == 0.0 else " at offset 2^20"

        def add(VA, VB, pos_b, label, exact):
            cs.add_by_reference(cs.mesh(VA, o), cs.mesh(VB, o + np.asarray(pos_b, dtype=np.float64)), label + tag)
            cs.exact.append(exact)

        add(cube, 0.5 * cube, (0.125, 0, 0), "cube in cube, offset along x", 0.625)
        add(cube, 0.5 * cube, (0, 0, 0), "cube in cube, centred", 0.75)
        add(cube, octa, (0.875, 0.125, -0.0625), "corner into face", 0.125)
        add(roof_a, roof_b, (0.375, 0.25, 0.125), "edge across edge", 0.125)
        add(cube, cube + [0.0, 0.25, -0.25], (1.0, 0, 0), "touching face / face", 0.0)
        add(cube, cube, (1.0, 1.0, 0.0), "touching edge / edge", 0.0)
        add(octa, octa, (1.0, 0, 0), "touching corner / corner", 0.0)
        add(cube, 0.25 * octa, (0.125, 0.0625, 0), "cube containing an octahedron", None)
        add(0.25 * octa, cube, (0.125, 0.0625, 0), "octahedron inside a cube", None)
        add(square, square, (0.25, 0.25, 0), "overlapping coplanar squares", 0.0)
    return cs


@functools.lru_cache(maxsize=None)
def continuity_cases(seed=47):
    """(e) A capped cylinder against a mesh, placed with the cores 1e-6 apart and 1e-6 deep along the witness.  The draw is
    the first of the seed's whose closest feature pair is a facet of A - B (the reference's depth at the deep placement is
    1e-6 to 1e-13; at a vertex or an edge of A - B the depth falls short of the travel at first order) and whose
    reference witness is good enough for the certificate of the placement with the cores apart."""
    rng = np.random.default_rng(seed)
    for i in range(200):
        cs = P.Cases()
        VA, _, qa, qb, u = P._draw_mesh_pair(rng)
        dims = (rng.uniform(0.1, 0.4), 2.0 ** -7, 0)     # a thin one: the witness's error enters times the radius
        b = cs.mesh(VA, (0, 0, 0), qa)
        (WB, _), (WA0, _) = cs.core(b), cs.core(P.make_shape(T.SHAPE_CCYLINDER, u, dims, qb))
        d, pa, pb = P.polytope_distance(WA0, WB, None, cs.features(b))
        n = (pb - pa) / np.linalg.norm(pb - pa)      # from the capped cylinder's axis towards the mesh
        for t in (-1e-6, 1e-6):
            cs.add_by_reference(P.make_shape(T.SHAPE_CCYLINDER, u + n * (d + t), dims, qb), b,
                                f"seed {seed} draw {i} capped cylinder / mesh nv {len(VA)} travel {t:g}")
        refs = family_references(cs)
        # (gjk_records.certificate steps the radius off along the reference's witness pb - pa, which at a gap of 1e-6 is a
        # direction good to 1e-10 or so: the draw must also be one whose witness meets the feature pair's normal)
        apart, d0, pa0, pb0 = refs[0][4]
        if apart and not refs[1][4][0] and abs(d0 - 1e-6) <= 1e-13 and abs(refs[1][5] - 1e-6) <= 1e-13 and \
                dims[1] * float(np.max(np.abs((pb0 - pa0) / np.linalg.norm(pb0 - pa0) - refs[0][6]))) <= 2e-13:
            return cs
    raise AssertionError("continuity_cases: no draw with a facet contact")


def families():
    return (("shallow", shallow_cases()), ("deep", deep_cases()), ("partners", partner_cases()), ("hand", hand_cases()),
            ("continuity", continuity_cases()))
