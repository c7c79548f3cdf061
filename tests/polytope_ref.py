"""Exact distance between two convex polytopes given by their vertices, in plain fp64 numpy -- and NO GJK.

The reference for the support-map query of reak_amd/csrc/gjk_device.h (and its CPU twin oracle/reak_gjk.hpp), which
otherwise is only compared with itself.  Two formulations:

  * polytope_distance: hull faces and edges by brute force (a vertex triple is a face if no vertex lies strictly on
    both sides of its plane, so a coplanar face contributes all its triples), then the minimum over vertex / triangle
    and edge / edge pairs with Ericson's closest-point routines (Real-Time Collision Detection 5.1.5, 5.1.9).  Any
    triangle or segment spanned by vertices lies inside the hull, so a feature too many never changes the minimum of a
    separated pair; the hull only keeps the lists short.
  * polytope_distance_all: the same minimum over ALL vertex triples and ALL vertex pairs, no hull.  Slow; cross-check.

Verdict without an LP: the witness direction n = pb - pa of a separated pair separates the vertex sets with a gap equal
to the distance; intersecting sets have no separating direction at all.  So `separation` (the widest support gap along
the witness and along the normal of the closest feature pair) is a lower bound of the distance that meets the upper
bound `dist` when the answer is right, and it is <= 0 for every intersecting pair.  Its reach: pa and pb carry the
rounding of the coordinates (1e-16), so the witness of a gap g is good to 1e-16 / g rad and the bound to about
1e-17 / g; the generators ask it for gaps down to 1e-8 only, and take closer pairs from constructions whose answer is
known (touching and 1e-12 gaps of dyadic coordinates, a shared point for the penetrating pairs).

Every partner of the query goes through the same routine by its core (sphere: 1 point, capped cylinder: 2 points, box:
8 corners, mesh: its vertices); the radii are subtracted afterwards, as the query defines it.

Also here: the deterministic case generators shared by tests/test_gjk_polytope_cpu.py and _gpu.py."""
import functools
import itertools

import numpy as np

from reak_amd import scenarios
from reak_amd import types as T

OVERLAP = 1e-9   # kGjkOverlap: intersecting cores return -(rA + rB) - OVERLAP


# ------------------------------------------------------------------ closest points (Ericson), vectorised
def _dot(a, b):
    return np.einsum("...i,...i->...", a, b)


def closest_point_triangle(p, a, b, c):
    """Closest point of triangle (a, b, c) to p; all arguments broadcast over leading axes (Ericson 5.1.5)."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        tab = d1 / (d1 - d3)
        tac = d2 / (d2 - d6)
        tbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
    e = lambda x: x[..., None]
    shape = np.broadcast(e(d1), a).shape
    full = lambda x: np.broadcast_to(x, shape)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    vals = [full(a), full(b), a + e(tab) * ab, full(c), a + e(tac) * ac, b + e(tbc) * (c - b)]
    inside = a + e(vb * den) * ab + e(vc * den) * ac
    return np.select([e(k) for k in conds], vals, default=inside)


def closest_points_segments(p1, q1, p2, q2):
    """Closest points (c1 on [p1, q1], c2 on [p2, q2]), broadcasting (Ericson 5.1.9, degenerate segments included),
    followed by two rounds of alternating projection: they can only shorten |c1 - c2|, and repair the parameter that
    the near-parallel determinant a*e - b*b leaves inexact."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f = _dot(d1, d1), _dot(d2, d2), _dot(d2, r)
    c, b = _dot(d1, r), _dot(d1, d2)
    sa, se = np.where(a > 0, a, 1.0), np.where(e > 0, e, 1.0)
    den = a * e - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(den > 0, np.clip((b * f - c * e) / np.where(den > 0, den, 1.0), 0.0, 1.0), 0.0)
    s = np.where(a > 0, s, 0.0)
    for _ in range(3):
        t = np.where(e > 0, np.clip((b * s + f) / se, 0.0, 1.0), 0.0)
        s = np.where(a > 0, np.clip((b * t - c) / sa, 0.0, 1.0), 0.0)
    t = np.where(e > 0, np.clip((b * s + f) / se, 0.0, 1.0), 0.0)
    return p1 + s[..., None] * d1, p2 + t[..., None] * d2


# ------------------------------------------------------------------ features
@functools.lru_cache(maxsize=None)
def _triples(n):
    return np.array(list(itertools.combinations(range(n), 3)), dtype=np.int64).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def _pairs(n):
    if n == 1:
        return np.array([[0, 0]], dtype=np.int64)
    return np.array(list(itertools.combinations(range(n), 2)), dtype=np.int64)


def hull_features(V):
    """(faces [F][3], edges [E][2]) of the convex hull of the vertex set V by brute force.  A triple is kept unless some
    vertex lies clearly on each side of its plane ("clearly": beyond the rounding of the plane's own normal, so a true
    face is never dropped; a near-coplanar triple too many is harmless).  Collinear triples carry no plane and are left
    out; a set without any face (fewer than three vertices, or all collinear) hands over all its vertex pairs."""
    V = np.asarray(V, dtype=np.float64)
    n = len(V)
    if n < 3:
        return np.zeros((0, 3), dtype=np.int64), _pairs(n)
    V = V - V.mean(axis=0)    # rigid motions do not change the features; centred, the plane offsets cancel least
    tri = _triples(n)
    a, b, c = V[tri[:, 0]], V[tri[:, 1]], V[tri[:, 2]]
    ab, ac = b - a, c - a
    nrm = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                    ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], axis=1)
    ln = np.sqrt(_dot(nrm, nrm))
    scale = max(float(np.sqrt(np.max(_dot(V, V)))), 1e-300)
    ok = ln > 1e-12 * scale * scale
    tri, a, nrm, ln = tri[ok], a[ok], nrm[ok], ln[ok]
    if len(tri) == 0:
        return np.zeros((0, 3), dtype=np.int64), _pairs(n)
    s = (nrm @ V.T - _dot(nrm, a)[:, None]) / ln[:, None]
    tol = (scale * (1e-12 + 1e-15 * scale * scale / ln))[:, None]
    face = ~((s > tol).any(axis=1) & (s < -tol).any(axis=1))
    faces = tri[face]
    e = np.concatenate([faces[:, [0, 1]], faces[:, [0, 2]], faces[:, [1, 2]]])
    return faces, np.unique(e, axis=0)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _min_over_features(WA, WB, FA, EA, FB, EB):
    """WB carries a leading axis: G placements [G][nB][3] of the same vertex set, answered in one sweep.  Besides the
    distance and the closest points, the normal of the winning feature pair (the triangle's normal, or the cross
    product of the two edges): for `separation`, which needs a direction better than pb - pa is at a tiny distance."""
    G = len(WB)
    best, bpa, bpb, bax = np.full(G, np.inf), np.zeros((G, 3)), np.zeros((G, 3)), np.zeros((G, 3))
    g = np.arange(G)

    def take(d2, pa, pb, ax):
        shape = d2.shape
        d2 = d2.reshape(G, -1)
        k = np.argmin(d2, axis=1)
        better = d2[g, k] < best
        sel = lambda x: np.broadcast_to(x, shape + (3,)).reshape(G, -1, 3)[g, k][better]
        best[better], bpa[better], bpb[better], bax[better] = d2[g, k][better], sel(pa), sel(pb), sel(ax)

    if len(FA):    # vertices of B against the triangles of A
        a, b, c = WA[FA[:, 0]][None, None], WA[FA[:, 1]][None, None], WA[FA[:, 2]][None, None]
        p = np.broadcast_to(WB[:, :, None, :], (G, WB.shape[1], len(FA), 3))
        q = closest_point_triangle(p, a, b, c)
        take(_dot(p - q, p - q), q, p, _cross(b - a, c - a))
    if len(FB):
        a, b, c = WB[:, FB[:, 0]][:, None], WB[:, FB[:, 1]][:, None], WB[:, FB[:, 2]][:, None]
        p = np.broadcast_to(WA[None, :, None, :], (G, len(WA), len(FB), 3))
        q = closest_point_triangle(p, a, b, c)
        take(_dot(p - q, p - q), p, q, _cross(b - a, c - a))
    p1, q1 = WA[EA[:, 0]][None, :, None], WA[EA[:, 1]][None, :, None]
    p2, q2 = WB[:, EB[:, 0]][:, None], WB[:, EB[:, 1]][:, None]
    c1, c2 = closest_points_segments(p1, q1, p2, q2)
    take(_dot(c1 - c2, c1 - c2), c1, c2, _cross(q1 - p1, q2 - p2))
    return np.sqrt(best), bpa, bpb, bax


def polytope_distance(WA, WB, feat_a=None, feat_b=None, with_axis=False):
    """(dist, pa, pb): distance between conv(WA) and conv(WB) and a closest pair of points.  Meaningful for separated
    sets; for intersecting ones it is some distance between boundary features -- ask `separation` for the verdict.
    feat_a, feat_b: hull_features of the sets where the caller has them already (a rigid motion keeps them).
    WB may be [G][nB][3], G placements of one vertex set: then dist is [G] and pa, pb are [G][3].
    with_axis: a fourth value, the (unnormalised, possibly zero) normal of the closest feature pair."""
    WA, WB = np.atleast_2d(np.asarray(WA, dtype=np.float64)), np.atleast_2d(np.asarray(WB, dtype=np.float64))
    many = WB.ndim == 3
    FA, EA = feat_a if feat_a is not None else hull_features(WA)
    FB, EB = feat_b if feat_b is not None else hull_features(WB[0] if many else WB)
    r = _min_over_features(WA, WB if many else WB[None], FA, EA, FB, EB)
    r = r if many else (float(r[0][0]), r[1][0], r[2][0], r[3][0])
    return r if with_axis else r[:3]


def polytope_distance_all(WA, WB):
    """The same over all vertex triples and all vertex pairs of each set: no hull.  Cross-check only."""
    WA, WB = np.atleast_2d(np.asarray(WA, dtype=np.float64)), np.atleast_2d(np.asarray(WB, dtype=np.float64))

    def feats(V):
        n = len(V)
        tri = _triples(n) if n >= 3 else np.zeros((0, 3), dtype=np.int64)
        if len(tri):    # a collinear triple is covered by its pairs; Ericson's interior branch would divide by zero on it
            nrm = _cross(V[tri[:, 1]] - V[tri[:, 0]], V[tri[:, 2]] - V[tri[:, 0]])
            tri = tri[_dot(nrm, nrm) > 0.0]
        return tri, _pairs(n)

    FA, EA = feats(WA)
    FB, EB = feats(WB)
    d, pa, pb, _ = _min_over_features(WA, WB[None], FA, EA, FB, EB)
    return float(d[0]), pa[0], pb[0]


def separation(WA, WB, pa, pb, axis=None):
    """The widest support gap min_B n.b - max_A n.a of the two vertex sets over the candidate directions n: the witness
    (pb - pa) / |pb - pa| and, where given, +-axis (the normal of the closest feature pair, whose direction does not
    degrade as the sets approach).  Any positive gap proves the sets apart and bounds the distance from below; for the
    closest pair of separated sets it EQUALS the distance.  Intersecting sets have no separating direction: <= 0
    (0.0 when pa == pb and no axis separates)."""
    WA, WB = np.asarray(WA, dtype=np.float64), np.asarray(WB, dtype=np.float64)
    cand = [np.asarray(pb, dtype=np.float64) - np.asarray(pa, dtype=np.float64)]
    if axis is not None:
        cand += [np.asarray(axis, dtype=np.float64), -np.asarray(axis, dtype=np.float64)]
    best = -np.inf
    for n in cand:
        ln = np.sqrt(n @ n)
        if ln > 0.0:
            n = n / ln
            best = max(best, float(np.min(WB @ n) - np.max(WA @ n)))
    return best if best > -np.inf else 0.0


def cores_distance(WA, WB):
    """(dist, pa, pb, free).  free = the cores are apart; certified: the separation along the witness is positive and
    meets dist (the caller may assert that).  Touching (dist == 0) counts as intersecting."""
    d, pa, pb, ax = polytope_distance(WA, WB, with_axis=True)
    return d, pa, pb, separation(WA, WB, pa, pb, ax) > 0.0


def expected_query(WA, WB, ra=0.0, rb=0.0):
    """What the support-map query is defined to return for cores WA, WB swept by the radii ra, rb."""
    d, _, _, free = cores_distance(WA, WB)
    return d - ra - rb if free else -(ra + rb) - OVERLAP


# ------------------------------------------------------------------ shapes <-> cores
def quat_rotmat(q):
    w, x, y, z = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def make_shape(kind, pos, dims, quat=(1.0, 0.0, 0.0, 0.0)):
    s = T.Shape(kind=kind, anchor=-1)
    s.pose = T.make_pose(tuple(float(v) for v in pos), tuple(float(v) for v in quat))
    s.dims[:] = [float(v) for v in dims]
    return s


def core_local(shape, pool=None):
    """(local core vertices, radius) of a world-anchored shape."""
    k, d = shape.kind, list(shape.dims)
    if k == T.SHAPE_SPHERE:
        return np.zeros((1, 3)), d[0]
    if k == T.SHAPE_CCYLINDER:
        return np.array([[0.0, 0.0, -0.5 * d[0]], [0.0, 0.0, 0.5 * d[0]]]), d[1]
    if k == T.SHAPE_BOX:
        return scenarios.box_as_mesh(d), 0.0
    assert k == T.SHAPE_MESH
    return np.asarray(pool, dtype=np.float64).reshape(-1, 3)[int(d[0]):int(d[0]) + int(d[1])], 0.0


def core_world(shape, pool=None):
    V, r = core_local(shape, pool)
    return V @ quat_rotmat(list(shape.pose.quat)).T + np.array(list(shape.pose.pos)), r


class Cases:
    """A family of world-anchored pairs for gjk_distance(A, B, pool), with the reference's value for each."""

    def __init__(self):
        self._mesh, self._feat = {}, {}
        self.A, self.B, self._pool, self.expect, self.label, self._n, self._rsum = [], [], [], [], [], 0, []

    def mesh(self, V, pos=(0.0, 0.0, 0.0), quat=(1.0, 0.0, 0.0, 0.0)):
        V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
        s = make_shape(T.SHAPE_MESH, pos, (float(self._n), float(len(V)), 0.0), quat)
        self._pool.append(V)
        self._mesh[self._n] = V
        self._feat[self._n] = self.features_of(V)
        self._n += len(V)
        return s

    @property
    def pool(self):
        return np.concatenate(self._pool) if self._pool else np.zeros((1, 3))

    def core(self, s):
        """(world core vertices, radius) of one of this family's shapes."""
        if s.kind == T.SHAPE_MESH:
            V = self._mesh[int(s.dims[0])]
            return V @ quat_rotmat(list(s.pose.quat)).T + np.array(list(s.pose.pos)), 0.0
        return core_world(s)

    def features_of(self, V):
        key = np.ascontiguousarray(V, dtype=np.float64).tobytes()
        if key not in self._feat:
            self._feat[key] = hull_features(V)
        return self._feat[key]

    def features(self, s):
        """hull_features of a mesh of this family (computed once per vertex set, in its local frame); None otherwise."""
        return self._feat[int(s.dims[0])] if s.kind == T.SHAPE_MESH else None

    def add(self, a, b, expect, label):
        self.A.append(a); self.B.append(b); self.expect.append(float(expect)); self.label.append(label)
        self._rsum.append(core_local(a, np.zeros((0, 3)))[1] + core_local(b, np.zeros((0, 3)))[1])

    def add_by_reference(self, a, b, label):
        """Expected value = the reference evaluated on the shapes exactly as the query will see them.  Returns the
        reference's certificate (dist, separation along the witness, free)."""
        (WA, ra), (WB, rb) = self.core(a), self.core(b)
        d, pa, pb, ax = polytope_distance(WA, WB, self.features(a), self.features(b), with_axis=True)
        sep = separation(WA, WB, pa, pb, ax)
        self.add(a, b, d - ra - rb if sep > 0.0 else -(ra + rb) - OVERLAP, label)
        return d, sep, sep > 0.0

    def add_placements(self, a, bs, labels):
        """add_by_reference for several placements bs of one shape against a, in one sweep of the reference."""
        WA, ra = self.core(a)
        WB = np.stack([self.core(b)[0] for b in bs])
        rb = self.core(bs[0])[1]
        d, pa, pb, ax = polytope_distance(WA, WB, self.features(a), self.features(bs[0]), with_axis=True)
        out = []
        for g, (b, lab) in enumerate(zip(bs, labels)):
            sep = separation(WA, WB[g], pa[g], pb[g], ax[g])
            self.add(a, b, d[g] - ra - rb if sep > 0.0 else -(ra + rb) - OVERLAP, lab)
            out.append((float(d[g]), sep, sep > 0.0))
        return out

    def __len__(self):
        return len(self.A)

    def free(self):
        return np.array(self.expect) > -np.array(self._rsum) - 0.5 * OVERLAP

    def check(self, got, tol=1e-10):
        """Indices of the cases that `got` misses: free pairs to tol, colliding pairs exactly."""
        got, exp, free = np.asarray(got), np.array(self.expect), self.free()
        bad = np.where(free, np.abs(got - exp) > tol, got != exp)
        return [(int(i), self.label[i], exp[i], got[i]) for i in np.nonzero(bad)[0]]


def _rand_quat(rng):
    q = rng.normal(size=4)
    return tuple(q / np.linalg.norm(q))


def _draw_mesh_pair(rng):
    """A mesh (as in the issue: 4-32 vertices on an ellipsoid of bounding radius 0.2, random attitude, at the origin)
    and a partner 0.6 away in a random direction."""
    VA, VB = (scenarios.random_convex_mesh(rng, int(rng.integers(4, 33)), 0.2) for _ in range(2))
    qa, qb = _rand_quat(rng), _rand_quat(rng)
    u = rng.normal(size=3)
    u = 0.6 * u / np.linalg.norm(u)
    return VA, VB, qa, qb, u


GAPS = (1e-2, 1e-4, 1e-6, 1e-8)
# (seed, pairs drawn).  Of seeds 11-14 at 400 pairs each (6400 cases) the GJK before the certified exit got four cases
# wrong: seed 11 pair 392 at 1e-6 (0.0212), seed 13 pair 73 at 1e-4 (collision) and pair 358 at 1e-4 (2.3e-4), seed 14
# pair 118 at 1e-2 (0.0425).  Kept: the shortest prefixes that hold three of them.
GAP_SEEDS = ((13, 360), (14, 120))


@functools.lru_cache(maxsize=None)
def gap_placed_cases(seeds=GAP_SEEDS, gaps=GAPS):
    """(a) Free mesh / mesh pairs placed at a known gap: B is moved along the witness n of the comfortable placement so
    that its closest point lands `gap` short of A's.  Expected = the reference at the placed pose, not the gap."""
    cs = Cases()
    cs.cert = []
    for seed, count in seeds:
        rng = np.random.default_rng(seed)
        for i in range(count):
            VA, VB, qa, qb, u = _draw_mesh_pair(rng)
            WA, WB0 = VA @ quat_rotmat(qa).T, VB @ quat_rotmat(qb).T + u
            d, pa, pb = polytope_distance(WA, WB0, cs.features_of(VA), cs.features_of(VB))
            n = (pb - pa) / np.linalg.norm(pb - pa)
            a = cs.mesh(VA, (0, 0, 0), qa)
            cs.cert += cs.add_placements(a, [cs.mesh(VB, u - n * (d - gap), qb) for gap in gaps],
                                         [f"seed {seed} pair {i} nv {len(VA)}/{len(VB)} gap {gap:g}" for gap in gaps])
    return cs


EPS = (1e-2, 1e-4, 1e-6)


@functools.lru_cache(maxsize=None)
def penetrating_cases(seed=21, count=100):
    """(b) Pairs that intersect by construction: B is translated so that its closest boundary point pb lands on
    pa + eps (cA - pa), a point of A (cA = vertex mean of A).  Expected: -(rA + rB) - 1e-9 exactly."""
    cs = Cases()
    cs.shared = []
    rng = np.random.default_rng(seed)
    for i in range(count):
        VA, VB, qa, qb, u = _draw_mesh_pair(rng)
        WA, WB0 = VA @ quat_rotmat(qa).T, VB @ quat_rotmat(qb).T + u
        d, pa, pb = polytope_distance(WA, WB0, cs.features_of(VA), cs.features_of(VB))
        a = cs.mesh(VA, (0, 0, 0), qa)
        for eps in EPS:
            shared = pa + eps * (WA.mean(axis=0) - pa)
            b = cs.mesh(VB, u + shared - pb, qb)
            cs.add(a, b, -OVERLAP, f"seed {seed} pair {i} nv {len(VA)}/{len(VB)} eps {eps:g}")
            cs.shared.append(shared)
    return cs


@functools.lru_cache(maxsize=None)
def partner_cases(seed=31, count=60):
    """(d) Mesh against sphere, capped cylinder and box, drawn and gap-placed as in (a), in both argument orders."""
    cs = Cases()
    cs.cert = []
    rng = np.random.default_rng(seed)
    for i in range(count):
        for kind in ("sphere", "ccyl", "box"):
            VA, _, qa, qb, u = _draw_mesh_pair(rng)
            if kind == "sphere":
                k, dims = T.SHAPE_SPHERE, (rng.uniform(0.05, 0.2), 0, 0)
            elif kind == "ccyl":
                k, dims = T.SHAPE_CCYLINDER, (rng.uniform(0.1, 0.4), rng.uniform(0.03, 0.1), 0)
            else:
                k, dims = T.SHAPE_BOX, tuple(rng.uniform(0.1, 0.3, 3))
            a = cs.mesh(VA, (0, 0, 0), qa)
            b0 = make_shape(k, u, dims, qb)
            (WA, _), (WB0, rb) = cs.core(a), cs.core(b0)
            d, pa, pb = polytope_distance(WA, WB0, cs.features(a))
            n = (pb - pa) / np.linalg.norm(pb - pa)
            labs = [f"seed {seed} pair {i} mesh nv {len(VA)} / {kind} gap {gap:g}" for gap in GAPS]
            cs.cert += cs.add_placements(a, [make_shape(k, u - n * (d - rb - gap), dims, qb) for gap in GAPS], labs)
            for b, e, lab in list(zip(cs.B, cs.expect, cs.label))[-len(GAPS):]:
                cs.add(b, a, e, lab + " swapped")
    return cs


@functools.lru_cache(maxsize=None)
def edge_cases():
    """(c) Hand-built degenerate pairs with analytic expectations.  The coordinates are dyadic, so a touching pair
    touches exactly (and collides) and a placed gap g is g to the rounding of 0.5 + g (1e-16); a gap of 1e-12 is free."""
    cs = Cases()
    cube = scenarios.box_as_mesh([1.0, 1.0, 1.0])             # corners at +-0.5
    qz45 = (np.cos(np.pi / 8), 0.0, 0.0, np.sin(np.pi / 8))
    s2 = np.sqrt(2.0)
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64) * 0.5
    # the gap is carried by B's position: A's face / edge / corner sits at x = 0.5
    gaps = (1.0, 1e-3, 1e-6, 1e-9, 1e-12, 0.0)
    for g in gaps:
        exp = g if g > 0 else -OVERLAP
        # face to face (B's vertices shifted in y, z: the faces overlap partly)
        cs.add(cs.mesh(cube), cs.mesh(cube + [0.0, 0.25, -0.25], (1.0 + g, 0, 0)), exp, f"cube face/face gap {g:g}")
        # parallel edges: two squares' worth of cube edges along z, B offset diagonally in x, y
        cs.add(cs.mesh(cube), cs.mesh(cube, (1.0 + g, 1.0, 0.0)), exp, f"cube edge/edge parallel gap {g:g}")
        # vertex to vertex: octahedra tip to tip
        cs.add(cs.mesh(octa), cs.mesh(octa, (1.0 + g, 0, 0)), exp, f"octahedron vertex/vertex gap {g:g}")
        # vertex to face
        cs.add(cs.mesh(cube), cs.mesh(octa, (1.0 + g, 0.125, -0.0625)), exp, f"cube face / octahedron vertex gap {g:g}")
        # crossed edges: a segment along y over a segment along z
        cs.add(cs.mesh([[0.5, -1, 0], [0.5, 1, 0]]), cs.mesh([[0, 0, -1], [0, 0, 1]], (0.5 + g, 0.25, 0.125)), exp,
               f"crossed segments gap {g:g}")
        # meshes of 1, 2, 3 and 4 coplanar vertices against the cube's face
        flat = np.array([[0, 0.25, 0.125], [0, -0.125, 0.25], [0, -0.25, -0.25], [0, 0.125, -0.375]])
        for nv in (1, 2, 3, 4):
            cs.add(cs.mesh(cube), cs.mesh(flat[:nv], (0.5 + g, 0, 0)), exp, f"cube face / {nv} coplanar vertices gap {g:g}")
            cs.add(cs.mesh(flat[:nv], (0.5 + g, 0, 0)), cs.mesh(cube), exp, f"{nv} coplanar vertices / cube face gap {g:g}")
        # duplicated vertices, and vertices inside the hull and on its faces
        dup = np.concatenate([cube, cube[::2], [[0, 0, 0], [0.25, 0.125, 0.0], [0.5, 0.25, 0.25], [-0.5, 0, 0]]])
        cs.add(cs.mesh(dup), cs.mesh(dup[::-1], (1.0 + g, 0.5, 0.25)), exp, f"duplicated and interior vertices gap {g:g}")
        # primitives through their cores: sphere and capped cylinder (axis z) beside the cube's face
        # (their cores stay apart at gap 0: the swept shapes touch, the value is 0.0 and no collision)
        cs.add(cs.mesh(cube), make_shape(T.SHAPE_SPHERE, (0.75 + g, 0.25, 0), (0.25, 0, 0)), g, f"cube / sphere gap {g:g}")
        cs.add(make_shape(T.SHAPE_CCYLINDER, (0.625 + g, 0, 0.25), (0.5, 0.125, 0)), cs.mesh(cube), g, f"capsule / cube gap {g:g}")
        cs.add(cs.mesh(cube), make_shape(T.SHAPE_BOX, (1.0 + g, 0.5, 0), (1.0, 0.5, 0.25)), exp, f"cube mesh / box gap {g:g}")
    # a rotated cube: edge (along z) against face, gap through the diagonal sqrt(2)/2 (not exactly representable)
    for g in (1.0, 1e-3, 1e-6):
        cs.add(cs.mesh(cube), cs.mesh(cube, (0.5 + 0.5 * s2 + g, 0, 0.25), qz45), g, f"cube face / rotated cube edge gap {g:g}")
    # offsets up to 1e6 and scales 1e-6 .. 1e3 (powers of two keep the coordinates exact)
    for off in (2.0 ** 10, 2.0 ** 20):
        o = np.array([off, -off, off])
        cs.add(cs.mesh(cube, o), cs.mesh(octa, o + [1.25, 0.125, 0], ), 0.25, f"offset {off:g}")
        cs.add(cs.mesh(cube + o), cs.mesh(octa + o, (1.25, 0.125, 0)), 0.25, f"offset {off:g} in the vertices")
    for sc in (2.0 ** -20, 2.0 ** -10, 2.0 ** 10):
        cs.add(cs.mesh(cube * sc), cs.mesh(octa * sc, (1.25 * sc, 0.125 * sc, 0)), 0.25 * sc, f"scale {sc:g}")
        cs.add(cs.mesh(cube * sc), cs.mesh(cube * sc, (1.5 * sc, 1.5 * sc, 1.5 * sc)), 0.5 * np.sqrt(3.0) * sc, f"scale {sc:g} corners")
    # a vertex deep inside, and identical meshes
    cs.add(cs.mesh(cube), cs.mesh([[0.0, 0.0, 0.0]], (0.125, 0.0625, 0)), -OVERLAP, "point inside a cube")
    cs.add(cs.mesh(cube), cs.mesh(cube), -OVERLAP, "identical cubes")
    cs.add(cs.mesh(cube), make_shape(T.SHAPE_SPHERE, (0.125, 0, 0), (0.25, 0, 0)), -0.25 - OVERLAP, "sphere centre inside a cube")
    return cs


def inside_hull(V, p, tol=0.0):
    """p lies in conv(V) (a full-dimensional vertex set), to tol: on the inner side of every hull face's plane."""
    V = np.asarray(V, dtype=np.float64)
    faces, _ = hull_features(V)
    a = V[faces[:, 0]]
    nrm = _cross(V[faces[:, 1]] - a, V[faces[:, 2]] - a)
    nrm /= np.sqrt(_dot(nrm, nrm))[:, None]
    s = nrm @ V.T - _dot(nrm, a)[:, None]                       # [F][nv]: which side the other vertices are on
    side = np.sign(s[np.arange(len(s)), np.argmax(np.abs(s), axis=1)])
    return bool(np.all(side * (nrm @ np.asarray(p, dtype=np.float64) - _dot(nrm, a)) >= -tol))


@functools.lru_cache(maxsize=None)
def gap_scene(seed=42, radius=0.05, length=0.5):
    """(scenario, states [7][2], expected min distance [7]): a one-link chain (revolute about -y, link along x) carrying
    a capped cylinder, and seven convex-mesh obstacles.  Obstacle i is built around configuration q_i: 1e-6 clear of the
    swept cylinder (i even) or 1e-6 into it (i odd; the cores stay apart, so the value is -1e-6); the last one sits on
    the cylinder's axis (cores intersect: -radius - 1e-9).  Expected = the reference over ALL obstacles, per state."""
    rng = np.random.default_rng(seed)
    scn = scenarios.make_pendulum(length=length)
    cap = T.Shape(kind=T.SHAPE_CCYLINDER, anchor=1)
    cap.pose = T.make_pose((0.5 * length, 0.0, 0.0), (np.cos(np.pi / 4), 0.0, np.sin(np.pi / 4), 0.0))   # axis z -> x
    cap.dims[:] = [length, radius, 0.0]
    q = -2.4 + 0.8 * np.arange(7)

    def axis_world(qi):   # the revolute joint turns about -y: x -> (cos q, 0, sin q)
        return np.array([[0.0, 0.0, 0.0], [length * np.cos(qi), 0.0, length * np.sin(qi)]])

    shapes, pool, world = [cap], [], []
    for i, qi in enumerate(q):
        S = axis_world(qi)
        V = scenarios.random_convex_mesh(rng, int(rng.integers(8, 25)), 0.08)
        quat = _rand_quat(rng)
        W0 = V @ quat_rotmat(quat).T
        on_axis = S[0] + rng.uniform(0.6, 1.0) * (S[1] - S[0])
        if i == len(q) - 1:
            c = on_axis
        else:
            u = rng.normal(size=3)
            c0 = on_axis + 0.3 * u / np.linalg.norm(u)
            d, pa, pb = polytope_distance(S, W0 + c0)
            gap = 1e-6 if i % 2 == 0 else -1e-6
            c = c0 - (pb - pa) / d * (d - radius - gap)
        s = T.Shape(kind=T.SHAPE_MESH, anchor=-1)
        s.pose = T.make_pose(tuple(c), quat)
        s.dims[:] = [float(sum(len(v) for v in pool)), float(len(V)), 0.0]
        pool.append(V)
        shapes.append(s)
        world.append(W0 + c)
    scn.shapes = shapes
    scn.mesh_vertices = np.concatenate(pool)
    expect = np.array([min(expected_query(axis_world(qi), W, radius, 0.0) for W in world) for qi in q])
    x = np.zeros((len(q), 2))
    x[:, 0] = q
    return scn, x, expect


@functools.lru_cache(maxsize=None)
def capsule_box_cases(first=7500, last=7600):
    """Capped cylinder / box pairs first..last of the 10 000 random poses of test_gjk_reproduces_the_closed_forms
    (generator seed 123).  Pair 7561 is in it: the query once took its cores, 0.0123 apart, for crossing."""
    from test_oracle_kat import gjk_pair_sets

    A, B = gjk_pair_sets(np.random.default_rng(123), 10000)[("ccyl", "box")]
    cs = Cases()
    for i in range(first, last):
        cs.add_by_reference(A[i], B[i], f"capped cylinder / box pair {i}")
    return cs
