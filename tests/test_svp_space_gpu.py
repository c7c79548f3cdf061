"""The order-1 rate-limited joint space with SVP profiles on the device against the Python twin (tests/svp_ref.py, pinned
on the CPU by tests/test_svp_space_cpu.py): bit-identical times, peaks, points and distances, equal indices, counts and
flags.  The arithmetic is +, -, *, /, sqrt and comparisons in fp64 with contraction off on both sides, so a difference
is a bug (an operation order, a contraction), not a tolerance to widen."""
import math
import os
import sys

import numpy as np
import pytest

import svp_ref as R
from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_INDEX = 0xFFFFFFFF
PASS = 32   # points per live edge and pass of the walk (kSvpPass, svp_space.hip)
SLICE = 256  # points per slice of the nearest sweep at the sizes used here (svp_slice, svp_space.hip: 256 up to 524 288
             # point-query pairs); 5000 points are 20 slices, the last one of 136


@pytest.fixture(scope="module")
def ctx():
    from reak_amd import lib as L
    return L.Context(0)


def _same(got, want):
    """bit-identical arrays of doubles (NaN payloads aside: none are produced)"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---- reach time and interpolate ---------------------------------------------------------------------------------------------
_PAIRS = {}


def _pairs(n):
    """1000 random pairs + the special ones, and the twin's answers, computed once per n"""
    if n not in _PAIRS:
        sp = R.test_space(n)
        a, b, n_random = R.random_pairs(sp, 1000, seed=100 + n)
        twin = [R.reach(sp, x, y) for x, y in zip(a.tolist(), b.tolist())]
        times = np.array([t for t, _ in twin])
        n_fin = int(np.isfinite(times[:n_random]).sum())
        # the condition on the inputs, asserted on the twin: mostly finite, some infinite (one joint alone always has a
        # peak for its own minimum time: at n = 1 only the special pairs are infinite)
        assert n_fin >= 0.9 * n_random and (n_fin < n_random or n == 1), (n, n_fin)
        assert np.isinf(times[n_random + 3:]).all() and (times[n_random:n_random + 3] == 0.0).all()
        _PAIRS[n] = (sp, a, b, times, np.array([p for _, p in twin]))
    return _PAIRS[n]


@pytest.mark.parametrize("n", [1, 2, 3, 6, 7, 12])
def test_reach_time_and_peaks_are_the_twins(ctx, n):
    from reak_amd import lib as L
    sp, a, b, times, peaks = _pairs(n)
    space = L.SvpSpace(sp.c_space(), ctx=ctx)
    total = len(a)
    for B in (1, 63, 64, 65, 1000, total):
        sel = slice(total - B, total) if B < 1000 else slice(0, B)   # small batches hold the special pairs
        t, p = space.reach_time(a[sel], b[sel])
        assert _same(t, times[sel]), (n, B, np.flatnonzero(t != times[sel])[:5])
        assert _same(p, peaks[sel]), (n, B)
    assert _same(space.reach_time(a[:65], b[:65], peaks=False), times[:65])


@pytest.mark.parametrize("n", [1, 2, 3, 6, 7, 12])
def test_interpolate_is_the_twins(ctx, n):
    from reak_amd import lib as L
    sp, a, b, times, _ = _pairs(n)
    space = L.SvpSpace(sp.c_space(), ctx=ctx)
    total = len(a)
    sel = np.concatenate([np.arange(59), np.arange(total - 6, total)])   # 65 pairs, the special ones among them
    fr = np.array([-0.5, 0.0, 1e-9, 0.13, 0.5, 0.77, 0.999999, 1.0, 1.5])
    tf = np.where(np.isfinite(times[sel]), times[sel], 1.0)
    t = fr[None, :] * tf[:, None]
    want = np.array([R.interpolate(sp, x, y, tt)[0] for x, y, tt in zip(a[sel].tolist(), b[sel].tolist(), t.tolist())])
    for B in (1, 63, 64, 65):
        out, rt = space.interpolate(a[sel][:B], b[sel][:B], t[:B])
        assert _same(rt, times[sel][:B]) and _same(out, want[:B]), (n, B)
    out, _ = space.interpolate(a[sel], b[sel], t)
    assert _same(out[:, 0], a[sel]) and _same(out[:, 1], a[sel])           # t <= 0: a
    fin = np.isfinite(times[sel])
    pos = fin & (times[sel] > 0.0)   # (T == 0, the same-point shortcut: every time is "at or before 0", a)
    assert _same(out[pos][:, 7], b[sel][pos]) and _same(out[pos][:, 8], b[sel][pos])   # t >= T: b
    assert _same(out[~fin], np.repeat(a[sel][~fin][:, None], len(fr), axis=1))       # infeasible: a at every time
    # M == 0 and B == 0
    out, rt = space.interpolate(a[sel][:3], b[sel][:3], np.zeros((3, 0)))
    assert out.shape == (3, 0, 2 * n) and _same(rt, times[sel][:3])
    B1000, _ = space.interpolate(a[:1000], b[:1000], (0.37 * np.where(np.isfinite(times[:1000]), times[:1000], 1.0))[:, None])
    want = np.array([R.interpolate(sp, x, y, [0.37 * (tt if tt < math.inf else 1.0)])[0]
                     for x, y, tt in zip(a[:1000].tolist(), b[:1000].tolist(), times[:1000].tolist())])
    assert _same(B1000, want)


# ---- nearest ----------------------------------------------------------------------------------------------------------------
_CLOUD = {}


def _cloud():
    """5000 points of a 3-joint space with duplicates (ties), 33 queries, and the twin's full table of distances in both
    directions; computed once"""
    if not _CLOUD:
        sp = R.test_space(3)
        pts, qs, _ = R.random_pairs(sp, 5000, seed=77, special=False)
        qs = qs[:33].copy()
        pts[1] = pts[0]; pts[64] = pts[0]; pts[300] = pts[10]; pts[4999] = pts[10]   # duplicates, across lanes and slices
        qs[2, 1] = 1.5 * sp.vm[0]    # a query nothing reaches and that reaches nothing: all padding
        qs[1] = pts[70]              # a query on a point: distance 0
        table = np.zeros((2, 33, 5000))
        pl, ql = pts.tolist(), qs.tolist()
        for qi, q in enumerate(ql):
            for pi, p in enumerate(pl):
                table[0, qi, pi] = R.reach(sp, p, q)[0]
                table[1, qi, pi] = R.reach(sp, q, p)[0]
        _CLOUD["v"] = (sp, pts, qs, table)
    return _CLOUD["v"]


def _knn_from_table(row, k):
    order = np.lexsort((np.arange(len(row)), row))
    order = order[np.isfinite(row[order])][:k]
    idx = np.full(k, NO_INDEX, dtype=np.uint32)
    dist = np.full(k, np.inf)
    idx[:len(order)], dist[:len(order)] = order, row[order]
    return idx, dist


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("n_pts", [1, 63, 64, 65, 257, 5000])
def test_nearest_is_the_twins_full_sort(ctx, n_pts, direction):
    """Every (n_pts, B, k): the first n_pts points of the cloud; compared with the sort of the twin's distances by
    (distance, index).  257 and 5000 points cross a slice boundary (SLICE = 256)."""
    from reak_amd import lib as L
    sp, pts, qs, table = _cloud()
    space = L.SvpSpace(sp.c_space(), ctx=ctx)
    assert n_pts <= SLICE or n_pts % SLICE != 0
    for B in (1, 3, 33):
        for k in (1, 5, 64):
            idx, dist = space.nearest(pts[:n_pts], qs[:B], k, direction)
            for qi in range(B):
                wi, wd = _knn_from_table(table[direction, qi, :n_pts], k)
                assert np.array_equal(idx[qi], wi), (n_pts, B, k, qi, idx[qi][:8], wi[:8])
                assert _same(dist[qi], wd), (n_pts, B, k, qi)
    # the conditions on the inputs, on the twin's values: ties, a padded query, k > n_pts
    if n_pts >= 65:
        assert table[direction, 0, 0] == table[direction, 0, 1] == table[direction, 0, 64]
    assert np.isinf(table[direction, 2]).all() and table[direction, 1, 70] == 0.0
    if n_pts == 5000:
        fin = np.isfinite(table[direction, :, :]).sum(axis=1)
        assert (fin[[0, 1] + list(range(3, 33))] >= 64).all() and fin[2] == 0


def test_nearest_matches_the_twins_own_nearest(ctx):
    """svp_ref.nearest (the twin's own sort) on a small case, so that the table above is not the only yardstick"""
    from reak_amd import lib as L
    sp, pts, qs, _ = _cloud()
    space = L.SvpSpace(sp.c_space(), ctx=ctx)
    for direction in (0, 1):
        idx, dist = space.nearest(pts[:65], qs[:3], 64, direction)
        for qi in range(3):
            wi, wd = R.nearest(sp, pts[:65].tolist(), qs[qi].tolist(), 64, direction)
            assert idx[qi].tolist() == wi and _same(dist[qi], np.array(wd))


class _DeviceArray:
    """A numpy array's bytes in device memory, through the HIP runtime the library itself runs on"""
    _hip = None

    def __init__(self, host):
        import ctypes as C
        if _DeviceArray._hip is None:
            _DeviceArray._hip = C.CDLL("libamdhip64.so")
        self.host = np.ascontiguousarray(host)
        self.ptr = C.c_void_p()
        assert self._hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.host.nbytes)) == 0
        assert self._hip.hipMemcpy(self.ptr, C.c_void_p(self.host.ctypes.data), C.c_size_t(self.host.nbytes), 1) == 0   # host to device

    def download(self):
        import ctypes as C
        assert self._hip.hipMemcpy(C.c_void_p(self.host.ctypes.data), self.ptr, C.c_size_t(self.host.nbytes), 2) == 0   # device to host
        return self.host

    def free(self):
        self._hip.hipFree(self.ptr)


def test_nearest_async_is_the_host_form(ctx):
    from reak_amd import lib as L
    sp, pts, qs, _ = _cloud()
    space = L.SvpSpace(sp.c_space(), ctx=ctx)
    k = 16
    want_i, want_d = space.nearest(pts, qs, k, 0)
    d_pts, d_q = _DeviceArray(pts), _DeviceArray(qs)
    d_idx, d_dist = _DeviceArray(np.zeros((33, k), dtype=np.uint32)), _DeviceArray(np.zeros((33, k)))
    for _ in range(2):   # the second launch finds the context's scratch in place
        space.nearest_async(d_pts.ptr, len(pts), d_q.ptr, 33, k, 0, d_idx.ptr, d_dist.ptr)
    ctx.synchronize()
    got_i, got_d = d_idx.download(), d_dist.download()
    for d in (d_pts, d_q, d_idx, d_dist):
        d.free()
    assert np.array_equal(got_i, want_i) and _same(got_d, want_d)


# ---- walk -------------------------------------------------------------------------------------------------------------------
def _limits(n):
    speed = [(1.0, 0.0, 1.5, 2.0, 0.5)[i % 5] for i in range(n)]
    accel = [(2.0, 4.0, 0.0, 3.0)[i % 4] for i in range(n)]
    return speed, accel


SCENES = {
    # name: (scenario, half width of the joint box in model units, seed of the edge generator -- the first seed whose batch
    # of 130 holds every class of edge, found by counting upwards from 1)
    "c2": (lambda: scenarios.make_c2(world_seed=1), 2.5, 1),
    "c1_planar": (scenarios.make_c1_planar, 2.5, 1),
    # (the track scene with its default 40 obstacles keeps them out of the arm's reach: no configuration collides; 150 do)
    "track": (lambda: scenarios.make_crs_a465_track(n_obstacles=150), 2.5, 1),
    "c4_meshes": (lambda: scenarios.make_c4(meshes=True), 2.0, 6),
    "hidim3": (lambda: scenarios.make_hidim(3), 1.0, 1),
}


def _walk_case(name, scene, scn, seed):
    """space, 130 edges with their fractions, and the twin's walk over them with rkh_min_distance as the collision test"""
    n = scn.n_dof
    half = SCENES[name][1]
    speed, accel = _limits(n)
    sp_probe = R.Space(n, [0.0] * n, [1.0] * n, 1.0, speed, accel)
    if name == "hidim3":
        lower, upper = [0.0] * n, [1.0 / s for s in sp_probe.speed]
    else:
        lower, upper = [-half / s for s in sp_probe.speed], [half / s for s in sp_probe.speed]
    # reach times are a few units: 0.06 gives edges from 0 to about 3 x PASS points
    sp = R.Space(n, lower, upper, 0.06, speed, accel)
    a, b, _ = R.random_pairs(sp, 124, seed=seed)          # + 6 special: a == b, same point x 2, beyond the limit x 2, NaN
    B = len(a)
    assert B == 130
    rng = np.random.default_rng(seed + 1000)
    vm = np.array(sp.vm)
    # starts that are themselves acceptable (at rest, inside the box) for most edges, so that walks get under way
    a[:100, 1::2] = 0.0
    a[:100, 0::2] *= 0.8
    b[:60, 1::2] *= 0.3
    b[:60, 0::2] *= 0.8
    a[100, 0::2] = np.array(sp.upper) * 0.999             # leaves the box at once, whatever the scene
    a[100, 1::2] = 0.9 * vm
    fraction = np.array([(1.0, 0.37, 1.0, 0.0, 0.81)[e % 5] for e in range(B)])
    fraction[:5] = (1.0, 0.37, 0.0, 1.0, 1.0)
    has_pairs = scene.num_pairs > 0
    if has_pairs:
        # edges that start in a colliding configuration (stopped at their first point) and edges from a free one to a
        # colliding one (stopped later), whatever the density of the scene's obstacles
        rest = np.zeros((4000, 2 * n))
        rest[:, 0::2] = rng.uniform(0.8 * np.array(sp.lower), 0.8 * np.array(sp.upper), size=(4000, n))
        d = scene.min_distance(np.array([R.model_units(sp, x) for x in rest.tolist()]))
        hit, free = rest[d < 0.0], rest[d > 0.05]
        assert len(hit) >= 4 and len(free) >= 4, (name, len(hit), len(free))
        a[101:105], b[105:109], a[105:109] = hit[:4], hit[:4], free[:4]
        fraction[101:109] = 1.0
    return sp, a, b, fraction, has_pairs


def _twin_walks(sp, scene, a, b, fraction, has_pairs, oracle_scene=None):
    """edge_walk of the twin for every edge; the collision test of all points of all edges in ONE rkh_min_distance call"""
    edges, rows = [], []
    for ae, be, f in zip(a.tolist(), b.tolist(), fraction):
        Tt, peak = R.reach(sp, ae, be)
        pts = []
        if Tt < math.inf:
            pts = [R.point(sp, ae, be, peak, Tt, d) for d in R.walk_times(sp, Tt * f)]
        edges.append((len(rows), len(pts)))
        rows.extend(R.model_units(sp, x) for x in pts)
    dist = scene.min_distance(np.array(rows)) if (rows and has_pairs) else np.full(len(rows), np.inf)
    if oracle_scene is not None and rows:
        # the CPU oracle's distance agrees on which points are free (its arithmetic is the reference's, not bit-identical)
        od = oracle_scene.min_distance(np.array(rows))
        clear = np.abs(dist) > 1e-9
        assert ((od < 0.0) == (dist < 0.0))[clear].all()
    out = []
    for (first, count), ae, be, f in zip(edges, a.tolist(), b.tolist(), fraction):
        it = iter(range(first, first + count))
        out.append(R.edge_walk(sp, ae, be, float(f), lambda x: not (dist[next(it)] < 0.0)))
    return out


_WALKS = {}


def _walk(name, ctx):
    if name not in _WALKS:
        from reak_amd import lib as L
        scn = SCENES[name][0]()
        scene = L.Scene(ctx, scn)
        sp, a, b, fraction, has_pairs = _walk_case(name, scene, scn, SCENES[name][2])
        osc = None
        if name == "c2":
            import oracle_lib
            oracle_lib.build()
            osc = oracle_lib.OracleScene(scn)
        want = {"mixed": _twin_walks(sp, scene, a, b, fraction, has_pairs, osc),
                "null": _twin_walks(sp, scene, a, b, np.ones(len(a)), has_pairs)}
        _WALKS[name] = (scene, sp, a, b, fraction, has_pairs, want)
    return _WALKS[name]


def _census(walks):
    kinds = {}
    for out, Tt, nc, reached, why in walks:
        key = why
        if why == "collision":
            key = "collision_first" if nc == 1 else "collision_later"
        if why == "bounds":
            key = "bounds_first" if nc == 1 else "bounds_later"
        kinds[key] = kinds.get(key, 0) + 1
    return kinds


@pytest.mark.parametrize("name", sorted(SCENES))
def test_edge_walk_is_the_twins_loop(ctx, name):
    """out, n_checked, reached and reach_time of B = 1, 7, 130 edges with per-edge fractions 0, 0.37, 0.81, 1.0 and with
    fraction NULL, against the twin's loop whose predicate is its bounds rule plus rkh_min_distance at the same
    model-unit points (and, on C2, the CPU oracle's verdict on those points)."""
    from reak_amd import lib as L
    scene, sp, a, b, fraction, has_pairs, want = _walk(name, ctx)
    space = L.SvpSpace(sp.c_space(), scene=scene)
    for mode in ("mixed", "null"):
        kinds = _census(want[mode])
        print(name, mode, kinds, "most points", max(w[2] for w in want[mode]))
        # every class of edge is present (asserted on the expected values); a scene without proxy pairs has no collisions
        need = ["completed", "infeasible", "zero", "bounds_first"] + (["collision_later", "collision_first"] if has_pairs else [])
        assert all(kinds.get(kk, 0) >= 1 for kk in need), (name, mode, kinds)
        assert kinds.get("bounds_first", 0) + kinds.get("bounds_later", 0) >= 1
        assert max(w[2] for w in want[mode]) > 2 * PASS or name == "hidim3"   # the pass boundary is crossed, twice
        for B in (1, 7, 130):
            fr = None if mode == "null" else fraction[:B]
            out, rt, nc, reached = space.edge_check(a[:B], b[:B], fr)
            w = want[mode][:B]
            assert _same(rt, np.array([x[1] for x in w])), (name, mode, B)
            assert nc.tolist() == [x[2] for x in w], (name, mode, B)
            assert reached.tolist() == [x[3] for x in w], (name, mode, B)
            ok = [_same(out[e], np.array(w[e][0])) for e in range(B)]
            assert all(ok), (name, mode, B, [e for e in range(B) if not ok[e]][:5])
    # scalar fractions 0 and 1 through the same entry
    out, _, nc, reached = space.edge_check(a[:7], b[:7], 0.0)
    fin = np.isfinite([w[1] for w in want["null"][:7]])
    assert _same(out, a[:7]) and not nc.any() and reached.tolist() == fin.astype(int).tolist()


def test_edge_walk_counts_the_failing_point_not_the_pass(ctx):
    """An edge that fails at its third point reports n_checked == 3 however many points the pass tested: one joint of
    the obstacle-free cube walking out of its box."""
    from reak_amd import lib as L
    scn = scenarios.make_hidim(3)
    scene = L.Scene(ctx, scn)
    sp = R.Space(3, [0.0] * 3, [1.0] * 3, 0.1)
    space = L.SvpSpace(sp.c_space(), scene=scene)
    a = np.array([[0.5, 0.0, 0.5, 0.0, 0.9, 0.0]])
    b = np.array([[0.5, 0.0, 0.5, 0.0, 1.5, 0.0]])   # the target is outside: the walk ends where stopping would overshoot 1
    w = R.edge_walk(sp, a[0].tolist(), b[0].tolist(), 1.0, lambda x: True)
    assert w[4] == "bounds" and 2 <= w[2] <= PASS
    out, rt, nc, reached = space.edge_check(a, b)
    assert nc[0] == w[2] and reached[0] == 0 and _same(out[0], np.array(w[0])) and rt[0] == w[1]


# ---- host-driven RRT --------------------------------------------------------------------------------------------------------
class _TwinSpace:
    """The entries the example's loop uses, from the twin plus rkh_min_distance"""

    def __init__(self, sp, scene):
        self.sp, self.scene = sp, scene

    def in_bounds(self, pts):
        return np.array([R.in_bounds(self.sp, p) for p in np.atleast_2d(pts).tolist()])

    def nearest(self, points, queries, k, direction):
        res = [R.nearest(self.sp, np.atleast_2d(points).tolist(), q, k, direction) for q in np.atleast_2d(queries).tolist()]
        return np.array([r[0] for r in res], dtype=np.uint32), np.array([r[1] for r in res])

    def reach_time(self, a, b, peaks=True):
        return np.array([R.reach(self.sp, x, y)[0] for x, y in zip(np.atleast_2d(a).tolist(), np.atleast_2d(b).tolist())])

    def edge_check(self, a, b, fraction=None):
        a, b = np.atleast_2d(a), np.atleast_2d(b)
        w = _twin_walks(self.sp, self.scene, a, b, np.full(len(a), 1.0 if fraction is None else fraction), True)
        return (np.array([x[0] for x in w]), np.array([x[1] for x in w]), np.array([x[2] for x in w], dtype=np.uint32),
                np.array([x[3] for x in w], dtype=np.uint8))


def test_host_driven_rrt_grows_the_twins_tree(ctx):
    """The loop of examples/plan_svp_rrt.py on C2, to a goal and to 60 vertices: once with the device entries, once with
    the twin plus rkh_min_distance; same parents, same vertices bit for bit."""
    from reak_amd import lib as L
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import plan_svp_rrt as E
    scn = scenarios.make_c2(world_seed=1)
    scene = L.Scene(ctx, scn)
    n, lower, upper, mi, speed, accel = E.c2_space()
    sp = R.Space(n, lower, upper, mi, speed, accel)
    start = E.to_space(scn.start[0::2])
    # a goal the direct edge does not reach (the scenario's own goal is reached at once), and no goal at all: 60 vertices
    for goal, least in ((E.to_space(E.GOAL), 3), (None, 60)):
        dev = E.svp_rrt(L.SvpSpace(sp.c_space(), scene=scene), lower, upper, sp.vm, start, goal, max_vertices=60, seed=4)
        twin = E.svp_rrt(_TwinSpace(sp, scene), lower, upper, sp.vm, start, goal, max_vertices=60, seed=4)
        print("rrt: vertices", len(dev["vertices"]), "iterations", dev["iterations"], "goal from", dev["goal_parent"])
        assert len(twin["vertices"]) >= least and (goal is None) == (twin["goal_parent"] < 0)
        assert dev["iterations"] == twin["iterations"] and dev["goal_parent"] == twin["goal_parent"]
        assert np.array_equal(dev["parent"], twin["parent"]) and _same(dev["vertices"], twin["vertices"])
