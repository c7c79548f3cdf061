"""The transfers around the launch of the one-shot entry points (reak_amd/csrc/staged_call.h) at the shapes where staging
itself can go wrong: absent optional outputs, zero-sized batches, and the arrays allocated with one element for none.
Every call goes through ctypes on the loaded library with sentinel-filled outputs.  For each entry with optional outputs,
the call with one of them NULL must leave the others bit-equal to those of the full call, at B = 1 and B = 3, on the C1
chain and its planar form; B = 0 answers RKH_OK and writes nothing; the GJK diagnostics run without a vertex pool.  (cap = 0
of the record entries is covered by test_proximity_records_gpu.py and its planar twin.)"""
import ctypes as C

import numpy as np
import pytest

from reak_amd import scenarios
from reak_amd import types as T

pytestmark = pytest.mark.gpu

NO_INDEX = 0xFFFFFFFF
_FILL = {np.dtype(np.float64): -777.0, np.dtype(np.uint32): 0xA5A5A5A5, np.dtype(np.uint8): 0xA5}
_CTYPE = {np.dtype(np.float64): C.c_double, np.dtype(np.uint32): C.c_uint32, np.dtype(np.uint8): C.c_uint8}


def _out(shape, dtype=np.float64):
    """a sentinel-filled output array (of one element at least: B = 0 still hands a valid pointer)"""
    shape = (max(shape[0], 1),) + tuple(shape[1:])
    return np.full(shape, _FILL[np.dtype(dtype)], dtype=dtype)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(_CTYPE[a.dtype]))


def _untouched(a):
    return bool((a == _FILL[a.dtype]).all())


@pytest.fixture(scope="module")
def ctx():
    from reak_amd import lib as L
    return L.Context(0)


@pytest.fixture(scope="module")
def scenes(ctx):
    from reak_amd import lib as L
    c1 = scenarios.make_c1()
    d = c1.dyn  # C1 is planned quasi-statically: its dynamic space is filled in here
    d.steps_per_edge, d.dt = 20, 1e-3
    d.kp, d.kd, d.u_max, d.goal_tol = 50.0, 10.0, 50.0, 1e-3
    for j in range(c1.n_dof):
        d.lower[2 * j], d.upper[2 * j] = -np.pi, np.pi
        d.lower[2 * j + 1], d.upper[2 * j + 1] = -2.0, 2.0
    planar = scenarios.make_c1_planar(dynamics=True)
    return {"c1": L.Scene(ctx, c1), "c1_planar": L.Scene(ctx, planar)}


# ---- the entries: each returns its sentinel-filled outputs and call(outs) -> status, outs[name] = array or None ------------
def _states(B, n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.8, 0.8, size=(max(B, 1), 2 * n)), rng.uniform(-1.0, 1.0, size=(max(B, 1), n))


def _svp_space(n):
    return T.make_svp_space(n, [-2.5] * n, [2.5] * n, 0.06)


def _svp_pairs(B, n, seed):
    rng = np.random.default_rng(seed)
    a, b = np.zeros((max(B, 1), 2 * n)), np.zeros((max(B, 1), 2 * n))
    a[:, 0::2], b[:, 0::2] = rng.uniform(-1.0, 1.0, size=(2, max(B, 1), n))  # both ends at rest
    return a, b


def _state_derivative(sc, B):
    x, u = _states(B, sc.n, 11)
    outs = {"pd": _out((B, sc.D)), "M": _out((B, sc.n, sc.n)), "f": _out((B, sc.n))}
    return outs, lambda o: sc.lib.rkh_state_derivative(sc.h, _p(x), _p(u), B, _p(o["pd"]), _p(o["M"]), _p(o["f"]))


def _propagate(sc, B):
    a, _ = _states(B, sc.n, 12)
    b, _ = _states(B, sc.n, 13)
    dyn = sc.scn.dyn
    outs = {"x_out": _out((B, sc.D)), "steps_free": _out((B,), np.uint32), "record": _out((B, dyn.steps_per_edge + 1, sc.D))}
    return outs, lambda o: sc.lib.rkh_propagate(sc.h, C.byref(dyn), _p(a), _p(b), B, 1.0, _p(o["x_out"]), _p(o["steps_free"]),
                                                _p(o["record"]))


def _svp_reach_time(sc, B):
    sp = _svp_space(sc.n)
    a, b = _svp_pairs(B, sc.n, 14)
    outs = {"time": _out((B,)), "peak": _out((B, sc.n))}
    return outs, lambda o: sc.lib.rkh_svp_reach_time(sc.ctx.h, C.byref(sp), _p(a), _p(b), B, _p(o["time"]), _p(o["peak"]))


def _svp_edge_check(sc, B):
    sp = _svp_space(sc.n)
    a, b = _svp_pairs(B, sc.n, 15)
    outs = {"out": _out((B, sc.D)), "reach_time": _out((B,)), "n_checked": _out((B,), np.uint32), "reached": _out((B,), np.uint8)}
    return outs, lambda o: sc.lib.rkh_svp_edge_check(sc.h, C.byref(sp), _p(a), _p(b), B, None, _p(o["out"]), _p(o["reach_time"]),
                                                     _p(o["n_checked"]), _p(o["reached"]))


_FRAMES = np.array([0, 3, 6], dtype=np.int32)  # the base, a joint's end, the last link's end


def _direct_kinematics(sc, B):
    x, _ = _states(B, sc.n, 16)
    q, qd = np.ascontiguousarray(x[:, :sc.n]), np.ascontiguousarray(x[:, sc.n:])
    F, planar = len(_FRAMES), sc.planar
    outs = {"pos": _out((B, F, 2 if planar else 3)), "rot": _out((B, F, 2 if planar else 4)),
            "vel": _out((B, F, 2 if planar else 3)), "ang_vel": _out((B, F, 1 if planar else 3))}
    fn = sc.lib.rkh_direct_kinematics_2d if planar else sc.lib.rkh_direct_kinematics
    return outs, lambda o: fn(sc.h, _p(q), _p(qd), B, _FRAMES.ctypes.data_as(C.POINTER(C.c_int32)), F, _p(o["pos"]), _p(o["rot"]),
                              _p(o["vel"]), _p(o["ang_vel"]))


def _inverse_kinematics(sc, B):
    n, S = sc.n, 2
    x, _ = _states(B, n, 17)
    fk = sc.direct_kinematics(x[:, :n], [6])  # reachable targets: the last frame at B random joint points
    targets = T.as_array([T.make_pose(fk["pos"][t, 0], fk["rot"][t, 0]) for t in range(max(B, 1))], T.Pose)
    seeds = np.random.default_rng(18).uniform(-0.8, 0.8, size=(max(B, 1), S, n))
    lower, upper, prm = np.full(n, -np.pi), np.full(n, np.pi), T.make_ik_params()
    outs = {"q": _out((B, S, n)), "res_pos": _out((B, S)), "res_rot": _out((B, S)), "iters": _out((B, S), np.uint32),
            "flags": _out((B, S), np.uint32), "best": _out((B,), np.uint32)}
    return outs, lambda o: sc.lib.rkh_inverse_kinematics(sc.h, 6, targets, B, _p(seeds), S, _p(lower), _p(upper), C.byref(prm),
                                                         _p(o["q"]), _p(o["res_pos"]), _p(o["res_rot"]), _p(o["iters"]),
                                                         _p(o["flags"]), _p(o["best"]))


def _diag_sssp(sc, B):
    n = 5  # a ring of five vertices, both directions; search i starts at vertex i % 5
    row_ptr = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
    col = np.array([[(v + 1) % n, (v - 1) % n] for v in range(n)], dtype=np.uint32).reshape(-1)
    w = np.linspace(0.5, 1.4, 2 * n)
    seed_ptr = np.arange(max(B, 1) + 1, dtype=np.uint32)
    seed_v = np.array([i % n for i in range(max(B, 1))], dtype=np.uint32)
    seed_d, marks = np.zeros(max(B, 1)), np.full(max(B, 1), NO_INDEX, dtype=np.uint32)
    outs = {"dist": _out((B, n)), "pred": _out((B, n), np.uint32), "rounds": _out((B,), np.uint32)}
    return outs, lambda o: sc.lib.rkh_diag_sssp(sc.ctx.h, n, _p(row_ptr), _p(col), _p(w), B, _p(seed_ptr), _p(seed_v), _p(seed_d),
                                                _p(marks), _p(o["dist"]), _p(o["pred"]), _p(o["rounds"]))


# name: (the entry, the scenes it runs on, its optional outputs)
ENTRIES = {
    "state_derivative": (_state_derivative, ("c1", "c1_planar"), ("M", "f")),
    "propagate": (_propagate, ("c1", "c1_planar"), ("record",)),
    "svp_reach_time": (_svp_reach_time, ("c1",), ("peak",)),
    "svp_edge_check": (_svp_edge_check, ("c1", "c1_planar"), ("reach_time", "n_checked", "reached")),
    "direct_kinematics": (_direct_kinematics, ("c1", "c1_planar"), ("pos", "rot", "vel", "ang_vel")),
    "inverse_kinematics": (_inverse_kinematics, ("c1",), ("res_pos", "res_rot", "iters", "flags", "best")),
    "diag_sssp": (_diag_sssp, ("c1",), ("dist", "pred", "rounds")),
}
CASES = [(e, s) for e, (_, on, _) in ENTRIES.items() for s in on]


def _run(scenes, entry, scene, B, drop=None):
    outs, call = ENTRIES[entry][0](scenes[scene], B)
    st = call({k: (None if k == drop else v) for k, v in outs.items()})
    assert st == 0, (entry, scene, B, drop, st, scenes[scene].lib.rkh_last_error().decode())
    return outs


@pytest.mark.parametrize("entry,scene", CASES)
@pytest.mark.parametrize("B", [1, 3])
def test_an_absent_optional_output_leaves_the_others_bit_equal(scenes, entry, scene, B):
    full = _run(scenes, entry, scene, B)
    for k, v in full.items():
        assert not _untouched(v), (k, "the full call writes every output")
    for drop in ENTRIES[entry][2]:
        part = _run(scenes, entry, scene, B, drop)
        assert _untouched(part[drop])
        for k, v in part.items():
            if k != drop:
                assert v.tobytes() == full[k].tobytes(), (entry, scene, B, drop, k)


@pytest.mark.parametrize("entry,scene", CASES)
def test_an_empty_batch_is_ok_and_writes_nothing(scenes, entry, scene):
    for k, v in _run(scenes, entry, scene, 0).items():
        assert _untouched(v), (entry, scene, k)


def test_svp_interpolate_without_samples_or_without_reach_time(scenes):
    sc = scenes["c1"]
    n, M = sc.n, 4
    sp = _svp_space(n)
    for B in (1, 3):
        a, b = _svp_pairs(B, n, 19)
        t = np.ascontiguousarray(np.random.default_rng(20).uniform(0.0, 2.0, size=(B, M)))

        def call(m, out, rt):
            st = sc.lib.rkh_svp_interpolate(sc.ctx.h, C.byref(sp), _p(a), _p(b), B, _p(t) if m else None, m, _p(out), _p(rt))
            assert st == 0, (B, m, sc.lib.rkh_last_error().decode())
        out, rt = _out((B, M, 2 * n)), _out((B,))
        call(M, out, rt)
        assert not _untouched(out) and not _untouched(rt)
        out_only, rt_only = _out((B, M, 2 * n)), _out((B,))
        call(M, out_only, None)
        call(0, None, rt_only)
        assert out_only.tobytes() == out.tobytes() and rt_only.tobytes() == rt.tobytes()
    out, rt = _out((0, M, 2 * n)), _out((0,))
    assert sc.lib.rkh_svp_interpolate(sc.ctx.h, C.byref(sp), _p(a), _p(b), 0, _p(t), M, _p(out), _p(rt)) == 0
    assert _untouched(out) and _untouched(rt)


def test_gjk_diagnostics_without_a_vertex_pool(ctx):
    """n_mesh_vertices = 0 (a NULL pool, one element allocated for none): the answers of the pairs without mesh shapes are
    those of the same call with a pool beside them -- one mesh pair behind the others, which reads it."""
    from reak_amd import lib as L

    def shape(kind, pos, dims):
        s = T.Shape(kind=kind, anchor=-1)
        s.pose = T.make_pose(pos)
        s.dims[:] = dims
        return s
    a = [shape(T.SHAPE_SPHERE, (0.0, 0.0, 0.0), [0.2, 0.0, 0.0]), shape(T.SHAPE_BOX, (0.1, 0.0, 0.0), [0.4, 0.4, 0.4])]
    b = [shape(T.SHAPE_BOX, (1.0, 0.3, 0.0), [0.4, 0.6, 0.2]), shape(T.SHAPE_CCYLINDER, (0.0, 1.0, 0.2), [0.5, 0.1, 0.0])]
    pool = scenarios.box_as_mesh([0.4, 0.6, 0.2])
    mesh = shape(T.SHAPE_MESH, (1.0, 0.3, 0.0), [0.0, float(len(pool)), 0.0])
    for fn, keys in ((L.gjk_distance, None), (L.gjk_records, ("dist", "point1", "point2")),
                     (L.gjk_depth_records, ("dist", "point1", "point2", "normal"))):
        bare, pooled = fn(ctx, a, b), fn(ctx, a + [a[0]], b + [mesh], pool)
        for k in keys or (None,):
            x, y = (bare, pooled) if k is None else (bare[k], pooled[k])
            assert np.isfinite(x).all() and x.tobytes() == y[:len(a)].tobytes(), (fn.__name__, k)
        assert fn(ctx, [], []) is not None  # n = 0: RKH_OK
