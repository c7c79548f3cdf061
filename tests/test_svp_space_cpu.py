"""The order-1 rate-limited joint space with SVP profiles without a GPU: the device header under sanitizers and bit for
bit against the Python twin, the twin's own pins, rkh_svp_in_bounds through the library, the argument rules.

The twin (tests/svp_ref.py) is what the GPU tests compare the device with, so it is pinned first, against things it
shares no code with: the kinematics of its own profiles (ends, rates, the cruise segment) and a grid search over peak
velocities that knows nothing of the closed forms."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import svp_ref as R
from reak_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lcg():
    state = [20261020]

    def uni():
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return float(state[0] >> 11) / 9007199254740992.0
    return uni


def _same_bits(x, y):
    return (math.isnan(x) and math.isnan(y)) or x.hex() == y.hex()


def test_device_header_on_the_host_under_sanitizers_and_against_the_twin(tmp_path):
    """reak_amd/csrc/svp_device.h through the host stand-in: hand-worked cases for every branch of the three closed forms
    and of the bounds rule (tests/cpp/svp_host.cpp lists them), AddressSanitizer + UBSan linked in; then the 400 seeded
    pairs it prints -- reach time, peaks, a point of the profile in both coordinate sets, the bounds verdicts -- against the
    twin, bit for bit."""
    exe = str(tmp_path / "svp_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tests", "cpp", "hip_host"),
                    os.path.join(ROOT, "tests", "cpp", "svp_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "svp host ok:" in out.stdout
    sp = R.Space(3, [-2.0] * 3, [2.0] * 3, 0.05, [1.0, 0.5, 3.0], [1.0, 1.0, 1.5])
    uni = _lcg()
    rng = lambda lo, hi: lo + (hi - lo) * uni()
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("pair ")]
    assert len(lines) == 400
    n_inf = 0
    for e, w in enumerate(lines):
        a, b = [0.0] * 6, [0.0] * 6
        for i in range(3):
            a[2 * i], a[2 * i + 1] = rng(-2, 2), rng(-sp.vm[i], sp.vm[i])
            b[2 * i] = a[2 * i] + rng(-0.05, 0.05) if e % 5 == 0 else rng(-2, 2)
            b[2 * i + 1] = rng(-sp.vm[i], sp.vm[i])
        Tt, peak = R.reach(sp, a, b)
        want = [Tt] + peak
        if Tt < math.inf:
            x = R.point(sp, a, b, peak, Tt, 0.37 * Tt)
            want += x + R.model_units(sp, x)
        else:
            n_inf += 1
        got = [float.fromhex(v) for v in w[2:-2]]
        assert int(w[1]) == e and len(got) == len(want), (e, w)
        assert all(_same_bits(g, x) for g, x in zip(got, want)), (e, got, want)
        assert [int(w[-2]), int(w[-1])] == [int(R.in_bounds(sp, a)), int(R.in_bounds(sp, b))]
    assert 0 < n_inf < 40


@pytest.mark.parametrize("n", [1, 4, 12])
def test_profiles_of_the_twin_are_rate_limited_motions(n):
    """Along every feasible profile, sampled at 200 times: the ends are a and b exactly, |v_i| <= 1.001 vm_i (the solver's
    own guard), the velocity changes by at most the time step and the position by at most 1.001 x the time step (in the
    space's units: rate v / vm), and the cruise segment is consistent to 1e-12: the ramp end positions differ by
    peak / vm x cruise time."""
    sp = R.test_space(n)
    a, b, _ = R.random_pairs(sp, 120, seed=11 + n, special=False)
    n_fin = 0
    for ae, be in zip(a.tolist(), b.tolist()):
        Tt, peak = R.reach(sp, ae, be)
        if not Tt < math.inf:
            continue
        n_fin += 1
        assert R.point(sp, ae, be, peak, Tt, 0.0) == ae and R.point(sp, ae, be, peak, Tt, Tt * (1 + 1e-9) + 1e-12) == be
        step = Tt / 199
        slack = 4e-13 * max(1.0, Tt)   # rounding of the sampled times and of the closed forms (values of order 1..10)
        prev = None
        for k in range(200):
            x = R.point(sp, ae, be, peak, Tt, k * step)
            for i in range(n):
                assert abs(x[2 * i + 1]) <= 1.001 * sp.vm[i]
                if prev is not None:
                    assert abs(x[2 * i + 1] - prev[2 * i + 1]) <= step + slack
                    assert abs(x[2 * i] - prev[2 * i]) <= 1.001 * step + slack
            prev = x
        for i in range(n):
            p0, p1, v0, v1, vp, vm = ae[2 * i], be[2 * i], ae[2 * i + 1], be[2 * i + 1], peak[i], sp.vm[i]
            if R.same_point(p0, p1, v0, v1, vm):
                continue
            d1, cruise, d2 = R.profile_segments(v0, v1, vp, Tt)
            ps = p0 + 0.5 * (v0 + vp) * d1 / vm
            pe = p1 - 0.5 * (vp + v1) * d2 / vm
            assert cruise >= -1e-3 * vm
            # the peak solve's own guards accept a candidate 1e-3 vm off; within them the segment closes to rounding
            assert abs((pe - ps) - vp / vm * cruise) <= 1e-12 * max(1.0, abs(p0), abs(p1), Tt), (ae, be, i)
    assert n_fin >= 100


def _grid_time(dp, v0, v1, vm, vp):
    """Travel time of the ramp / cruise / ramp profile through peak velocity vp, or None where its cruise time is negative
    (or vp cannot cruise at all): ramps at rate 1, positions at rate v / vm."""
    x1 = 0.5 * (v0 + vp) * abs(vp - v0) / vm
    x2 = 0.5 * (vp + v1) * abs(v1 - vp) / vm
    left = dp - x1 - x2
    if vp == 0.0:
        return abs(v0) + abs(v1) if left == 0.0 else None
    cruise = left * vm / vp
    if cruise < 0.0:
        return None
    return abs(vp - v0) + abs(v1 - vp) + cruise


def test_minimum_time_against_a_grid_search_over_peak_velocities():
    """Time optimality of one joint against a search that knows nothing of the closed form: peak velocities on a grid of
    4001 values in [-vm, vm].  The closed form must not exceed the grid minimum (beyond rounding, 1e-12), and must not
    undercut it by more than the grid can explain.

    The margin: the grid point nearest the optimal peak vp* on the side where the cruise time stays >= 0 is at most one
    step h = 2 vm / 4000 away.  t(vp) = |vp - v0| + |v1 - vp| + c(vp) with c = N(vp) / vp, N = vm dp - X(vp), X the two
    ramps' travel: |d/dvp of the ramp times| <= 2, |X'| <= 2 |vp| <= 2 vm, c' = -X' / vp - c / vp, and c <= t.  So within
    that step |t'| <= 2 + (2 vm + t) / (|vp*| - h) =: L and the grid minimum is at most L h above the optimum.  Pairs whose
    optimal peak is within 10 h of zero are left out (L has no bound there)."""
    rng = np.random.default_rng(5)
    worst, n_used = 0.0, 0
    for vm in (1.0, 0.5, 2.0):
        h = 2.0 * vm / 4000
        grid = [-vm + k * h for k in range(4001)]
        grid[4000] = vm
        for _ in range(60):
            dp = float(rng.uniform(-2, 2)) if rng.uniform() < 0.7 else float(rng.uniform(-0.05, 0.05))
            v0, v1 = float(rng.uniform(-vm, vm)), float(rng.uniform(-vm, vm))
            ok, t, vp = R.joint_min_time(0.0, dp, v0, v1, vm)
            assert ok
            if abs(vp) < 10 * h:
                continue
            times = [g for g in (_grid_time(dp, v0, v1, vm, x) for x in grid) if g is not None]
            assert times, (dp, v0, v1, vm)
            tg = min(times)
            L = 2.0 + (2.0 * vm + tg) / (abs(vp) - h)
            assert t <= tg + 1e-12, (dp, v0, v1, vm, t, tg)
            assert tg - t <= L * h, (dp, v0, v1, vm, t, tg, L * h)
            worst, n_used = max(worst, (tg - t) / (L * h)), n_used + 1
    print("grid search: pairs", n_used, "worst (grid - closed form) / margin", worst)
    assert n_used >= 150


def test_asymmetry_infeasibility_and_limits():
    sp = R.Space(1, [-4.0], [4.0], 0.05)
    # moving with the start velocity is quicker than against it
    a, b = [0.0, 0.9], [1.0, 0.0]
    assert R.reach(sp, a, b)[0] < R.reach(sp, b, a)[0] < math.inf
    # a velocity beyond its limit
    assert R.reach(sp, [0.0, 1.5], [1.0, 0.0])[0] == math.inf and R.reach(sp, [0.0, 0.0], [1.0, -1.5])[0] == math.inf
    # the gap: every joint has its own minimum, the common-time solve fails (a seeded search finds one)
    sp4 = R.Space(4, [-2.0] * 4, [2.0] * 4, 0.05)
    a, b, _ = R.random_pairs(sp4, 4000, seed=3, special=False)
    gap = None
    for ae, be in zip(a.tolist(), b.tolist()):
        each = [R.joint_min_time(ae[2 * i], be[2 * i], ae[2 * i + 1], be[2 * i + 1], 1.0) for i in range(4)]
        if all(f for f, _, _ in each) and R.reach(sp4, ae, be)[0] == math.inf:
            gap = (ae, be, max(t for _, t, _ in each))
            break
    assert gap is not None
    print("gap pair", gap)
    # limits of 0 and of 1 are the same space
    s0, s1 = R.Space(2, [-1, -1], [1, 1], 0.1, [0, 0], [0, 0]), R.Space(2, [-1, -1], [1, 1], 0.1, [1, 1], [1, 1])
    assert s0.vm == s1.vm == [1.0, 1.0]


@pytest.fixture(scope="module")
def lib():
    from reak_amd import lib as L

    L.build()
    return L.load()


def _ok(lib, space, pts):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    ok = np.full(len(pts), 7, dtype=np.uint8)
    st = lib.rkh_svp_in_bounds(C.byref(space), T.dptr(pts), len(pts), ok.ctypes.data_as(C.POINTER(C.c_uint8)))
    return st, ok


def test_in_bounds_through_the_library(lib):
    """rkh_svp_in_bounds needs no device: against the twin on seeded points, and the three-point rule at its edges."""
    sp = R.Space(1, [-1.0], [1.0], 0.05)
    pts = [[0.9, 0.5], [0.8, 0.5], [-0.9, 0.5], [0.875, 0.5], [-0.875, -0.5], [0.0, 1.5], [0.0, 1.0], [1.5, 0.0], [1.0, 0.0],
           [-1.0, 0.0], [0.875, -0.5], [0.9, -0.5]]
    st, ok = _ok(lib, sp.c_space(), pts)
    assert st == 0
    # stops at 1.025 | 0.925 | started at -1.025 | stops at 1.0 exactly | its mirror | v beyond vm | v = vm, stops at 0.5 |
    # p outside | p on the upper face | on the lower | moving inwards, started at 1.0 exactly | started at 1.025
    assert ok.tolist() == [0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 1, 0]
    assert ok.tolist() == [int(R.in_bounds(sp, p)) for p in pts]
    for n in (1, 3, 7, 12):
        sp = R.test_space(n, half_width=1.0)
        a, b, _ = R.random_pairs(sp, 300, seed=n)
        a[:, 0::2] *= 1.05   # some points outside the box
        st, ok = _ok(lib, sp.c_space(), a)
        want = [int(R.in_bounds(sp, p)) for p in a.tolist()]
        assert st == 0 and ok.tolist() == want
        assert 0 < sum(want) < len(want)


def test_argument_rules_refused_before_a_launch(lib):
    """Every rule that is checked before a device is touched: the entries look at the space first, then at k, direction
    and the pointers, at the context last, so the rules can be told apart here by the error text."""
    good = R.test_space(3).c_space()
    pts = np.zeros((2, 6))
    ok = np.zeros(2, dtype=np.uint8)
    okp = ok.ctypes.data_as(C.POINTER(C.c_uint8))

    def variant(**kw):
        s = R.test_space(3).c_space()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return s

    bad_spaces = {
        "struct_size": variant(struct_size=C.sizeof(T.SvpSpace) - 8), "n_dof 0": variant(n_dof=0), "n_dof 13": variant(n_dof=13),
        "min_interval 0": variant(min_interval=0.0), "min_interval inf": variant(min_interval=math.inf),
        "min_interval nan": variant(min_interval=math.nan), "lower > upper": variant(lower=(1, 3.0)),
        "negative speed": variant(speed_limits=(0, -1.0)), "nan accel": variant(accel_limits=(2, math.nan)),
        "inf speed": variant(speed_limits=(1, math.inf)),
    }
    idx, dist, t = np.zeros((2, 4), dtype=np.uint32), np.zeros((2, 4)), np.zeros((2, 3))
    out = np.zeros((2, 3, 6))
    calls = {
        "in_bounds": lambda s: lib.rkh_svp_in_bounds(C.byref(s), T.dptr(pts), 2, okp),
        "reach_time": lambda s: lib.rkh_svp_reach_time(None, C.byref(s), T.dptr(pts), T.dptr(pts), 2, T.dptr(dist), None),
        "nearest": lambda s: lib.rkh_svp_nearest(None, C.byref(s), T.dptr(pts), 2, T.dptr(pts), 2, 4, 0, T.u32ptr(idx), T.dptr(dist)),
        "nearest_async": lambda s: lib.rkh_svp_nearest_async(None, C.byref(s), 8, 2, 8, 2, 4, 0, 8, 8),
        "interpolate": lambda s: lib.rkh_svp_interpolate(None, C.byref(s), T.dptr(pts), T.dptr(pts), 2, T.dptr(t), 3, T.dptr(out), None),
    }
    for cname, call in calls.items():
        for sname, s in bad_spaces.items():
            assert call(s) == -1, (cname, sname)
            assert b"ctx" not in lib.rkh_last_error(), (cname, sname)
        # a good space: what is left to refuse is the missing context (in_bounds needs none)
        if cname != "in_bounds":
            assert call(good) == -1 and b"ctx is NULL" in lib.rkh_last_error(), cname
    assert calls["in_bounds"](good) == 0
    # k, direction, pointers
    near = lambda k, d, p=T.dptr(pts): lib.rkh_svp_nearest(None, C.byref(good), p, 2, T.dptr(pts), 2, k, d, T.u32ptr(idx), T.dptr(dist))
    for k, d in ((0, 0), (65, 0), (4, 2), (4, -1)):
        assert near(k, d) == -1 and b"ctx" not in lib.rkh_last_error(), (k, d)
    assert near(4, 0, None) == -1 and b"pointer" in lib.rkh_last_error()
    assert lib.rkh_svp_in_bounds(C.byref(good), None, 2, okp) == -1 and lib.rkh_svp_in_bounds(None, T.dptr(pts), 2, okp) == -1
    assert lib.rkh_svp_reach_time(None, C.byref(good), None, T.dptr(pts), 2, T.dptr(dist), None) == -1 and b"pointer" in lib.rkh_last_error()
    assert lib.rkh_svp_interpolate(None, C.byref(good), T.dptr(pts), T.dptr(pts), 2, None, 3, T.dptr(out), None) == -1
    assert b"pointer" in lib.rkh_last_error()
    assert lib.rkh_svp_edge_check(None, C.byref(good), T.dptr(pts), T.dptr(pts), 2, None, T.dptr(pts), None, None, None) == -1
    # nothing to do is RKH_OK, and needs no device
    assert lib.rkh_svp_in_bounds(C.byref(good), None, 0, None) == 0
    assert lib.rkh_svp_reach_time(None, C.byref(good), None, None, 0, None, None) == 0
    assert lib.rkh_svp_nearest(None, C.byref(good), None, 0, T.dptr(pts), 0, 4, 0, None, None) == 0
    assert lib.rkh_svp_interpolate(None, C.byref(good), None, None, 0, None, 3, None, None) == 0
    # no points: every query is padded
    assert lib.rkh_svp_nearest(None, C.byref(good), None, 0, T.dptr(pts), 2, 4, 0, T.u32ptr(idx), T.dptr(dist)) == 0
    assert (idx == 0xFFFFFFFF).all() and np.isinf(dist).all()


def test_boundary_declares_the_entries_and_keeps_its_abi_number():
    import re

    from reak_amd import lib as L

    hdr = open(os.path.join(ROOT, "include", "rkh.h")).read()
    for name in ("rkh_svp_in_bounds", "rkh_svp_reach_time", "rkh_svp_nearest", "rkh_svp_nearest_async", "rkh_svp_edge_check",
                 "rkh_svp_interpolate"):
        assert re.search(r"rkh_status " + name + r"\(", hdr), name
        assert name in L.EXPORTS
    assert re.search(r"#define RKH_ABI_VERSION 3u\b", hdr) and L.ABI_VERSION == 3 and len(L.abi_sizes()) == 10
    src = '#include <stdio.h>\n#include "rkh_types.h"\nint main(){printf("%zu\\n",sizeof(rkh_svp_space));return 0;}\n'
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")], check=True)
        size = int(subprocess.run([os.path.join(td, "t")], check=True, capture_output=True, text=True).stdout)
    assert size == C.sizeof(T.SvpSpace) == T.make_svp_space(1, [0], [1], 0.1).struct_size
