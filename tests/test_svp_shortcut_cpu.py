"""CPU side of rkh_svp_shortcut_paths.  (1) The twin the GPU tests compare with (tests/svp_shortcut_ref.py): its search
equals a brute force over all subsequences on asymmetric weights with +inf entries and exact ties, a goal out of reach
included.  (2) The header declares the entry, the binding mirrors it, and the ABI is what it was.  (3) The argument rules
that are refused before any launch.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import shortcut_ref as S
import svp_ref as R
import svp_shortcut_ref as SS
from reak_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


def _bits(x):
    return np.float64(x).view(np.uint64)


def _forward_weights(rng, L, max_span, exact):
    """Weights of the candidate pairs from a full asymmetric [L][L] table (w[i][j] != w[j][i]): only the entries i < j are
    ever read.  exact: multiples of 0.25, so that every sum is exact and different subsequences tie."""
    full = 0.25 * rng.integers(1, 6, (L, L)) if exact else rng.uniform(0.1, 1.0, (L, L))
    assert L < 3 or not np.array_equal(full, full.T)
    return np.array([full[i, j] for i, j in S.pairs(L, max_span)], dtype=np.float64)


def test_the_twins_search_is_the_optimum_over_all_subsequences():
    rng = np.random.default_rng(12)
    n_cases = n_inf_goal = n_ties = n_bypassed = 0
    for L in range(1, 10):
        for max_span in (0, 1, 3):
            pr = S.pairs(L, max_span)
            idx = {p: k for k, p in enumerate(pr)}
            for p_ok, p_inf, exact in ((0.3, 0.0, False), (0.7, 0.2, False), (1.0, 0.4, False), (0.6, 0.2, True),
                                       (0.0, 0.1, True)):
                ok = (rng.uniform(size=len(pr)) < p_ok).astype(np.uint8)
                w = _forward_weights(rng, L, max_span, exact)
                planted = rng.uniform(size=len(pr)) < p_inf
                w[planted] = INF
                ok[planted] = 0   # (an infinite pair never has a true verdict)
                keep, t_out, n_blocked = SS.search(L, max_span, ok, w)
                b_time, b_keep = SS.brute_force(L, max_span, ok, w)
                assert _bits(t_out) == _bits(b_time), (L, max_span, p_ok, p_inf)
                assert keep == b_keep, (L, max_span, p_ok, p_inf, exact)
                t_in = SS.time_in(L, max_span, w)
                assert t_out <= t_in
                assert math.isinf(t_in) == any(math.isinf(w[idx[(v, v + 1)]]) for v in range(L - 1))
                if math.isinf(t_out):
                    assert keep == [] and n_blocked == 0
                    n_inf_goal += 1
                else:
                    assert keep[0] == 0 and keep[-1] == L - 1 and all(a < b for a, b in zip(keep[:-1], keep[1:]))
                    hops = list(zip(keep[:-1], keep[1:]))
                    assert all(w[idx[h]] < INF for h in hops)                     # an infinite weight is never taken
                    assert n_blocked == sum(1 for h in hops if not ok[idx[h]])
                    assert all(v == u + 1 for u, v in hops if not ok[idx[(u, v)]])  # blocked hops are input hops
                    n_bypassed += math.isinf(t_in)
                if exact and L >= 4 and max_span != 1 and p_ok > 0:
                    n_ties += 1
                n_cases += 1
    assert n_cases == 9 * 3 * 5
    assert n_inf_goal >= 5 and n_bypassed >= 5 and n_ties >= 5


def test_finite_weights_give_the_quasi_static_reference():
    """without +inf the twin's search is shortcut_ref.dp"""
    rng = np.random.default_rng(3)
    for L in (1, 2, 5, 9):
        for max_span in (0, 1, 3):
            n = len(S.pairs(L, max_span))
            ok, w = (rng.uniform(size=n) < 0.5).astype(np.uint8), 0.25 * rng.integers(1, 8, n)
            assert SS.search(L, max_span, ok, w) == S.dp(L, max_span, ok, w)


def _case(L, finite, ok_pairs, inf_pairs):
    pr = S.pairs(L, 0)
    idx = {p: k for k, p in enumerate(pr)}
    w, ok = np.full(len(pr), 1.0), np.zeros(len(pr), dtype=np.uint8)
    for p, wt in finite.items():
        w[idx[p]] = wt
    for p in ok_pairs:
        ok[idx[p]] = 1
    for p in inf_pairs:
        w[idx[p]] = INF
    return ok, w


def test_an_infinite_consecutive_hop_that_a_shortcut_bypasses():
    """1 -> 2 has no profile; 0 -> 3 and 1 -> 3 pass over vertex 2.  0 -> 1 -> 3 (0.5 + 0.75) ties with 0 -> 3 (1.25):
    the lowest predecessor of 3 wins."""
    ok, w = _case(5, {(0, 1): 0.5, (1, 3): 0.75, (0, 3): 1.25, (3, 4): 1.0}, [(0, 3), (1, 3)], [(1, 2), (2, 3), (2, 4)])
    assert SS.search(5, 0, ok, w) == ([0, 3, 4], 2.25, 1)   # 3 -> 4 is an input hop whose verdict is false
    assert SS.brute_force(5, 0, ok, w) == (2.25, [0, 3, 4])
    assert SS.time_in(5, 0, w) == INF


def test_an_infinite_consecutive_hop_that_no_shortcut_bypasses():
    """every hop over 1 -> 2 is blocked or infinite: the goal is out of reach, and the search says so instead of walking
    predecessors that do not exist"""
    ok, w = _case(4, {}, [(0, 1), (2, 3)], [(1, 2), (0, 3)])
    assert SS.search(4, 0, ok, w) == ([], INF, 0)
    assert SS.brute_force(4, 0, ok, w) == (INF, [])
    # within span 1 there is nothing but the input
    ok1, w1 = S.restrict(4, 1, ok, w)
    assert SS.search(4, 1, ok1, w1) == ([], INF, 0)
    # and a path of one point is its own answer
    assert SS.search(1, 0, [], []) == ([0], 0.0, 0) and SS.time_in(1, 0, []) == 0.0


# ---- the entry's declaration and binding ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from reak_amd import lib as L

    L.build()
    return L.load()


def test_header_binding_and_abi(lib):
    from reak_amd import lib as L

    hdr = open(os.path.join(ROOT, "include", "rkh.h")).read()
    m = re.search(r"rkh_status rkh_svp_shortcut_paths\(([^;]*)\);", hdr)
    assert m, "include/rkh.h does not declare rkh_svp_shortcut_paths"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert args == ["rkh_scene* scene", "const rkh_svp_space* space", "const double* points", "const uint32_t* path_ptr",
                    "uint32_t B", "uint32_t max_span", "uint32_t* keep", "uint32_t* n_keep", "double* time_in",
                    "double* time_out", "uint32_t* n_blocked"]
    diag = open(os.path.join(ROOT, "include", "rkh_diag.h")).read()
    assert "rkh_diag_svp_shortcut_chunked(" in diag and "rkh_diag_svp_shortcut_ms(" in diag
    assert "rkh_diag_svp_shortcut" not in hdr
    for name in ("rkh_svp_shortcut_paths", "rkh_diag_svp_shortcut_chunked", "rkh_diag_svp_shortcut_ms"):
        assert name in L.EXPORTS and hasattr(lib, name)
    dp, u32p, u32, vp = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_uint32, C.c_void_p
    assert lib.rkh_svp_shortcut_paths.argtypes == [vp, C.POINTER(T.SvpSpace), dp, u32p, u32, u32, u32p, u32p, dp, dp, u32p]
    assert hasattr(L.SvpSpace, "shortcut_paths") and hasattr(L.SvpRrt, "shortcut_solutions")
    # no new struct: the ABI number and the handshake's argument list are what they were
    assert "#define RKH_ABI_VERSION 3u" in hdr and lib.rkh_abi_version() == L.ABI_VERSION == 3
    assert len(L.abi_sizes()) == 10 and lib.rkh_abi_check(L.ABI_VERSION, *L.abi_sizes()) == 0


# ---- refusals before any launch ---------------------------------------------------------------------------------------------
def _call(lib, space, pts, path_ptr, B):
    """the entry without a scene: whatever is refused before the scene is looked at is refused here with its own text"""
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    path_ptr = np.ascontiguousarray(path_ptr, dtype=np.uint32)
    total = max(int(path_ptr[-1]), 1)
    keep, n_keep, n_blocked = (np.zeros(total, dtype=np.uint32) for _ in range(3))
    t_in, t_out = np.zeros(total), np.zeros(total)
    st = lib.rkh_svp_shortcut_paths(None, C.byref(space) if space is not None else None, T.dptr(pts), T.u32ptr(path_ptr), B, 0,
                                    T.u32ptr(keep), T.u32ptr(n_keep), T.dptr(t_in), T.dptr(t_out), T.u32ptr(n_blocked))
    return st, lib.rkh_last_error().decode()


def test_arguments_refused_before_any_launch(lib):
    sp = R.test_space(2)
    space = sp.c_space()
    pts = np.zeros((5, 4))
    pts[:, 0] = np.linspace(-1.0, 1.0, 5)
    good_ptr = [0, 2, 5]
    BAD_ARG = -1
    st, msg = _call(lib, None, pts, good_ptr, 2)
    assert st == BAD_ARG and "space is NULL" in msg
    small = sp.c_space()
    small.struct_size -= 8
    st, msg = _call(lib, small, pts, good_ptr, 2)
    assert st == BAD_ARG and "struct_size" in msg
    st, msg = _call(lib, space, pts, [1, 2, 5], 2)
    assert st == BAD_ARG and "ascend from 0" in msg
    st, msg = _call(lib, space, pts, [0, 2, 2], 2)
    assert st == BAD_ARG and "empty" in msg
    nan = pts.copy()
    nan[3, 1] = math.nan
    st, msg = _call(lib, space, nan, good_ptr, 2)
    assert st == BAD_ARG and "not finite" in msg
    inf = pts.copy()
    inf[4, 2] = math.inf
    st, msg = _call(lib, space, inf, good_ptr, 2)
    assert st == BAD_ARG and "not finite" in msg
    keep = np.zeros(5, dtype=np.uint32)
    st = lib.rkh_svp_shortcut_paths(None, C.byref(space), T.dptr(pts), T.u32ptr(np.array(good_ptr, dtype=np.uint32)), 2, 0,
                                    T.u32ptr(keep), None, None, None, None)
    assert st == BAD_ARG and "pointer is NULL" in lib.rkh_last_error().decode()
    # valid arguments without a scene: only the scene is missing
    st, msg = _call(lib, space, pts, good_ptr, 2)
    assert st == BAD_ARG and "scene is NULL" in msg
    # an empty batch is served, whatever the other pointers are
    assert _call(lib, space, pts, [0], 0)[0] == 0
    assert lib.rkh_svp_shortcut_paths(None, C.byref(space), None, None, 0, 0, None, None, None, None, None) == 0
    # ... but not with a space the entries refuse
    assert _call(lib, small, pts, [0], 0)[0] == BAD_ARG
