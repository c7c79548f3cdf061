"""Pass 2 of the mirror sweep over the open (row slice, query) pairs only (reak_amd/csrc/nn_mirror.hip, the plan in
nn_mirror.h) against the linear search of the oracle and against the pass over all queries (RKH_NN_MIRROR_OPEN=0,
which rkh_diag_nn_mirror_query reads at every call): index and distance bit for bit, in every case.

A single tree of n rows is swept in gx = min(8192 / gy, slabs / 32, 32) row slices of ceil(slabs / gx) 32-row slabs
(slabs = ceil(n / 32), gy = ceil(B / 384)): two slices need n >= 2017.  The clouds below are built so that the slices a
query is open in are known -- a slice with no open query, queries open in two slices, lists of 0, 1, 32, 33 and 385
entries, lists that overflow -- and what the planted answers must be is asserted on the oracle before the GPU is asked."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCH = "RKH_NN_MIRROR_OPEN"


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


@contextlib.contextmanager
def _switch(value):
    saved = os.environ.pop(SWITCH, None)
    if value is not None:
        os.environ[SWITCH] = value
    try:
        yield
    finally:
        os.environ.pop(SWITCH, None)
        if saved is not None:
            os.environ[SWITCH] = saved


def slices(n, B):
    """(gx, rows per slice) of launch_nn1_mirror for one tree."""
    gy = (B + 383) // 384
    slabs = (n + 31) // 32
    gx = max(1, min(8192 // gy, slabs // 32, 32))
    return gx, 32 * ((slabs + gx - 1) // gx)


def check(L, ctx, oracle, pts, q, bound, ridx=None, rdist=None):
    """Both forms of pass 2 against the oracle; returns the oracle's answer."""
    assert np.all(np.abs(pts) <= bound) and np.all(np.abs(q) <= bound)
    if ridx is None:
        ridx, rdist = oracle.nn1(q, pts)
    with _switch(None):
        idx, dist = L.nn_mirror_query(ctx, pts, q, bound)
    with _switch("0"):
        idx0, dist0 = L.nn_mirror_query(ctx, pts, q, bound)
    assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist)
    assert np.array_equal(idx0, ridx) and np.array_equal(dist0, rdist)
    assert np.array_equal(idx, idx0) and np.array_equal(dist, dist0)
    return ridx, rdist


def test_a_slice_nobody_is_open_in(L, ctx, oracle):
    n, D, B, bound = 2048, 12, 40, 3.0
    assert slices(n, B) == (2, 1024)
    rng = np.random.default_rng(1)
    pts = rng.uniform(-bound, 0.0, size=(n, D))
    pts[1024:] = bound - rng.uniform(0.0, 0.05, size=(n - 1024, D))  # the second slice: a far corner
    q = rng.uniform(-bound, 0.0, size=(B, D))
    ridx, rdist = oracle.nn1(q, pts)
    assert np.all(ridx < 1024)
    far = np.sqrt(((q[:, None, :] - pts[None, 1024:, :]) ** 2).sum(-1)).min(1)
    assert np.all(far > rdist + 3.0)  # squared estimates differ by > 9: far outside every band
    check(L, ctx, oracle, pts, q, bound, ridx, rdist)


def test_queries_open_in_two_slices(L, ctx, oracle):
    n, D, B, bound = 4096, 12, 40, 3.0
    assert slices(n, B) == (4, 1024)
    rng = np.random.default_rng(2)
    pts = rng.uniform(-bound + 0.1, bound - 0.1, size=(n, D))
    pts[3000] = pts[10]                             # a copy two slices later
    pts[1024] = np.nextafter(pts[1023], np.inf)     # one ulp apart across the boundary of slices 0 and 1
    q = rng.uniform(-bound + 0.1, bound - 0.1, size=(B, D))
    q[0] = pts[10]
    q[1] = pts[10] + 1e-9
    q[2] = pts[1024]
    q[3] = pts[1023]
    q[4] = pts[1024] + 1e-9
    q[5] = pts[1023] - 1e-9
    ridx, rdist = oracle.nn1(q, pts)
    assert list(ridx[:6]) == [10, 10, 1024, 1023, 1024, 1023]  # exact ties: the lower index; else the closer vertex
    assert rdist[0] == 0.0 and rdist[2] == 0.0 and rdist[3] == 0.0 and rdist[1] > 0.0
    d4 = np.sqrt(((q[4] - pts[1023]) ** 2).sum())
    assert d4 > rdist[4]  # the closer vertex has the higher index
    check(L, ctx, oracle, pts, q, bound, ridx, rdist)


def test_smallest_estimate_and_nearest_row_in_different_slices(L, ctx, oracle):
    """Two vertices whose distances to the query differ by 1e-9 relative, the closer one in the later slice: in half
    precision either may have the smaller estimate, both lie within the band."""
    n, D, B, bound = 4096, 12, 16, 3.0
    assert slices(n, B) == (4, 1024)
    rng = np.random.default_rng(3)
    pts = rng.uniform(-bound, bound, size=(n, D))
    q = rng.uniform(-2.0, 2.0, size=(B, D))
    r = 0.4
    for b in range(B):
        u, v = rng.normal(size=D), rng.normal(size=D)
        pts[100 + b] = q[b] + r * u / np.linalg.norm(u)                   # slice 0
        pts[3500 + b] = q[b] + r * (1.0 - 1e-9) * v / np.linalg.norm(v)   # slice 3, closer
    ridx, rdist = oracle.nn1(q, pts)
    assert np.array_equal(ridx, 3500 + np.arange(B))
    d_first = np.sqrt(((q - pts[100:100 + B]) ** 2).sum(-1))
    assert np.all(d_first > rdist) and np.all(d_first < rdist * (1.0 + 1e-8))
    check(L, ctx, oracle, pts, q, bound, ridx, rdist)


def test_coincident_vertices_over_two_slices_overflow_the_list(L, ctx, oracle):
    n, D, B, bound = 4096, 12, 8, 3.0
    assert slices(n, B) == (4, 1024)
    rng = np.random.default_rng(4)
    pts = rng.uniform(-bound, bound, size=(n, D))
    p = rng.uniform(-1.0, 1.0, size=D)
    pts[1000:1020] = p   # 20 in slice 0
    pts[1024:1044] = p   # 20 in slice 1: 40 rows within every band, more than the 32 a list holds
    q = rng.uniform(-bound, bound, size=(B, D))
    q[0] = p
    q[1] = p + 1e-9
    q[2] = p - 1e-9
    ridx, rdist = oracle.nn1(q, pts)
    assert list(ridx[:3]) == [1000, 1000, 1000] and rdist[0] == 0.0
    check(L, ctx, oracle, pts, q, bound, ridx, rdist)


@pytest.mark.parametrize("B,counts", [(385, (0, 320, 32, 33)), (777, (385, 1, 32, 359))])
def test_list_lengths_around_a_group(L, ctx, oracle, B, counts):
    """Rows in four clusters, one per slice, far apart; every query sits in one cluster and is open in that slice alone,
    so the slices' lists have the planted lengths: none, one entry, exactly one group, one group and one entry, a full
    block and one entry.  Queries are shuffled: a list's entries are not consecutive queries."""
    n, D, bound = 5000, 12, 3.0
    gx, rows = slices(n, B)
    assert (gx, rows) == (4, 1280) and sum(counts) == B
    rng = np.random.default_rng(5 + B)
    centre = np.array([[-2.0] * D, [2.0] * D, [-2.0, 2.0] * (D // 2), [2.0, -2.0] * (D // 2)])
    of_row = np.minimum(np.arange(n) // rows, 3)
    pts = centre[of_row] + rng.uniform(-0.5, 0.5, size=(n, D))
    of_q = rng.permutation(np.repeat(np.arange(4), counts))
    q = centre[of_q] + rng.uniform(-0.5, 0.5, size=(B, D))
    ridx, rdist = oracle.nn1(q, pts)
    assert np.array_equal(np.minimum(ridx // rows, 3), of_q)
    assert rdist.max() < 2.0
    for s in range(4):  # two centres differ by 4 in at least six coordinates: other clusters' rows are 3 sqrt(6) away
        other = q[of_q != s]
        if len(other):
            assert np.sqrt(((other[:, None, :] - pts[None, of_row == s][:, ::16, :]) ** 2).sum(-1)).min() > 7.0
    check(L, ctx, oracle, pts, q, bound, ridx, rdist)


def test_short_last_slice_with_a_partial_last_slab(L, ctx, oracle):
    n, D, B, bound = 2017 + 37, 12, 40, 3.0
    assert slices(n, B) == (2, 33 * 32)  # slabs: 33 + 32, the last one holds 6 rows
    rng = np.random.default_rng(6)
    pts = rng.uniform(-bound + 0.01, bound - 0.01, size=(n, D))
    q = rng.uniform(-bound, bound, size=(B, D))
    q[:6] = pts[n - 6:] + 1e-9   # answers in the partial slab
    q[6] = pts[1055]
    q[7] = pts[1056]             # the two sides of the slice boundary
    ridx, rdist = oracle.nn1(q, pts)
    assert list(ridx[:8]) == list(range(n - 6, n)) + [1055, 1056]
    check(L, ctx, oracle, pts, q, bound, ridx, rdist)


def test_dense_low_dimensional_cloud(L, ctx, oracle):
    """D = 2, 100 000 rows within 0.5: many rows lie within a query's band, most of the 32 slices are open and lists
    overflow into the resolve kernel's exact scan."""
    n, D, B, bound = 100000, 2, 64, 0.5
    assert slices(n, B)[0] == 32
    rng = np.random.default_rng(7)
    pts = rng.uniform(-bound, bound, size=(n, D))
    q = rng.uniform(-bound, bound, size=(B, D))
    q[::8] = pts[rng.integers(0, n, size=len(q[::8]))]
    check(L, ctx, oracle, pts, q, bound)


@pytest.mark.parametrize("n", [1, 33])
def test_single_slice(L, ctx, oracle, n):
    D, B, bound = 12, 5, 3.0
    assert slices(n, B)[0] == 1
    rng = np.random.default_rng(8 + n)
    pts = rng.uniform(-bound, bound, size=(n, D))
    q = rng.uniform(-bound, bound, size=(B, D))
    q[0] = pts[n - 1]
    ridx, rdist = check(L, ctx, oracle, pts, q, bound)
    assert ridx[0] == n - 1 and rdist[0] == 0.0
