"""The mirror sweep (reak_amd/csrc/nn_mirror.hip) over the whole range of coordinate bounds its gate admits, [1e-3, 32]:
index AND distance of every query equal the oracle's linear search bit for bit, no tolerance, no query left out.

The sweep is switched on from the hyperbox alone, so it must hold for a box of side 0.002 as for the planner's, and for
a cloud far smaller than the bound that was promised.  The clouds (tests/nn_mirror_ref.py, shared with the band test
tests/test_nn_mirror_band_cpu.py) are the ones where a half-precision format goes wrong: dense clouds whose squared
norms and squared distances lie far below the resolution of a half, clusters around sqrt(D) * bound = 0.125, controls
whose band holds far more rows than a candidate list (the resolve kernel's exact scan), coordinates that are zero or
below the smallest normal half, and the two ends of the gate.  They are random and tie-free, which the tests assert, so
the index is also checked against np.argmin of plain float64 squared distances: the oracle is not the only witness."""
import numpy as np
import pytest

import nn_mirror_ref as ref

pytestmark = pytest.mark.gpu

SWITCH = "RKH_NN_MIRROR_OPEN"
RKH_ERR_UNSUPPORTED = -5


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


_answers = {}


def answer(oracle, name):
    """The cloud of a case and what the sweep must return, computed once: the oracle's (index, distance), with the index
    confirmed by np.argmin on a cloud asserted to be tie-free."""
    if name not in _answers:
        pts, q, bound = ref.cloud(name)
        assert np.all(np.abs(pts) <= bound) and np.all(np.abs(q) <= bound)
        d2 = ref.exact_sq(pts, q)
        ref.assert_tie_free(d2)
        ridx, rdist = oracle.nn1(q, pts)
        assert np.array_equal(ridx, d2.argmin(axis=0))
        for a in (pts, q, ridx, rdist):
            a.setflags(write=False)
        _answers[name] = (pts, q, bound, ridx, rdist)
    return _answers[name]


def check(L, ctx, oracle, name):
    pts, q, bound, ridx, rdist = answer(oracle, name)
    idx, dist = L.nn_mirror_query(ctx, pts, q, bound)
    wrong = np.flatnonzero((idx != ridx) | (dist != rdist))
    assert len(wrong) == 0, f"{name}: {len(wrong)} of {len(q)} queries differ from the linear search, first {wrong[:5]}"
    assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_mirror_sweep_is_bit_exact(L, ctx, oracle, monkeypatch, name):
    monkeypatch.delenv(SWITCH, raising=False)
    if name.startswith("tiny"):  # the cloud is what it claims to be
        pts, q, bound = answer(oracle, name)[:3]
        k = 1 if pts.shape[1] < 12 else 2
        assert np.all(pts[0::3, :k] == 0.0) and np.all(np.abs(pts[1::3, -k:]) <= 6e-5) and np.any(pts[1::3, -k:] != 0.0)
        on_row = (ref.exact_sq(pts, q[::7]).min(axis=0) == 0.0)
        assert np.all(on_row)
    if name == "gate-12d-32":
        assert (answer(oracle, name)[0] ** 2).sum(axis=1).max() > 6000.0  # rows far out: the pad norm must still lose
    check(L, ctx, oracle, name)


@pytest.mark.parametrize("name", ["uniform-2d-2e-3", "cluster-2d-0.05"])
def test_mirror_sweep_is_bit_exact_with_pass_2_over_all_queries(L, ctx, oracle, monkeypatch, name):
    """RKH_NN_MIRROR_OPEN=0 (read at every call of the diagnostic entry): pass 2 without the open lists."""
    monkeypatch.setenv(SWITCH, "0")
    check(L, ctx, oracle, name)


@pytest.mark.parametrize("bound", [np.nextafter(ref.MIN_BOUND, 0.0), np.nextafter(ref.MAX_BOUND, np.inf), 0.0, 1e-4, 33.0])
def test_bounds_outside_the_gate_are_refused(L, ctx, bound):
    rng = np.random.default_rng(0)
    pts, q = rng.uniform(-1e-4, 1e-4, size=(100, 12)), rng.uniform(-1e-4, 1e-4, size=(8, 12))
    with pytest.raises(L.RkhError) as err:
        L.nn_mirror_query(ctx, pts, q, bound)
    assert err.value.status == RKH_ERR_UNSUPPORTED
    L.nn_mirror_query(ctx, pts, q, ref.MIN_BOUND)  # the same call at the gate's end is taken
