"""The device's f-eval (rkh_state_derivative: the kernels of every chain length and joint mix) against the energy
reference of tests/lagrange_ref.py, read from tests/golden/lagrange_feval.npz only: each family once with all its 24
states and once with the first 17 (a ragged last wave).  pd's velocities must be the input bits; M, f and q'' are held
to the derived bounds of lagrange_ref.bounds (1e-12 relative; DESIGN.md "The f-eval is not the Lagrangian field").  The
steer mappings are held bit-identical to this f-eval and to each other elsewhere, which pins them transitively."""
import functools
import os

import numpy as np
import pytest

import lagrange_ref as LR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lagrange_feval.npz")
RAGGED = 17


@functools.lru_cache(maxsize=None)
def golden():
    return LR.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def L():
    from reak_amd import lib

    return lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.Context(0)


@pytest.mark.parametrize("name", LR.FAMILY_NAMES)
def test_device_satisfies_the_energy_relation(L, ctx, name):
    ref = golden()[name]
    assert len(ref["x"]) == LR.N_STATES
    sc = L.Scene(ctx, LR.scene(name))
    runs = [sc.state_derivative(ref["x"][:B], ref["u"][:B]) for B in (LR.N_STATES, RAGGED)]
    sc.close()
    worst = np.zeros(3)
    for (pd, M, f), B in zip(runs, (LR.N_STATES, RAGGED)):
        assert pd.shape[0] == B
        bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
        assert np.array_equal(bits(pd[:, 0::2]), bits(ref["x"][:B, 1::2]))
        for i in range(B):
            r = np.array(LR.ratios(M[i], f[i], pd[i, 1::2], ref, i))
            worst = np.maximum(worst, r)
    print("device %-18s worst error/bound  M %.3g  f %.3g  q'' %.3g" % (name, *worst))
    assert np.all(worst <= 1.0), (name, "error / bound of (M, f, q'')", worst.tolist())
