"""Generates tests/golden/lagrange_feval.npz: per case family of tests/lagrange_ref.py the states x, the drives u and the
energy reference's M, f, q'', kappa_2(M) and G -- plus c and dV/dq, which the bound on f is made of -- as doubles
rounded from the 50-digit values.  Every state must have kappa_2(M) <= 1e6; none is skipped (change a family's seed
instead).  About a minute.  tests/test_lagrange_feval_cpu.py recomputes every fourth state and compares bit for bit.
Run:  python tests/make_lagrange_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lagrange_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "lagrange_feval.npz")

if __name__ == "__main__":
    out = {}
    for name in lagrange_ref.FAMILY_NAMES:
        arrays = lagrange_ref.reference_arrays(name)
        kappa = arrays["kappa"]
        assert kappa.max() <= lagrange_ref.KAPPA_MAX, (name, kappa.max())
        print("%-18s n = %d  kappa_2(M) in [%.3g, %.3g]" % (name, arrays["u"].shape[1], kappa.min(), kappa.max()), flush=True)
        for key in lagrange_ref.GOLDEN_KEYS:
            out[name + "/" + key] = arrays[key]
    np.savez_compressed(GOLDEN, **out)
    largest = max(os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f)) for f in os.listdir(os.path.dirname(GOLDEN))
                  if f != os.path.basename(GOLDEN))
    print("wrote %s: %d bytes (largest other golden: %d)" % (GOLDEN, os.path.getsize(GOLDEN), largest))
    assert os.path.getsize(GOLDEN) <= largest
