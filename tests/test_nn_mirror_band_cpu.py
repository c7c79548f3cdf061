"""The band of the mirror sweep (reak_amd/csrc/nn_mirror.hip, error bound) checked where it is stated, without a GPU.

The sweep is exact iff, for every query, the rows with estimate c <= thr include every row at the true nearest
distance: the resolve kernel looks nowhere else.  That is a claim about arithmetic.  Here the operands come from a numpy
model of the documented format (tests/nn_mirror_ref.py), the estimates from exact products and a float64 sum -- an IDEAL
accumulate, so the matrix instruction's own share of the error (15 roundings of 2^-24 on partial sums below S) is added
against the claim on both sides: the smallest estimate is lowered by it before the threshold is taken, the nearest rows'
estimates are raised by it -- and the threshold from mirror_threshold itself: tests/cpp/nn_mirror_band_host.cpp, the
header read by the host compiler, built with AddressSanitizer and UBSan and run directly.

The clouds are those tests/test_nn_mirror_bounds_gpu.py puts to the device.  With the operands unscaled and the threshold
without a term for the split of |x_h|^2 (the format before the prescale) the uniform and cluster cases lose the nearest
row of up to 61 of 64 queries here."""
import os
import subprocess

import numpy as np
import pytest

import nn_mirror_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "cpp", "nn_mirror_band_host.cpp")
    exe = str(tmp_path_factory.mktemp("nn_mirror_band") / "nn_mirror_band_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "reak_amd", "csrc"), src, "-o", exe], check=True)

    def run(mode, rows):
        text = "".join(" ".join(float(v).hex() for v in np.atleast_1d(r)) + "\n" for r in rows)
        out = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        vals = [float.fromhex(t) for t in out.stdout.split()]
        assert len(vals) == len(rows)
        return np.array(vals)

    return run


def test_prescale_brings_every_admitted_bound_into_16_32(host):
    bounds = np.concatenate([[ref.MIN_BOUND, ref.MAX_BOUND, 1.0, np.pi, 0.5, np.nextafter(0.5, 0), 16.0, np.nextafter(16.0, 0)],
                             np.exp(np.random.default_rng(0).uniform(np.log(ref.MIN_BOUND), np.log(ref.MAX_BOUND), size=200))])
    p = host("prescale", bounds)
    assert np.all((p * bounds >= 16.0) & (p * bounds < 32.0))
    assert np.array_equal(np.frexp(p)[0], np.full(len(p), 0.5))  # powers of two
    assert np.array_equal(p, [ref.prescale(b) for b in bounds])  # the model scales as the header does


def test_threshold_edges(host):
    # an empty tree (cmin = +inf) opens everything; a threshold is never below its cmin, and grows with it
    rows = [(np.inf, 1.0, 0.0, 1.0, 0.0, 16.0), (-5.0, 5.0, 0.0, 2.3, 0.0, 16.0), (-4.0, 5.0, 0.0, 2.3, 0.0, 16.0),
            (-5.0, 5.0, 1e-3, 2.3, 2e-3, 16.0)]
    t = host("thr", rows)
    assert np.isinf(t[0]) and t[0] > 0
    assert t[1] > -5.0 and t[2] > t[1] and t[3] > t[1]
    # exact operands (dq = dx = 0): the band is 2 eps, eps = 2^-19 S + 2^-14 + 1e-9 with X widened by 1e-3
    X = 16.0 * (1.0 + 1e-3)
    eps = 2.0 ** -19 * (X * X + 2.0 * X * 2.3) + 2.0 ** -14 + 1e-9
    assert t[1] == pytest.approx(-5.0 + 2.0 * eps, rel=1e-6)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_the_band_holds_every_nearest_row(host, name):
    pts, q, bound = ref.cloud(name)
    D, B = pts.shape[1], len(q)
    assert ref.MIN_BOUND <= bound <= ref.MAX_BOUND and np.all(np.abs(pts) <= bound) and np.all(np.abs(q) <= bound)
    d2 = ref.exact_sq(pts, q)
    ref.assert_tie_free(d2)
    nearest = d2 == d2.min(axis=0)[None, :]  # every row tying for the true nearest distance (one per query here)
    assert np.all(nearest.sum(axis=0) >= 1)

    scale = ref.prescale(bound)
    xh, pieces, dx = ref.row_operands(pts, scale)
    qh, qh2, dq, qn = ref.query_operands(q, scale)
    assert np.all((xh == 0) | (np.abs(xh) >= ref.HALF_MIN_NORMAL)) and np.all((qh == 0) | (np.abs(qh) >= ref.HALF_MIN_NORMAL))
    assert np.all((pieces == 0) | (np.abs(pieces) >= ref.HALF_MIN_NORMAL))  # no operand below the normal range
    c = ref.estimates(xh, pieces, qh)
    assert c.max() < 60000.0  # a pad row loses against every real one
    share = ref.accumulate_share(D, bound, scale, qn)
    cmin = ref.float_down(c.min(axis=0) - share).astype(np.float64)
    X = np.sqrt(float(D)) * bound * scale
    thr = host("thr", [(cmin[b], qh2[b], dq[b], qn[b], dx, X) for b in range(B)])

    worst = np.where(nearest, c + share[None, :], -np.inf).max(axis=0)  # per query, over its nearest rows
    lost = np.flatnonzero(worst > thr)
    assert len(lost) == 0, f"{name}: the band loses the nearest row of {len(lost)} of {B} queries, first {lost[:5]}"
    if name in ref.CONTROLS:  # more rows within the band than a candidate list holds: the resolve kernel's exact scan
        in_band = (c <= thr[None, :]).sum(axis=0)
        assert in_band.min() > ref.CAND_CAP, in_band.min()
