"""The k-NN search's launch plan (reak_amd/csrc/knn_plan.h) and the plain reference the GPU tests compare with
(tests/knn_ref.py).  No GPU.

tests/cpp/knn_plan_test.cpp runs the plan over a grid of requests -- grid and subset bounds, the sorts' LDS limits, the
workspace carve, the graph batch's workspace, the guarantee of the exact retry as a predicate of the plan, k outside
[1, 1024] -- compiled by the host compiler with AddressSanitizer and UBSan and run directly.

knn_ref is pinned once against the oracle's linear search (the restated min_dist_linear_search) on tie-free data, where
the order of the result is fully determined: distances, counts and indices bit for bit."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_plan_under_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "knn_plan_test.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "knn_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "reak_amd", "csrc"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
        one = subprocess.run([exe, "3000", "33", "100"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "knn plan ok: 810 requests" in out.stdout
    assert one.returncode == 0 and "m_sub=96 cmax=2048" in one.stdout and "needs_retry=1" in one.stdout, one.stdout


@pytest.mark.parametrize("D,n,B,k,radius", [(3, 1000, 7, 10, np.inf), (12, 2500, 5, 64, np.inf), (1, 300, 4, 5, np.inf),
                                            (7, 900, 6, 20, 2.5), (12, 50, 3, 80, np.inf), (2, 400, 3, 8, 0.4)])
def test_knn_ref_equals_the_oracle_on_tie_free_data(oracle, D, n, B, k, radius):
    rng = np.random.default_rng(1000 + D + n)
    pts = rng.uniform(-3, 3, size=(n, D))
    q = rng.uniform(-3, 3, size=(B, D))
    idx, dist, cnt = knn_ref.knn(q, pts, k, radius)
    for b in range(B):  # tie-free: the premise of comparing indices with the oracle's heap order
        assert np.unique(dist[b, :cnt[b]]).size == cnt[b]
    ridx, rdist, rcnt = oracle.knn(q, pts, k, radius)
    assert np.array_equal(cnt, rcnt)
    assert np.array_equal(dist, rdist)
    assert np.array_equal(idx, ridx)
    if np.isfinite(radius):
        assert (cnt < k).any() and (cnt > 0).any()  # the radius cuts some of these lists


def test_knn_ref_order_ties_and_removed_rows():
    """What the oracle cannot pin: (distance, index) order among equal distances, the strict radius, removed rows."""
    pts = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0], [2.0, 0.0], [0.0, 0.0]])
    q = np.zeros((1, 2))
    idx, dist, cnt = knn_ref.knn(q, pts, 4)
    assert idx[0].tolist() == [5, 0, 1, 2] and dist[0].tolist() == [0.0, 1.0, 1.0, 1.0] and cnt[0] == 4
    idx, dist, cnt = knn_ref.knn(q, pts, 4, removed=[0, 5])
    assert idx[0].tolist() == [1, 2, 3, 4] and cnt[0] == 4
    idx, dist, cnt = knn_ref.knn(q, pts, 4, radius=1.0)  # strictly inside
    assert idx[0].tolist() == [5, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF] and cnt[0] == 1 and np.isinf(dist[0, 1:]).all()
    idx, dist, cnt = knn_ref.knn(q, pts, 3, removed=range(6))
    assert cnt[0] == 0 and (idx == 0xFFFFFFFF).all()
