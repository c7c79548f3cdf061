"""CPU side of path shortcutting.  (1) tests/cpp/path_shortcut_test.cpp -- the pair index and its inverse, the counts, the
allowed rule and the predecessor walk of reak_amd/csrc/path_shortcut.h -- compiled by the host compiler with
AddressSanitizer and UBSan and run directly.  (2) The reference the GPU tests compare with: tests/shortcut_ref.py's
sequential double loop equals a brute force over all subsequences for L <= 10 on random verdicts, and a planted tie
resolves to the lowest predecessor.  (3) The two new kernels spill nothing, use no private segment, and their rows in
profiles/r03_kernel_resources.txt are what the build gives.  No GPU."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import shortcut_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_path_shortcut_header_under_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "path_shortcut_test.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "path_shortcut_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "reak_amd", "csrc"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "path shortcut ok:" in out.stdout


def test_pair_order_of_the_reference():
    assert S.pairs(1, 0) == [] and S.pairs(2, 0) == [(0, 1)]
    assert S.pairs(4, 0) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert S.pairs(4, 2) == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]
    assert S.pairs(4, 1) == [(0, 1), (1, 2), (2, 3)] and S.pairs(4, 9) == S.pairs(4, 0) == S.pairs(4, 3)


def test_dp_is_the_optimum_over_all_subsequences():
    rng = np.random.default_rng(5)
    n_cases = 0
    for L in range(1, 11):
        for max_span in (0, 1, 2, 5, L):
            for p_ok in (0.0, 0.3, 0.7, 1.0):
                pr = S.pairs(L, max_span)
                ok = (rng.uniform(size=len(pr)) < p_ok).astype(np.uint8)
                w = rng.uniform(0.1, 1.0, len(pr))
                keep, cost, n_blocked = S.dp(L, max_span, ok, w)
                bcost, bkeep = S.brute_force(L, max_span, ok, w)
                assert np.float64(cost).view(np.uint64) == np.float64(bcost).view(np.uint64), (L, max_span, p_ok)
                assert keep == bkeep, (L, max_span, p_ok)   # (random weights: no two subsequences tie)
                assert keep[0] == 0 and keep[-1] == L - 1 and all(a < b for a, b in zip(keep[:-1], keep[1:]))
                idx = {p: k for k, p in enumerate(pr)}
                assert n_blocked == sum(1 for u, v in zip(keep[:-1], keep[1:]) if not ok[idx[(u, v)]])
                assert all(v == u + 1 for u, v in zip(keep[:-1], keep[1:]) if not ok[idx[(u, v)]])   # only input hops
                if p_ok == 0.0 or max_span == 1:
                    assert keep == list(range(L))       # nothing but the input
                n_cases += 1
    assert n_cases == 200


def test_the_row_form_of_the_reference_is_the_double_loop():
    rng = np.random.default_rng(8)
    for L in (1, 2, 3, 17, 70):
        for max_span in (0, 1, 2, 5, L):
            n = len(S.pairs(L, max_span))
            for ok, w in (((rng.uniform(size=n) < 0.3), rng.uniform(0.1, 1.0, n)),
                          ((rng.uniform(size=n) < 0.6), 0.25 * rng.integers(1, 8, n))):   # the second: exact ties
                keep, cost, nb = S.dp(L, max_span, ok, w)
                assert S.dp_rows(L, max_span, ok, w) == (keep, cost, nb), (L, max_span)


def planted_tie(L=8):
    """Weights in multiples of 0.25 (every sum exact): vertex 5 is reached at cost 1.5 through 1 (0 -> 1 -> 5), through 2
    (0 -> 2 -> 5) and through 3 (0 -> 3 -> 5); 0 -> 5 itself is blocked.  The lowest predecessor, 1, must win; and the goal
    L - 1 ties between 5 and 6."""
    pr = S.pairs(L, 0)
    ok = np.zeros(len(pr), dtype=np.uint8)
    w = np.full(len(pr), 4.0)
    idx = {p: k for k, p in enumerate(pr)}
    for (i, j), wt in {(0, 1): 0.5, (0, 2): 0.75, (0, 3): 1.0, (1, 5): 1.0, (2, 5): 0.75, (3, 5): 0.5, (5, L - 1): 1.0,
                       (5, 6): 0.25, (6, L - 1): 0.75}.items():
        ok[idx[(i, j)]], w[idx[(i, j)]] = 1, wt
    return ok, w


def test_a_planted_tie_resolves_to_the_lowest_predecessor():
    L = 8
    ok, w = planted_tie(L)
    keep, cost, n_blocked = S.dp(L, 0, ok, w)
    assert (keep, cost, n_blocked) == ([0, 1, 5, L - 1], 2.5, 0)
    assert S.brute_force(L, 0, ok, w) == (2.5, [0, 1, 5, L - 1])


@pytest.fixture(scope="module")
def res():
    import kernel_resources as kr

    from reak_amd import lib

    lib.build()
    return kr.kernel_resources()


def _table(name):
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", name)):
        if line.startswith("#") or line.startswith("kernel") or not line.strip():
            continue
        rows[line[:78].strip()] = [int(x) for x in line[78:].split()]
    return rows


def _figures(d):
    return [d["vgpr_count"], d["agpr_count"], d["vgpr_spill_count"], d["sgpr_count"], d["private_segment_fixed_size"],
            d["group_segment_fixed_size"]]


def test_shortcut_kernels_spill_nothing_and_their_rows_equal_the_build(res):
    table = _table("r03_kernel_resources.txt")
    names = ["rkh::shortcut_pairs_kernel", "rkh::shortcut_dp_kernel"]
    assert sorted(k for k in res if "shortcut" in k) == sorted(names)
    assert not any("sssp" in k for k in names)
    for k in names:
        d = res[k]
        print(k, _figures(d))
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (k, d)
        assert d["agpr_count"] == 0 and d["vgpr_count"] <= 64, (k, d)
        assert table[k][:6] == _figures(d), (k, table[k], d)
    # the search keeps a path's predecessors and the reversed walk in LDS (2 x 1024 words), the published distance and
    # the scratch of the block-wide count: 19 workgroups fit a CU's 160 KiB
    assert 8192 <= res[names[1]]["group_segment_fixed_size"] <= 8192 + 512
    assert res[names[0]]["group_segment_fixed_size"] == 0


def test_the_new_rows_are_appended_to_the_table():
    lines = open(os.path.join(ROOT, "profiles", "r03_kernel_resources.txt")).read().splitlines()
    assert [i for i, ln in enumerate(lines) if "shortcut" in ln] == [len(lines) - 2, len(lines) - 1]
    assert lines[-3].startswith("rkh::roadmap_sssp_kernel<true>")   # the last row of the table as it was
