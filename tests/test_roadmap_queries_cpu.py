"""CPU side of the roadmap queries.  (1) tests/cpp/roadmap_csr_test.cpp -- the CSR builder, the predecessor walk, the
capacity rule and the goal-side reduction of reak_amd/csrc/roadmap_csr.h -- compiled by the host compiler with
AddressSanitizer and UBSan and run directly.  (2) The argument the device search rests on: the pull iteration (every
round each vertex takes the minimum over its edges of dist[u] + w, strict <) has ONE fixed point, the distances of a
sequential Dijkstra, bit for bit; tests/roadmap_ref.py's Dijkstra is checked against the numpy pull iteration on the
graph families the GPU tests use.  (3) The search kernel's two forms spill nothing and use no private segment, and the
rows of profiles/r03_kernel_resources.txt that existed before are what they were.  No GPU."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import roadmap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_roadmap_csr_under_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "roadmap_csr_test.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "roadmap_csr_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "reak_amd", "csrc"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "roadmap csr ok:" in out.stdout


FAMILIES = R.families()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_dijkstra_is_the_fixed_point_of_the_pull_iteration(name):
    n, eu, ev, ew = FAMILIES[name]
    adj = R.adjacency(n, eu, ev, ew)
    seed_lists = [[(0, 0.0)], [(n - 1, 0.0)], [(n // 2, 0.125), (0, 0.5), (n - 1, 0.0)]]
    for seeds in seed_lists:
        d = np.array(R.dijkstra(adj, seeds))
        p, rounds = R.pull_iteration(n, adj, seeds)
        assert rounds <= n, (name, rounds)   # Bellman-Ford: n - 1 rounds settle, one more sees no change
        assert np.array_equal(d.view(np.uint64), p.view(np.uint64)), name
    if name.startswith("path"):
        assert R.pull_iteration(n, adj, [(0, 0.0)])[1] == n   # the case that needs every round


def test_predecessor_rule_and_goal_side_of_the_reference():
    n, eu, ev, ew, (a, b, lo, hi) = R.planted_tie_graph(200, 6, np.random.default_rng(3))
    adj = R.adjacency(n, eu, ev, ew)
    d, pred = R.vertex_search(adj, a)
    assert d[b] == 0.75 and d[hi] == 0.25 and d[lo] == 0.5 and pred[b] == lo and pred[a] == R.NIL
    d, pred = R.vertex_search(adj, b)
    assert d[a] == 0.75 and pred[a] == lo and R.walk(pred, a) == [b, lo, a]
    # a seed that ties with a graph route: the query point counts as lower than every id
    d, pred = R.search(adj, [(a, 0.0), (b, 0.75)], R.QUERY_POINT)
    assert d[b] == 0.75 and pred[b] == R.QUERY_POINT and pred[a] == R.QUERY_POINT
    assert R.goal_side(d, [(hi, 0.5), (lo, 0.25), (b, 0.0)]) == (lo, 0.75)
    # unreached: +inf and NIL
    n2, u2, v2, w2 = R.two_components(np.random.default_rng(1))
    d, pred = R.vertex_search(R.adjacency(n2, u2, v2, w2), 0)
    assert np.isinf(d[40:]).all() and (pred[40:] == R.NIL).all() and np.isfinite(d[:40]).all()


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


def test_search_kernel_forms_spill_nothing(res):
    table = _table("r03_kernel_resources.txt")
    names = ["rkh::roadmap_sssp_kernel<true>", "rkh::roadmap_sssp_kernel<false>"]
    assert sorted(k for k in res if "sssp" in k) == sorted(names)
    for k in names:
        d = res[k]
        print(k, _figures(d))
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (k, d)
        assert d["agpr_count"] == 0 and d["vgpr_count"] <= 64, (k, d)
        assert table[k][:6] == _figures(d), (k, table[k], d)
    # the LDS form holds 4096 distances and the three round flags; the global form only the flags
    assert 4096 * 8 <= res[names[0]]["group_segment_fixed_size"] <= 4096 * 8 + 64
    assert res[names[1]]["group_segment_fixed_size"] <= 64


def test_no_kernel_that_existed_moved(res):
    """Against the table as committed before the search kernel's rows were appended: every other row still holds."""
    import kernel_resources as kr

    table = {k: v for k, v in _table("r03_kernel_resources.txt").items() if "sssp" not in k}
    built = dict(res)
    built.update(kr.kernel_resources(kr.PRISMATIC_PAIR_SO))
    built = {k[:78]: v for k, v in built.items()}
    moved = {k: (v[:6], _figures(built[k]) if k in built else None) for k, v in table.items()
             if k not in built or v[:6] != _figures(built[k])}
    assert len(table) >= 28 and not moved, moved
