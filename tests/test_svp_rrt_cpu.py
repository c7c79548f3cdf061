"""The batch RRT over the SVP space without a GPU: the twin's generator against std::mt19937's check value and numpy's
raw draws, the candidate stream's independence of how it is consumed, the twin's loop on C2 with the CPU oracle's distance
as the collision predicate (every way an iteration can end, every way a problem can end, the tree's invariants), the
scalar rules of reak_amd/csrc/svp_rrt_device.h under a host compiler with AddressSanitizer + UBSan, and the binding."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import svp_ref as R
import svp_rrt_ref as RR
from reak_amd import scenarios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def test_generator_is_std_mt19937():
    g = RR.Mt19937()
    y = 0
    for _ in range(10000):
        y = g.next()
    assert y == 4123659995   # the C++ standard's check value for the default seed 5489
    for seed in (0, 1, 5489, 20261021, 0xFFFFFFFF):
        g = RR.Mt19937(seed)
        want = np.random.RandomState(seed).randint(0, 1 << 32, size=1500, dtype=np.uint64)   # raw 32-bit draws
        assert [g.next() for _ in range(1500)] == want.tolist(), seed


def test_candidate_k_depends_only_on_seed_and_k():
    """one go against windows of 1, 7 and 625 draws' worth of candidates: D = 4 draws per candidate, 700 candidates cross
    the generator's 624-word boundary four times"""
    sp = R.Space(2, [-1.0, 0.0], [1.0, 4.0], 0.05, [1.0, 4.0], [2.0, 2.0])
    whole = RR.candidates(sp, RR.Mt19937(7), 700)
    for window in (1, 7, 625):
        rng, got = RR.Mt19937(7), []
        while len(got) < 700:
            got.extend(RR.candidates(sp, rng, min(window, 700 - len(got))))
        assert got == whole, window
    # another seed is another stream; the first candidate is the first D draws in point order
    assert RR.candidates(sp, RR.Mt19937(8), 3) != whole[:3]
    g = RR.Mt19937(7)
    u = [RR.unit(g.next()) for _ in range(4)]
    assert whole[0] == [-1.0 + u[0] * 2.0, -0.5 + u[1] * 1.0, 0.0 + u[2] * 4.0, -2.0 + u[3] * 4.0]


def test_scalar_rules_on_the_host_under_sanitizers_and_against_the_twin(tmp_path):
    """tests/cpp/svp_rrt_host.cpp: the generator's check value through the kernel's three stretches, the draw, the
    coordinate mapping, the steer fraction and the progress rule's strict edges by hand; then its 700 candidates of seed 7
    and their bounds verdicts against the twin, bit for bit.  Nothing is preloaded: the program has its own main."""
    exe = str(tmp_path / "svp_rrt_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tests", "cpp", "hip_host"),
                    os.path.join(ROOT, "tests", "cpp", "svp_rrt_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "svp rrt host ok:" in out.stdout
    sp = R.Space(2, [-1.0, 0.0], [1.0, 4.0], 0.05, [1.0, 4.0], [2.0, 2.0])
    assert sp.vm == [0.5, 2.0]
    want = RR.candidates(sp, RR.Mt19937(7), 700)
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("cand ")]
    assert len(lines) == 700
    n_in = 0
    for k, w in enumerate(lines):
        assert [float.fromhex(v) for v in w[2:6]] == want[k], k
        assert int(w[6]) == int(R.in_bounds(sp, want[k])), k
        n_in += int(w[6])
    assert 0 < n_in < 700
    # the twin's own copies of the rules, at the edges the program works by hand
    assert RR.fraction_of(2.0, 1.0) == 0.5 and RR.fraction_of(0.5, 1.0) == 1.0 and RR.fraction_of(0.0, 1.0) == 1.0
    assert not RR.progress(2.0, 2.0, 0.5, 0.1) and RR.progress(math.nextafter(2.0, 0.0), 2.0, 0.5, 0.1)
    assert not RR.progress(0.1, 2.0, 0.5, 0.1) and RR.progress(math.nextafter(0.1, 1.0), 2.0, 0.5, 0.1)
    assert not RR.progress(math.inf, 2.0, 0.5, 0.1)


# ---- the twin's loop on C2 with the CPU oracle's distance -------------------------------------------------------------------
# (seed, start, goal?, max_vertices, max_iterations, max_edge_time), chosen by running the twin: problem 0 reaches the goal
# from a later vertex, 1 grows to max_vertices, 2 starts in motion and cannot move (max_edge_time below min_interval: no
# point of any edge is tested) -- its candidate 117 is in bounds and out of reach of the start -- and ends on max_iterations
CASES = [(4, "rest", True, 40, 400, 1.0), (2, "rest", False, 12, 400, 1.0), (1, "moving", True, 40, 150, 0.04)]
_TREES = {}


def _c2():
    import plan_svp_rrt as E
    scn = scenarios.make_c2(world_seed=1)
    n, lower, upper, mi, speed, accel = E.c2_space()
    sp = R.Space(n, lower, upper, mi, speed, accel)
    rest = E.to_space(scn.start[0::2]).tolist()
    moving = list(rest)
    for i in range(n):
        moving[2 * i + 1] = (0.7 if i % 2 == 0 else -0.6) * sp.vm[i]
    return scn, sp, {"rest": rest, "moving": moving}, E.to_space(E.GOAL).tolist()


def _trees():
    if not _TREES:
        import oracle_lib
        oracle_lib.build()
        scn, sp, starts, goal = _c2()
        osc = oracle_lib.OracleScene(scn)
        free = lambda x: not (osc.min_distance(np.array([R.model_units(sp, x)]))[0] < 0.0)
        walks = []

        def walk(a, b, f):
            w = R.edge_walk(sp, a, b, f, free)
            walks.append(w[4])
            return w

        _TREES["sp"], _TREES["goal"] = sp, goal
        _TREES["trees"] = [RR.rrt(sp, walk, starts[s], goal if g else None, seed, mv, mi, met)
                           for seed, s, g, mv, mi, met in CASES]
        _TREES["walks"] = walks
    return _TREES


def test_twin_loop_takes_every_branch_and_ends_every_way():
    t = _trees()
    trees = t["trees"]
    print([(tr["why"], len(tr["vertices"]), tr["iterations"], tr["goal_parent"], tr["branches"]) for tr in trees])
    assert [tr["why"] for tr in trees] == ["goal", "max_vertices", "max_iterations"]
    assert trees[0]["goal_parent"] not in (0, RR.NO_INDEX) and trees[0]["goal_parent"] == len(trees[0]["vertices"]) - 1
    assert len(trees[1]["vertices"]) == 12 and trees[1]["goal_parent"] == RR.NO_INDEX
    assert trees[2]["iterations"] == 150 and len(trees[2]["vertices"]) == 1
    for key in ("out_of_bounds", "no_neighbour", "nothing_checked", "no_progress", "committed"):
        assert sum(tr["branches"][key] for tr in trees) >= 1, key
    for tr in trees:
        assert sum(tr["branches"].values()) == tr["iterations"]
    assert {"completed", "collision", "bounds", "zero"} <= set(t["walks"]), set(t["walks"])
    # the solution of problem 0: start ... goal, the duration the sum of the edges' times
    pts, dur = RR.solution(t["sp"], trees[0], t["goal"])
    assert pts[0] == trees[0]["vertices"][0] and pts[-1] == t["goal"] and len(pts) >= 3
    assert math.isfinite(dur) and dur > 0.0
    assert RR.solution(t["sp"], trees[1], t["goal"]) == ([], 0.0)


def test_tree_invariants():
    t = _trees()
    sp = t["sp"]
    for (seed, s, g, mv, mi, met), tr in zip(CASES, t["trees"]):
        V = len(tr["vertices"])
        assert V == len(tr["parent"]) == len(tr["edge_time"]) and 1 <= V <= mv and tr["iterations"] <= mi
        assert tr["parent"][0] == RR.NO_INDEX and tr["edge_time"][0] == 0.0
        for v in range(V):
            assert R.in_bounds(sp, tr["vertices"][v]), (seed, v)
        for v in range(1, V):
            p = tr["parent"][v]
            assert 0 <= p < v, (seed, v, p)   # parents precede children
            et = R.reach(sp, tr["vertices"][p], tr["vertices"][v])[0]
            assert tr["edge_time"][v] == et and math.isfinite(et) and 0.0 < et <= 2.0 * met * (1.0 + 4e-16), (seed, v, et)   # (asked x (met / asked) rounds twice)


def test_binding_mirrors_the_header():
    import ctypes as C

    from reak_amd import lib as L
    from reak_amd import types as T
    src = '#include <stdio.h>\n#include "rkh.h"\nint main(){printf("%zu %zu\\n",sizeof(rkh_svp_rrt_params),sizeof(rkh_svp_rrt_stats));return 0;}\n'
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")], check=True)
        sizes = [int(v) for v in subprocess.run([os.path.join(td, "t")], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [C.sizeof(T.SvpRrtParams), C.sizeof(L.SvpRrtStats)]
    pr = T.make_svp_rrt_params([0.1] * 12, goal=[0.2] * 12, seed=9, max_vertices=7, max_iterations=11, max_edge_time=0.5)
    assert pr.struct_size == sizes[0] and pr.has_goal == 1 and pr.goal[11] == 0.2 and pr.max_edge_time == 0.5
    assert T.make_svp_rrt_params([0.0] * 12).has_goal == 0
    for name in ("rkh_svp_rrt_create_batch", "rkh_svp_rrt_destroy", "rkh_svp_rrt_solve", "rkh_svp_rrt_get_status",
                 "rkh_svp_rrt_get_tree", "rkh_svp_rrt_get_solution", "rkh_diag_svp_rrt_profile"):
        assert name in L.EXPORTS
    L.build()
    lib = L.load()
    assert hasattr(lib, "rkh_svp_rrt_create_batch") and hasattr(L, "SvpRrt")
