"""The backward walk and the batch bidirectional RRT over the SVP space without a GPU: the twin of the backward walk
(tests/svp_back_ref.py) against first principles, the per-row rules of reak_amd/csrc/svp_walk_rules.h under a host compiler
with AddressSanitizer + UBSan against the twins, the twin loop (tests/svp_birrt_ref.py) on the 36 shared C2 problems with
the CPU oracle's distance as the collision predicate, the invariants of its trees and solutions, and the binding."""
import math
import os
import subprocess

import numpy as np
import pytest

import svp_back_ref as RB
import svp_birrt_ref as BR
import svp_ref as R
import svp_rrt_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = RR.NO_INDEX
FREE = lambda x: True


def _open_space(n, min_interval=0.05):
    """mixed limits, a box nothing leaves"""
    sp = R.test_space(n, min_interval)
    return R.Space(n, [-1e9] * n, [1e9] * n, min_interval, sp.speed, sp.accel)


# ---- the twin of the backward walk against first principles ------------------------------------------------------------------
def test_backward_walk_returns_the_profiles_point_at_the_remaining_time():
    sp = _open_space(4)
    a, b, _ = R.random_pairs(R.test_space(4), 60, seed=5)
    rng = np.random.default_rng(6)
    n_finite = n_inf = 0
    for e in range(len(a)):
        ae, be = a[e].tolist(), b[e].tolist()
        T, peak = R.reach(sp, ae, be)
        if not (T < math.inf):
            out, Tw, nc, reached, why = RB.edge_walk_back(sp, ae, be, 0.5, FREE)
            assert why == "infeasible" and nc == 0 and reached == 0 and Tw == math.inf
            assert out == be or (e == len(a) - 1 and math.isnan(ae[0]))   # an infinite pair returns b, nothing tested
            n_inf += 1
            continue
        if any(abs(pk) > vm for pk, vm in zip(peak, sp.vm)):
            continue   # (a peak within the solver's 1.001 vm guard but beyond vm: the bounds rule stops that walk)
        n_finite += 1
        for f in (1.0, 0.0, float(rng.uniform(0.01, 0.99))):
            out, Tw, nc, reached, _ = RB.edge_walk_back(sp, ae, be, f, FREE)
            assert Tw == T and reached == 1
            if f == 1.0:
                assert out == ae
            elif f == 0.0:
                assert out == be and nc == 0
            else:
                assert out == R.point(sp, ae, be, peak, T, T * (1.0 - f))
            # the count by repeated subtraction
            k, d = 0, T - sp.min_interval
            while d > T * (1.0 - f):
                k, d = k + 1, d - sp.min_interval
            assert nc == k
    assert n_finite >= 40 and n_inf >= 3


def test_backward_walk_counts_at_the_edges_of_min_interval():
    """one joint, unit limits, rest to rest over a distance that takes exactly T = 2 + x: T an exact multiple of
    min_interval tests T / min_interval - 1 points (0 itself is not above dt = 0), T below min_interval tests none"""
    sp = R.Space(1, [-1e9], [1e9], 0.25)
    T, _ = R.reach(sp, [0.0, 0.0], [2.0, 0.0])   # ramp up 1, cruise 1, ramp down 1
    assert T == 3.0
    out, _, nc, reached, why = RB.edge_walk_back(sp, [0.0, 0.0], [2.0, 0.0], 1.0, FREE)
    assert RB.back_times(sp, T, 0.0) == [2.75 - 0.25 * k for k in range(11)] and nc == 11 and reached == 1 and why == "completed"
    assert out == [0.0, 0.0]
    # half of it: the times above 1.5 -- 1.5 itself is not tested (strict)
    assert RB.back_times(sp, T, T * (1.0 - 0.5)) == [2.75, 2.5, 2.25, 2.0, 1.75]
    # T below min_interval: d = T - min_interval < 0 = dt
    Ts, _ = R.reach(sp, [0.0, 0.0], [0.01, 0.0])
    assert 0.0 < Ts < 0.25
    out, _, nc, reached, why = RB.edge_walk_back(sp, [0.0, 0.0], [0.01, 0.0], 1.0, FREE)
    assert (nc, reached, why, out) == (0, 1, "zero", [0.0, 0.0])
    # a predicate that fails at the third point from the end keeps the second
    seen = []
    def third(x):
        seen.append(x)
        return len(seen) < 3
    out, _, nc, reached, why = RB.edge_walk_back(sp, [0.0, 0.0], [2.0, 0.0], 1.0, third)
    assert (nc, reached, why) == (3, 0, "collision") and out == seen[1]
    # and at the first: b
    out, _, nc, reached, _ = RB.edge_walk_back(sp, [0.0, 0.0], [2.0, 0.0], 1.0, lambda x: False)
    assert (nc, reached, out) == (1, 0, [2.0, 0.0])


# ---- svp_walk_rules.h under a host compiler ------------------------------------------------------------------------------------
def _rows_for_the_host_program(sp):
    """seeded pairs with fractions, and two edges cut to 33 and to 65 points: a pass boundary (32, 64) inside the walk"""
    a, b, _ = R.random_pairs(sp, 40, seed=17)
    rng = np.random.default_rng(18)
    rows = []
    for e in range(len(a)):
        f = (1.0, 0.0, 1.0)[e % 3] if e % 4 == 0 else float(rng.uniform(0.05, 0.95))
        rows.append((a[e].tolist(), b[e].tolist(), f))
    long_ = [(r[0], r[1]) for r in rows if 70.0 * sp.min_interval < R.reach(sp, r[0], r[1])[0] < math.inf
             and R.edge_walk(sp, r[0], r[1], 1.0, FREE)[3]]   # the whole profile in bounds: both walks cross their passes
    assert len(long_) >= 2
    for (ae, be), k in zip(long_[:2], (33, 65)):
        T = R.reach(sp, ae, be)[0]
        rows.append((ae, be, ((k + 0.5) * sp.min_interval) / T))
    return rows


def test_walk_rules_on_the_host_under_sanitizers_and_against_the_twins(tmp_path):
    """tests/cpp/svp_walk_dir_host.cpp walks each row in both directions the staged way (passes of 32 points) with the
    bounds rule as its only test; its tested times, counts and returned points are the twins', bit for bit.  Nothing is
    preloaded: the program has its own main."""
    exe = str(tmp_path / "svp_walk_dir_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tests", "cpp", "hip_host"),
                    os.path.join(ROOT, "tests", "cpp", "svp_walk_dir_host.cpp"), "-o", exe], check=True)
    sp = R.test_space(3, 0.05, half_width=2.0)
    rows = _rows_for_the_host_program(sp)
    hx = lambda v: float(v).hex()
    text = ["%d %s" % (sp.n, hx(sp.min_interval))]
    text += [" ".join(hx(v) for v in (sp.lower[i], sp.upper[i], sp.speed[i], sp.accel[i])) for i in range(sp.n)]
    text.append(str(len(rows)))
    text += [" ".join(hx(v) for v in ae + be + [f]) for ae, be, f in rows]
    out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "svp walk dir host ok: %d rows" % len(rows) in out.stdout
    # parse: walk / pass* / out
    got, cur = [], None
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0] == "walk":
            cur = {"row": int(w[1]), "back": int(w[2]), "T": float.fromhex(w[4]), "K": int(w[6]), "passes": []}
            got.append(cur)
        elif w and w[0] == "pass":
            assert int(w[1]) == len(cur["passes"])
            cur["passes"].append([float.fromhex(v) for v in w[2:]])
        elif w and w[0] == "out":
            cur["nc"], cur["reached"], cur["out"] = int(w[1]), int(w[2]), [float.fromhex(v) for v in w[3:]]
    assert len(got) == 2 * len(rows)
    counts = {0: set(), 1: set()}
    whys = {0: set(), 1: set()}
    same = lambda x, y: len(x) == len(y) and all((p == q) or (p != p and q != q) for p, q in zip(x, y))
    for g in got:
        ae, be, f = rows[g["row"]]
        back = g["back"]
        want = RB.walk_dir(sp, ae, be, f, back, FREE)
        whys[back].add(want[4])
        assert g["T"] == want[1] and g["nc"] == want[2] and g["reached"] == want[3], (g["row"], back, g, want)
        assert same(g["out"], want[0]), (g["row"], back)
        if want[1] < math.inf:
            times = RB.times_dir(sp, want[1], f, back)
            assert g["K"] == len(times)
            tested = [t for p in g["passes"] for t in p]
            assert tested == times[:g["nc"]], (g["row"], back)    # bit for bit: floats compare by value, none is NaN
            assert all(len(p) == RB.PASS for p in g["passes"][:-1]) and (not g["passes"] or 1 <= len(g["passes"][-1]) <= RB.PASS)
            counts[back].add(len(times))
    for back in (0, 1):
        assert {33, 65} <= counts[back], sorted(counts[back])
        assert {"infeasible", "completed", "bounds", "zero"} <= whys[back], whys[back]


# ---- the twin loop on the shared C2 inputs with the CPU oracle's distance -----------------------------------------------------
_C2 = {}


def _c2():
    if not _C2:
        import oracle_lib
        oracle_lib.build()
        scn, sp, probs = BR.c2_inputs()
        osc = oracle_lib.OracleScene(scn)
        free = lambda x: not (osc.min_distance(np.array([R.model_units(sp, x)]))[0] < 0.0)
        walk = lambda a, b, f: R.edge_walk(sp, a, b, f, free)
        walk_back = lambda a, b, f: RB.edge_walk_back(sp, a, b, f, free)
        _C2["v"] = (sp, probs, [BR.run(sp, walk, walk_back, p) for p in probs])
    return _C2["v"]


def test_twin_loop_on_the_shared_c2_inputs_takes_every_branch_on_both_sides():
    sp, probs, want = _c2()
    for p, t in zip(probs, want):
        print(p["name"], p["seed"], t["why"], len(t["V"][0]), len(t["V"][1]), t["iterations"], t["join"], t["br"])
    BR.check_c2_conditions(want)
    by = lambda name: {p["seed"]: t for p, t in zip(probs, want) if p["name"] == name}
    # the outcomes recorded with the inputs
    assert all(t["why"] == "joined" for t in by("rest").values())
    assert {s for s, t in by("moving").items() if t["why"] == "joined"} == {1, 3, 6, 9, 11}
    assert {s for s, t in by("moving").items() if t["why"] == "max_vertices"} == {2, 4, 5, 8, 10, 12}
    assert by("moving")[7]["why"] == "max_iterations"
    for t in by("tiny").values():   # max_edge_time below min_interval: nothing can be tested, nothing moves
        assert t["why"] == "max_iterations" and len(t["V"][0]) == len(t["V"][1]) == 1 and t["iterations"] == 150
    assert sum(t["br"][0]["no_neighbour"] for t in by("tiny").values()) >= 1   # a candidate no vertex of tree 0 reaches
    for t in want:
        assert sum(sum(b.values()) for b in t["br"]) == t["half_steps"] + sum(b["out_of_bounds"] for b in t["br"])


def test_tree_and_solution_invariants_of_the_twin():
    sp, probs, want = _c2()
    n_solutions = 0
    for p, t in zip(probs, want):
        for side in (0, 1):
            V, P, E = t["V"][side], t["P"][side], t["E"][side]
            assert len(V) == len(P) == len(E) and 1 <= len(V) <= p["max_vertices"]
            assert P[0] == NO and E[0] == 0.0 and V[0] == (p["start"] if side == 0 else p["goal"])
            for v in range(len(V)):
                assert R.in_bounds(sp, V[v]), (p["name"], p["seed"], side, v)
            for v in range(1, len(V)):
                assert 0 <= P[v] < v   # parents precede children
                et = R.reach(sp, V[P[v]], V[v])[0] if side == 0 else R.reach(sp, V[v], V[P[v]])[0]
                assert E[v] == et and math.isfinite(et) and et > 0.0, (p["name"], p["seed"], side, v)
        assert t["iterations"] <= p["max_iterations"]
        pts, dur = BR.solution(t)
        if t["join"] is None:
            assert (pts, dur) == ([], 0.0)
            continue
        n_solutions += 1
        assert pts[0] == p["start"] and pts[-1] == p["goal"] and len(pts) >= 2
        hops = [R.reach(sp, pts[k], pts[k + 1])[0] for k in range(len(pts) - 1)]
        assert all(math.isfinite(h) for h in hops)    # every hop runs towards the goal
        total = 0.0
        for h in hops:   # the stored times are the hops' reach times, so the stated sum is this sum
            total += h
        assert dur == total
        j0, j1 = t["join"]
        assert t["join_time"] == R.reach(sp, t["V"][0][j0], t["V"][1][j1])[0]
    assert n_solutions == 17


# ---- the kernels' resources and the binding -----------------------------------------------------------------------------------
WALK_KERNELS = ["rkh::rl1dir_walk_solve_kernel", "rkh::rl1dir_walk_points_kernel", "rkh::rl1dir_walk_scan_kernel"]
PLANNER_KERNELS = ["rkh::rl1bi_init_kernel", "rkh::rl1bi_sample_kernel", "rkh::rl1bi_nearest_kernel", "rkh::rl1bi_steer_kernel",
                   "rkh::rl1bi_commit_kernel"]
RESERVED = ("svp_", "rl1rrt_", "nn1_", "propagate_pair", "propagate_kernel<6", "edge_points_kernel<6", "edge_check_kernel")


def _table(name):
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", name)):
        if line.startswith("#") or line.startswith("kernel") or not line.strip():
            continue
        rows[line[:78].strip()] = [int(x) for x in line[78:].split()]
    return rows


def test_new_kernels_exist_match_their_table_and_spill_nothing():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    from reak_amd import lib
    lib.build()
    res = kr.kernel_resources()
    table = _table("r25_svp_birrt_kernel_resources.txt")
    built = {k for k in res if "rl1bi_" in k or "rl1dir_" in k}
    assert built == set(WALK_KERNELS + PLANNER_KERNELS) == set(table), built ^ set(table)
    for k in sorted(built):
        d = res[k]
        print(k, "vgpr", d["vgpr_count"], "sgpr", d["sgpr_count"], "lds", d["group_segment_fixed_size"])
        assert not [s for s in RESERVED if s in k], k
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (k, d)
        assert d["private_segment_fixed_size"] == 0, (k, d)
        assert d["vgpr_count"] <= 128 and d["agpr_count"] == 0, (k, d)   # four waves per SIMD at the least
        assert d["max_flat_workgroup_size"] == 256, (k, d)
        assert table[k][:6] == [d["vgpr_count"], d["agpr_count"], d["vgpr_spill_count"], d["sgpr_count"],
                                d["private_segment_fixed_size"], d["group_segment_fixed_size"]], (k, table[k], d)
    # the kernels with `svp_` in their name are still svp_space.hip's seven, the RRT's still its six
    assert len([k for k in res if "svp_" in k]) == 7 and len([k for k in res if "rl1rrt_" in k]) == 6


def test_binding_lists_the_new_entries():
    from reak_amd import lib as L
    names = ("rkh_svp_edge_check_back", "rkh_diag_svp_edge_check_dir", "rkh_svp_birrt_create_batch", "rkh_svp_birrt_destroy",
             "rkh_svp_birrt_solve", "rkh_svp_birrt_get_status", "rkh_svp_birrt_get_tree", "rkh_svp_birrt_get_solution",
             "rkh_diag_svp_birrt_profile")
    L.build()
    lib = L.load()
    for name in names:
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert hasattr(L, "SvpBiRrt") and hasattr(L.SvpSpace, "edge_check_back")
    for m in ("solve", "status", "tree", "solution", "finished", "stats", "close"):
        assert m == "stats" or hasattr(L.SvpBiRrt, m), m
    hdr = open(os.path.join(ROOT, "include", "rkh.h")).read()
    assert "move_pt_back_to, and batch planners" not in hdr   # no longer among the things not built
