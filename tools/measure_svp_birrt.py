#!/usr/bin/env python3
"""The batch bidirectional RRT over the SVP space (reak_amd/csrc/svp_biplanner.hip) beside the batch RRT
(svp_planner.hip) on the same problems.  Needs the GPU.  A record, not a gate.

    python tools/measure_svp_birrt.py --out profiles/r25_svp_birrt.json

  workload   BASELINE config C2 with examples/plan_svp_rrt.py::c2_space() and its GOAL, rest to rest, P = 512 problems
             (seeds 1 .. P), max_vertices 1000 (per tree for the bidirectional planner), max_iterations 20000,
             max_edge_time 1.0
  both       wall time of the solve on a fresh planner (create and destroy are not timed), rounds, rounds per second, the
             share of problems that ended with a path, vertices at the end
  split      one more solve with the phases of every round bracketed by stream events
             (rkh_diag_svp_birrt_profile / rkh_diag_svp_rrt_profile), in milliseconds
Each time: one warm-up run, then the minimum and maximum of `--runs` timed runs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--problems", type=int, default=512)
    ap.add_argument("--max-vertices", type=int, default=1000)
    ap.add_argument("--max-iterations", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()

    import plan_svp_rrt as E
    from reak_amd import lib, scenarios
    from reak_amd import types as T

    scn = scenarios.make_c2(world_seed=1)
    ctx = lib.Context(0)
    scene = lib.Scene(ctx, scn)
    n, lower, upper, mi, speed, accel = E.c2_space()
    cs = T.make_svp_space(n, lower, upper, mi, speed, accel)
    start, goal = E.to_space(scn.start[0::2]), E.to_space(E.GOAL)
    P = a.problems
    params = [T.make_svp_rrt_params(start, goal, seed=1 + i, max_vertices=a.max_vertices, max_iterations=a.max_iterations,
                                    max_edge_time=1.0, steer_tol=0.1) for i in range(P)]
    result = {"workload": "C2 (world_seed 1), c2_space(), rest to GOAL, P %d, max_vertices %d, max_iterations %d, "
                          "max_edge_time 1.0, steer_tol 0.1" % (P, a.max_vertices, a.max_iterations)}

    def with_path(pl, kind):
        st = pl.status()
        return int(((st[3] if kind == "birrt" else st[2]) != 0xFFFFFFFF).sum())

    for kind, cls in (("birrt", lib.SvpBiRrt), ("rrt", lib.SvpRrt)):
        times, stats, solved = [], None, 0
        for run in range(a.runs + 1):
            pl = cls(scene, cs, params)
            t0 = time.perf_counter()
            stats = pl.solve()
            dt = time.perf_counter() - t0
            if run:   # the first is the warm-up
                times.append(dt)
            solved = with_path(pl, kind)
            pl.close()
        pl = cls(scene, cs, params)
        pl.profile(True)
        pl.solve()
        split = pl.profile(True)
        pl.close()
        rounds = max(int(stats.rounds), 1)
        row = {"planner": kind, "problems": P, "rounds": int(stats.rounds), "iterations": int(stats.iterations),
               "vertices_at_the_end": int(stats.vertices), "walk_passes": int(stats.walk_passes),
               "tested_points": int(stats.tested_points), "problems_with_a_path": solved, "share_with_a_path": solved / P,
               "seconds_min": min(times), "seconds_max": max(times), "rounds_per_s": [rounds / max(times), rounds / min(times)],
               "split_ms": split, "split_ms_per_round": {k: v / rounds for k, v in split.items()}}
        result[kind] = row
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
