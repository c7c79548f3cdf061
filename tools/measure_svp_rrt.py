#!/usr/bin/env python3
"""Throughput of the batch RRT over the SVP space (reak_amd/csrc/svp_planner.hip) against the host-driven loop of
examples/plan_svp_rrt.py.  Needs the GPU.

    python tools/measure_svp_rrt.py --out profiles/r22_svp_rrt.json

  batch      BASELINE config C2 with examples/plan_svp_rrt.py::c2_space(), no goal, max_vertices = 2000, P = 1 / 64 / 1024
             problems (seeds 1 .. P) in one planner: wall time of rkh_svp_rrt_solve on a fresh planner (create and destroy
             are not timed), iterations per second and vertices per second over all problems
  split      one more solve per P with the phases of every round bracketed by stream events
             (rkh_diag_svp_rrt_profile): sample, nearest + steer, extension walk, commit, probe walk, finish, in
             milliseconds; the walks include their read-backs of the live count, one per pass
  host_loop  examples/plan_svp_rrt.py::svp_rrt, one problem to the same size over rkh_svp_in_bounds / rkh_svp_nearest /
             rkh_svp_edge_check / rkh_svp_reach_time (five small calls per iteration, the tree uploaded again by each
             nearest call), vertices per second
Each figure: one warm-up run, then the minimum and maximum of three timed runs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-vertices", type=int, default=2000)
    ap.add_argument("--problems", type=int, nargs="*", default=[1, 64, 1024])
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
    start = E.to_space(scn.start[0::2])
    result = {"workload": "C2 (world_seed 1), c2_space(), no goal, max_vertices %d, max_edge_time 1.0, steer_tol 0.1" % a.max_vertices,
              "batch": [], "host_loop": None}

    def params(P):
        return [T.make_svp_rrt_params(start, None, seed=1 + i, max_vertices=a.max_vertices, max_iterations=1 << 30)
                for i in range(P)]

    for P in a.problems:
        times, stats = [], None
        for run in range(a.runs + 1):
            pl = lib.SvpRrt(scene, cs, params(P))
            t0 = time.perf_counter()
            stats = pl.solve()
            dt = time.perf_counter() - t0
            if run:   # the first is the warm-up
                times.append(dt)
            pl.close()
        pl = lib.SvpRrt(scene, cs, params(P))
        pl.profile(True)
        pl.solve()
        split = pl.profile(True)
        pl.close()
        row = {"problems": P, "rounds": int(stats.rounds), "iterations": int(stats.iterations), "vertices": int(stats.vertices),
               "walk_passes": int(stats.walk_passes), "tested_points": int(stats.tested_points),
               "seconds_min": min(times), "seconds_max": max(times),
               "iterations_per_s": [stats.iterations / max(times), stats.iterations / min(times)],
               "vertices_per_s": [stats.vertices / max(times), stats.vertices / min(times)],
               "split_ms": split, "split_ms_per_round": {k: v / max(int(stats.rounds), 1) for k, v in split.items()}}
        result["batch"].append(row)
        print(json.dumps(row), flush=True)

    space = lib.SvpSpace(cs, scene=scene)
    vm = np.array(speed) / np.array(accel)
    times, tree = [], None
    for run in range(a.runs + 1):
        t0 = time.perf_counter()
        tree = E.svp_rrt(space, lower, upper, vm, start, None, max_vertices=a.max_vertices if run else min(a.max_vertices, 100),
                         seed=1, max_iterations=1 << 30)
        dt = time.perf_counter() - t0
        if run:
            times.append(dt)
    V = len(tree["vertices"])
    result["host_loop"] = {"problems": 1, "vertices": V, "iterations": int(tree["iterations"]), "seconds_min": min(times),
                           "seconds_max": max(times), "vertices_per_s": [V / max(times), V / min(times)],
                           "iterations_per_s": [tree["iterations"] / max(times), tree["iterations"] / min(times)]}
    print(json.dumps(result["host_loop"]), flush=True)
    for row in result["batch"]:
        row["vertices_per_s_over_host_loop"] = row["vertices_per_s"][0] / result["host_loop"]["vertices_per_s"][1]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
