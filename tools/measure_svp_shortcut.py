#!/usr/bin/env python3
"""Time of rkh_svp_shortcut_paths on the solutions of P solved C2 problems of the batch SVP RRT (the problems of
examples/plan_svp_rrt_batch.py: rest to rest, seeds 1 .. P), every vertex pair tried.  Needs the GPU.

    python tools/measure_svp_shortcut.py --out profiles/svp_shortcut_c2.json

Per P, after one warm-up, minimum and maximum of `runs` runs of
  call_ms          wall time of rkh_svp_shortcut_paths (copies, the chunks' launches, the waits)
  pairs_ms, walks_ms, search_ms   the phases alone, between events, summed over the chunks (rkh_diag_svp_shortcut_ms); the
                                  walks include the read-back of the live count per pass
  edge_check_plus_host_dp_ms      what a caller could do without this entry: ONE rkh_svp_edge_check call over the
                                  host-gathered pairs (weight = reach_time, verdict = reached) and the search as a numpy
                                  loop on the host.  The reference for the comparison, not code under test; the answers
                                  must agree.
walk_share = walks_ms / (pairs_ms + walks_ms + search_ms) of the fastest runs.  Nothing here is a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def host_way(space, paths):
    """one rkh_svp_edge_check call for all pairs of all paths, then the double loop per path on the host (rows in numpy)"""
    a, b, rows = [], [], []
    for p in paths:
        n = len(p)
        i, j = np.triu_indices(n, 1)           # i ascending, then j ascending: the pair order
        a.append(p[i]), b.append(p[j]), rows.append(n)
    _, w, _, reached = space.edge_check(np.concatenate(a), np.concatenate(b))
    ok = reached != 0
    keeps, times, base = [], [], 0
    for n in rows:
        dist = np.full(n, np.inf)
        pred = np.zeros(n, dtype=np.int64)
        dist[0] = 0.0
        for i in range(n - 1):
            m = n - 1 - i
            allowed = ok[base:base + m].copy()
            allowed[0] = True
            c = dist[i] + w[base:base + m]
            upd = allowed & (c < dist[i + 1:])
            dist[i + 1:][upd] = c[upd]
            pred[i + 1:][upd] = i
            base += m
        keep = [n - 1] if dist[n - 1] < np.inf else []
        while keep and keep[-1] != 0:
            keep.append(int(pred[keep[-1]]))
        keeps.append(keep[::-1]), times.append(dist[n - 1])
    return keeps, np.array(times)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--problems", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--max-vertices", type=int, default=2000)
    a = ap.parse_args()
    from plan_svp_rrt import GOAL, c2_space, to_space
    from reak_amd import lib, scenarios
    from reak_amd import types as T

    scn = scenarios.make_c2(world_seed=1)
    scene = lib.Scene(lib.Context(0), scn)
    n, lower, upper, mi, speed, accel = c2_space()
    cs = T.make_svp_space(n, lower, upper, mi, speed, accel)
    space = lib.SvpSpace(cs, scene=scene)
    start, goal = to_space(scn.start[0::2]), to_space(GOAL)
    res = {"scene": "make_c2(world_seed=1)", "space": "c2_space() of examples/plan_svp_rrt.py", "max_span": 0, "warmup": 1,
           "runs": a.runs, "shapes": []}
    for P in a.problems:
        params = [T.make_svp_rrt_params(start, goal, seed=1 + i, max_vertices=a.max_vertices, max_iterations=20000,
                                        max_edge_time=1.0, steer_tol=0.1) for i in range(P)]
        planner = lib.SvpRrt(scene, cs, params)
        planner.solve()
        _, _, gp = planner.status()
        paths = [planner.solution(i)[0] for i in range(P) if gp[i] != planner.NO_INDEX]
        planner.close()
        if not paths:
            continue
        keep, t_in, t_out, nb = space.shortcut_paths(paths)              # warm-up, and the answer
        call = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            space.shortcut_paths(paths)
            call.append((time.perf_counter() - t0) * 1e3)
        ms = space.shortcut_ms(paths, runs=a.runs)
        hk, ht = host_way(space, paths)                                  # warm-up
        host = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            hk, ht = host_way(space, paths)
            host.append((time.perf_counter() - t0) * 1e3)
        agree = all(list(k) == h for k, h in zip(keep, hk)) and np.array_equal(t_out.view(np.uint64), ht.view(np.uint64))
        best = ms.min(axis=0)
        row = {"problems": P, "solved": len(paths), "points_per_path": [int(min(map(len, paths))), int(max(map(len, paths)))],
               "pairs": int(sum(len(p) * (len(p) - 1) // 2 for p in paths)),
               "points_kept": [int(min(len(k) for k in keep)), int(max(len(k) for k in keep))],
               "paths_with_blocked_hops": int((nb > 0).sum()),
               "duration_in_s": [float(t_in.min()), float(t_in.max())], "duration_out_s": [float(t_out.min()), float(t_out.max())],
               "mean_duration_ratio": float(np.mean(t_out / t_in)),
               "call_ms": [min(call), max(call)],
               "pairs_ms": [float(ms[:, 0].min()), float(ms[:, 0].max())],
               "walks_ms": [float(ms[:, 1].min()), float(ms[:, 1].max())],
               "search_ms": [float(ms[:, 2].min()), float(ms[:, 2].max())],
               "walk_share": float(best[1] / best.sum()),
               "edge_check_plus_host_dp_ms": [min(host), max(host)], "host_way_agrees": bool(agree)}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")
