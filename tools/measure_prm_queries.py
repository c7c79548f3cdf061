#!/usr/bin/env python3
"""Time of the roadmap search launch alone (reak_amd/csrc/roadmap_paths.hip) on C1 roadmaps, next to a single-thread
std::priority_queue Dijkstra over the same CSRs on the host: events around the launch (rkh_diag_prm_search_ms), one
warm-up, then the minimum and the spread of five runs, and the relaxation rounds the slowest search took.  Needs the GPU.

    python tools/measure_prm_queries.py --out profiles/r18_prm_queries.json

  whole_batch    256 C1 roadmaps of 2000 vertices, one search from the start vertex each (rkh_prm_get_solution's launch)
  many_sources   one such roadmap, 256 source vertices (rkh_prm_shortest_paths' launch)
Both in the LDS form and, RKH_PRM_PATHS_LDS_MAX lowered, in the global form.  The roadmaps are built first (not timed)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(pl, sources, runs):
    out = {}
    for form, env in (("lds", None), ("global", "1")):
        if env is None:
            os.environ.pop("RKH_PRM_PATHS_LDS_MAX", None)
        else:
            os.environ["RKH_PRM_PATHS_LDS_MAX"] = env
        ms, rounds, host_ms = pl.search_ms(sources, runs=runs)
        out[form] = {"search_launch_ms": float(ms.min()), "search_launch_ms_max": float(ms.max()),
                     "search_launch_ms_runs": [float(v) for v in ms], "max_rounds": int(rounds)}
        out["host_dijkstra_ms"] = min(out.get("host_dijkstra_ms", np.inf), float(host_ms))
    os.environ.pop("RKH_PRM_PATHS_LDS_MAX", None)
    out["host_over_device_lds"] = out["host_dijkstra_ms"] / out["lds"]["search_launch_ms"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--vertices", type=int, default=2000)
    ap.add_argument("--sources", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    from reak_amd import lib, scenarios

    c1 = scenarios.make_c1(world_seed=1)
    lo, hi, mi = c1.meta["lower"], c1.meta["upper"], c1.meta["min_interval"]
    sc = lib.Scene(lib.Context(0), c1)
    prms = [c1.prm_params(seed=1 + i, max_vertices=a.vertices, sampling_radius=1.0) for i in range(a.problems)]
    pl = lib.PrmPlanner(sc, prms, lib.make_qs_space(3, lo, hi, mi))
    pl.solve_planning_query()
    nv = [int(s.num_vertices) for s in pl.all_stats]
    ne = [int(s.num_edges) for s in pl.all_stats]
    res = {"scene": "make_c1(world_seed=1)", "warmup": 1, "runs": a.runs, "threads_per_workgroup": 256,
           "whole_batch": {"problems": a.problems, "vertices_per_roadmap": [min(nv), max(nv)], "edges_per_roadmap": [min(ne), max(ne)],
                           "sources_per_problem": 1}}
    res["whole_batch"].update(timed(pl, None, a.runs))
    connected = sum(1 for i in range(a.problems) if np.isfinite(pl.solution(i)[1]))
    res["whole_batch"]["problems_with_a_path"] = connected
    rng = np.random.default_rng(3)
    src = rng.choice(nv[0], size=a.sources, replace=False).astype(np.uint32)
    res["many_sources"] = {"problems": 1, "vertices_per_roadmap": nv[0], "edges": ne[0], "sources_per_problem": a.sources}
    res["many_sources"].update(timed(pl, src, a.runs))
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")
