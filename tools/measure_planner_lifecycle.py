"""Where a batch planner's time goes outside its solve loop: create, first sample upload, solve, counter reads, close.

Scene: C2 (scenarios.make_c2(world_seed=1)), the benchmark's.  The scene and the --problems rrt_params of every planner
are built before any clock starts.  Per size in --vertices, --planners planners are created, solved and closed one after
the other (the first one is the cold one), seeds as bench.py's steps take them.  Every phase ends in a device
synchronise and is timed with the host clock:
  create    RrtPlannerPool(...)
  enqueue0  enqueue(0): the first share of every problem's sample stream
  solve     enqueue(16) / sync until every problem is done
  counters  the reads bench.py does after a step: nn_profile, steer_profile, steer_steps, nn_pairs
  close     close()
RKH_PROFILE_NN=1 as in a benchmark run unless the environment says otherwise.  Prints one JSON line.
--tree measures another checkout (its reak_amd package and built librkh.so) with the same scene."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--problems", type=int, default=512)
ap.add_argument("--vertices", type=int, nargs="+", default=[100000, 2000])
ap.add_argument("--planners", type=int, default=3)
ap.add_argument("--groups", type=int, default=1)
ap.add_argument("--label", default="")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
os.environ.setdefault("RKH_PROFILE_NN", "1")

import torch  # noqa: E402

from reak_amd import dist_utils, lib, scenarios  # noqa: E402


def lifecycle(scene, prms):
    phases = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        phases[name] = time.perf_counter() - t0
        return out

    pl = timed("create", lambda: lib.RrtPlannerPool(scene, prms, groups=args.groups))
    timed("enqueue0", lambda: pl.enqueue(0))

    def solve():
        while not pl.done:
            pl.enqueue(16)
            pl.sync()
    timed("solve", solve)
    timed("counters", lambda: (pl.nn_profile(), pl.steer_profile(), pl.steer_steps(), pl.nn_pairs()))
    nodes = sum(int(st.num_vertices) - 1 for st in pl.all_stats)
    timed("close", pl.close)
    phases["vertices_added"] = nodes
    return phases


scn = scenarios.make_c2(world_seed=1)
ctx = lib.Context(0)
scene = lib.Scene(ctx, scn)
sizes = []
for vertices in args.vertices:
    batches = [[scn.rrt_params(seed=s, max_vertices=vertices) for s in dist_utils.seeds_for_rank(k, 0, 1, args.problems)]
               for k in range(args.planners)]
    runs = [lifecycle(scene, prms) for prms in batches]
    warm = runs[1:] or runs
    sizes.append({"max_vertices": vertices, "planners": runs,
                  "warm_create_plus_close_s": sum(r["create"] + r["close"] for r in warm) / len(warm),
                  "warm_outside_solve_s": sum(r["create"] + r["enqueue0"] + r["counters"] + r["close"] for r in warm) / len(warm),
                  "warm_solve_s": sum(r["solve"] for r in warm) / len(warm)})
print(json.dumps({"label": args.label, "problems": args.problems, "groups": args.groups,
                  "arena_cache": os.environ.get("RKH_ARENA_CACHE"), "sizes": sizes}))
