"""Throughput of a batch dynamic RRT on chains with prismatic joints, per steer mapping.

Scenes: `track` = the CRS A465 on its linear track (scenarios.make_crs_a465_track, 7 joints), `chain6` = the random
6-joint chain of scenarios.make_random_chain(6, seed=4, n_obstacles=16) with joints 0 and 3 turned prismatic (axis scaled
by 0.7 / 1.1, position bounds +-0.5), `analog2d` = the planar CRS A465 analog of scenarios.make_crs_a465_2d(dynamics=True)
(prismatic_joint_2D track + three revolute_joint_2D) and `analog2d_rev` = the same chain with joint 0 made revolute (the
comparison within one build: the planar prismatic forms against the revolute ones).  One warm-up solve at a tenth of the size, then --runs timed solves; the mapping
is whatever the environment asks for (RKH_LANES_PER_EDGE, see the steer plan in reak_amd/csrc/rkh_internal.h).  Prints
one JSON line: valid node expansions/s of every run (vertices added / wall time of the solve), their min and max.
--tree measures another checkout (its reak_amd package and built librkh.so) with the same scenes."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--scene", choices=["track", "chain6", "analog2d", "analog2d_rev"], required=True)
ap.add_argument("--problems", type=int, default=256)
ap.add_argument("--vertices", type=int, default=20000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--label", default="")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

from reak_amd import lib, scenarios  # noqa: E402
from reak_amd import types as T  # noqa: E402


def chain6():
    scn = scenarios.make_random_chain(6, seed=4, n_obstacles=16)
    for j, op in enumerate([o for o in scn.ops if o.kind == T.KTE_REVOLUTE_JOINT_3D]):
        if j in (0, 3):
            op.kind = T.KTE_PRISMATIC_JOINT_3D
            op.axis[:] = [{0: 0.7, 3: 1.1}[j] * v for v in op.axis]
            scn.dyn.lower[2 * j], scn.dyn.upper[2 * j] = -0.5, 0.5
    return scn


def solve(scene, scn, problems, vertices):
    prms = [scn.rrt_params(seed=5000 + i, max_vertices=vertices) for i in range(problems)]
    pl = lib.RrtPlanner(scene, prms)
    t0 = time.perf_counter()
    pl.solve_planning_query()
    dt = time.perf_counter() - t0
    nodes = sum(int(st.num_vertices) - 1 for st in pl.all_stats)
    steps = pl.steer_steps()
    pl.close()
    return nodes / dt, dt, nodes, steps


def analog2d(revolute_root):
    scn = scenarios.make_crs_a465_2d(dynamics=True)
    if revolute_root:
        next(o for o in scn.ops if o.kind == T.KTE_PRISMATIC_JOINT_2D).kind = T.KTE_REVOLUTE_JOINT_2D
    return scn


scn = {"track": scenarios.make_crs_a465_track, "chain6": chain6, "analog2d": lambda: analog2d(False),
       "analog2d_rev": lambda: analog2d(True)}[args.scene]()
ctx = lib.Context(0)
scene = lib.Scene(ctx, scn)
solve(scene, scn, args.problems, max(200, args.vertices // 10))
mapping = lib.steer_mapping_name() if hasattr(lib, "steer_mapping_name") else "n/a"
runs = [solve(scene, scn, args.problems, args.vertices) for _ in range(args.runs)]
print(json.dumps({"label": args.label, "scene": args.scene, "problems": args.problems, "max_vertices": args.vertices,
                  "lanes_per_edge": os.environ.get("RKH_LANES_PER_EDGE"), "mapping": mapping,
                  "expansions_per_s": [r[0] for r in runs], "min": min(r[0] for r in runs), "max": max(r[0] for r in runs),
                  "seconds": [r[1] for r in runs], "vertices_added": runs[0][2], "steer_steps": runs[0][3]}))
