#!/usr/bin/env python3
"""Kernel time of the record query next to rkh_min_distance on the same 65 536 random states: events around each launch
(rkh_diag_distance_query_ms), one warm-up, then the minimum of five runs.  Needs the GPU.

    python tools/measure_record_query.py --out profiles/r07_record_query.json                       C2, rkh_min_distance_records
    python tools/measure_record_query.py --scene planar4 --out profiles/r14_planar_record_query.json   make_planar_mixed(n=4),
                                                                                                    rkh_min_distance_records_2d
    python tools/measure_record_query.py --scene c4_meshes --out profiles/r16_mesh_record_query.json   make_c4(meshes=True),
                                                                                                    rkh_min_distance_records_meshes
    python tools/measure_record_query.py --scene c4_depth --out profiles/r17_depth_record_query.json   the same scene:
        rkh_min_distance_records_depth's kernel next to rkh_min_distance_records_meshes' (whose code the depth forms left
        as it was), on the random states and on sets of as many states that are all free and that all collide (the free
        and the colliding ones of 8 x as many draws, repeated in order)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--states", type=int, default=65536)
    ap.add_argument("--scene", choices=("c2", "planar4", "c4_meshes", "c4_depth"), default="c2")
    a = ap.parse_args()
    from reak_amd import lib, scenarios

    rng = np.random.default_rng(5)
    if a.scene in ("c2", "c4_meshes", "c4_depth"):  # (c4_meshes: 200 convex-mesh obstacles, 2400 support-map finders)
        scn, label = (scenarios.make_c2(), "make_c2()") if a.scene == "c2" else (scenarios.make_c4(meshes=True), "make_c4(meshes=True)")
        lo = np.array([scn.dyn.lower[i] for i in range(scn.D)])
        hi = np.array([scn.dyn.upper[i] for i in range(scn.D)])
        x = rng.uniform(lo, hi, size=(a.states, scn.D))
    else:  # a planar scene given at position level: joint angles in its box, rates zero
        scn, label = scenarios.make_planar_mixed(n=4), "make_planar_mixed(n=4)"
        x = np.zeros((a.states, scn.D))
        x[:, 0::2] = rng.uniform(scn.meta["lower"], scn.meta["upper"], size=(a.states, scn.n_dof))
    sc = lib.Scene(lib.Context(0), scn)
    res = {"scene": label, "states": a.states, "pairs": sc.num_pairs, "warmup": 1, "runs": 5}
    if a.scene == "c4_depth":
        more = rng.uniform(lo, hi, size=(8 * a.states, scn.D))
        d_more = sc.min_distance(more)
        hits, free = more[d_more < 0.0], more[d_more >= 0.0]
        sets = {"random": x}
        if len(free):      # no pair crosses on a free state: the expansion never runs
            sets["all_free"] = free[np.arange(a.states) % len(free)]
        if len(hits):
            sets["all_colliding"] = hits[np.arange(a.states) % len(hits)]
        res["colliding_draws"], res["free_draws"] = int(len(hits)), int(len(free))
        for tag, xs in sets.items():
            d_m, d_d = sc.min_distance_records_meshes(xs)["dist"], sc.min_distance_records_depth(xs)["dist"]
            r = {"colliding": int(np.sum(d_m < 0.0)), "deeper_than_the_sentinel": int(np.sum(d_d < d_m))}
            for name, records in (("min_distance_records_meshes_kernel_ms", True), ("min_distance_depth_kernel_ms", "depth")):
                ms = sc.distance_query_ms(xs, records, 6)[1:]
                r[name] = float(ms.min())
                r[name + "_runs"] = [float(v) for v in ms]
            r["ratio"] = r["min_distance_depth_kernel_ms"] / r["min_distance_records_meshes_kernel_ms"]
            res[tag] = r
        line = json.dumps(res)
        print(line)
        if a.out:
            open(a.out, "w").write(line + "\n")
        sys.exit(0)
    for name, records in (("min_distance_kernel_ms", False), ("min_distance_records_kernel_ms", True)):
        ms = sc.distance_query_ms(x, records, 6)[1:]
        res[name] = float(ms.min())
        res[name + "_runs"] = [float(v) for v in ms]
    res["ratio"] = res["min_distance_records_kernel_ms"] / res["min_distance_kernel_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")
