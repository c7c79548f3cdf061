#!/usr/bin/env python3
"""Kernel time of the record query next to rkh_min_distance on the same 65 536 random states: events around each launch
(rkh_diag_distance_query_ms), one warm-up, then the minimum of five runs.  Needs the GPU.

    python tools/measure_record_query.py --out profiles/r07_record_query.json                       C2, rkh_min_distance_records
    python tools/measure_record_query.py --scene planar4 --out profiles/r14_planar_record_query.json   make_planar_mixed(n=4),
                                                                                                    rkh_min_distance_records_2d
    python tools/measure_record_query.py --scene c4_meshes --out profiles/r16_mesh_record_query.json   make_c4(meshes=True),
                                                                                                    rkh_min_distance_records_meshes
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
    ap.add_argument("--scene", choices=("c2", "planar4", "c4_meshes"), default="c2")
    a = ap.parse_args()
    from reak_amd import lib, scenarios

    rng = np.random.default_rng(5)
    if a.scene in ("c2", "c4_meshes"):  # (c4_meshes: 200 convex-mesh obstacles, 2400 support-map finders)
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
    for name, records in (("min_distance_kernel_ms", False), ("min_distance_records_kernel_ms", True)):
        ms = sc.distance_query_ms(x, records, 6)[1:]
        res[name] = float(ms.min())
        res[name + "_runs"] = [float(v) for v in ms]
    res["ratio"] = res["min_distance_records_kernel_ms"] / res["min_distance_kernel_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")
