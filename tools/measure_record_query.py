#!/usr/bin/env python3
"""Kernel time of rkh_min_distance_records next to rkh_min_distance on the same 65 536 random C2 states: events around
each launch (rkh_diag_distance_query_ms), one warm-up, then the minimum of five runs.  Needs the GPU.

    python tools/measure_record_query.py --out profiles/r07_record_query.json
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
    a = ap.parse_args()
    from reak_amd import lib, scenarios

    scn = scenarios.make_c2()
    rng = np.random.default_rng(5)
    lo = np.array([scn.dyn.lower[i] for i in range(scn.D)])
    hi = np.array([scn.dyn.upper[i] for i in range(scn.D)])
    x = rng.uniform(lo, hi, size=(a.states, scn.D))
    sc = lib.Scene(lib.Context(0), scn)
    res = {"scene": "make_c2()", "states": a.states, "pairs": sc.num_pairs, "warmup": 1, "runs": 5}
    for name, records in (("min_distance_kernel_ms", False), ("min_distance_records_kernel_ms", True)):
        ms = sc.distance_query_ms(x, records, 6)[1:]
        res[name] = float(ms.min())
        res[name + "_runs"] = [float(v) for v in ms]
    res["ratio"] = res["min_distance_records_kernel_ms"] / res["min_distance_kernel_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")
