#!/usr/bin/env python3
"""Wall time per call of the one-shot entries the adaptors call once per edge -- rkh_propagate, rkh_edge_check -- and of
rkh_min_distance, on C2 at B = 1 and B = 256: the median of 2000 calls after 200 warm-up calls, through ctypes with the
arguments prepared once.  The host cost of a one-shot call (allocations, copies, the wait) is what these figures hold.

    python tools/measure_entry_latency.py [--root TREE] [--calls 2000] [--warmup 200] [--label NAME]

--root: the checkout whose built reak_amd is measured (default: this one), so that two builds are measured by one script.
Prints one JSON line: {"label": ..., "us": {entry: {B: median microseconds}}}."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from reak_amd import lib as L, scenarios
    from reak_amd import types as T

    ctx = L.Context(0)
    scn = scenarios.make_c2(world_seed=1)
    sc = L.Scene(ctx, scn)
    n, D = sc.n, sc.D
    rng = np.random.default_rng(0)
    lower, upper = np.full(n, -np.pi), np.full(n, np.pi)
    us = {}
    for B in (1, 256):
        xa = rng.uniform(-0.5, 0.5, size=(B, D))
        xb = xa + rng.uniform(-0.05, 0.05, size=(B, D))
        qa, qb = np.ascontiguousarray(xa[:, :n]), np.ascontiguousarray(xa[:, :n] + 0.2)
        x_out, steps, dist = np.zeros((B, D)), np.zeros(B, dtype=np.uint32), np.zeros(B)
        q_out, chk = np.zeros((B, n)), np.zeros(B, dtype=np.uint32)
        dyn = C.byref(scn.dyn)
        p = {k: T.dptr(v) for k, v in dict(xa=xa, xb=xb, qa=qa, qb=qb, x_out=x_out, dist=dist, q_out=q_out, lo=lower,
                                           hi=upper).items()}
        ps, pc = T.u32ptr(steps), T.u32ptr(chk)
        lib, h = sc.lib, sc.h
        entries = {
            "rkh_propagate": lambda: lib.rkh_propagate(h, dyn, p["xa"], p["xb"], B, 1.0, p["x_out"], ps, None),
            "rkh_edge_check": lambda: lib.rkh_edge_check(h, p["lo"], p["hi"], 0.05, p["qa"], p["qb"], B, 1.0, p["q_out"], pc),
            "rkh_min_distance": lambda: lib.rkh_min_distance(h, p["xa"], B, p["dist"]),
        }
        for name, call in entries.items():
            for _ in range(args.warmup):
                st = call()
                assert st == 0, (name, B, st, lib.rkh_last_error().decode())
            t = np.empty(args.calls)
            for i in range(args.calls):
                t0 = time.perf_counter()
                call()
                t[i] = time.perf_counter() - t0
            us.setdefault(name, {})[str(B)] = round(float(np.median(t)) * 1e6, 2)
    print(json.dumps({"label": args.label, "calls": args.calls, "warmup": args.warmup, "us": us}))


if __name__ == "__main__":
    main()
