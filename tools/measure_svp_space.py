#!/usr/bin/env python3
"""Times of the SVP-space kernels (reak_amd/csrc/svp_space.hip).  Needs the GPU.

    python tools/measure_svp_space.py --out profiles/r21_svp_space.json

  nearest   rkh_svp_nearest_async at n = 6 over 10 000 / 100 000 / 1 000 000 points, B = 1 / 64 / 1024 queries, k = 1 and 16,
            on device buffers: wall time of launch + rkh_ctx_synchronize, pairs per second
  walk      rkh_svp_edge_check on make_c2() at B = 256 and 16 384 (host copies included: the entry takes host pointers),
            tested points per second
  host      the same arithmetic (reach time per pair; interpolated point + bounds rule per walk point, no collision test)
            by the host build of svp_device.h on one core (tools/svp_host_bench.cpp)
  qs_walk   the existing straight-line walk rkh_edge_check on the same scene at about the same number of tested points:
            the nearest thing the library had before
Each figure: one warm-up call, then the minimum and maximum of three timed calls."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, runs=3):
    fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out), max(out)


class DeviceArray:
    """A numpy array's bytes in device memory, through the HIP runtime the library runs on"""
    hip = None

    def __init__(self, host):
        import ctypes as C
        if DeviceArray.hip is None:
            DeviceArray.hip = C.CDLL("libamdhip64.so")
        host = np.ascontiguousarray(host)
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(host.nbytes)) == 0
        assert self.hip.hipMemcpy(self.ptr, C.c_void_p(host.ctypes.data), C.c_size_t(host.nbytes), 1) == 0

    def free(self):
        self.hip.hipFree(self.ptr)


def points(rng, count, n, half=2.0):
    x = np.zeros((count, 2 * n))
    x[:, 0::2] = rng.uniform(-half, half, size=(count, n))
    x[:, 1::2] = rng.uniform(-1.0, 1.0, size=(count, n))
    return x


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-points", type=int, default=1000000)
    a = ap.parse_args()
    from reak_amd import lib, scenarios
    from reak_amd import types as T

    ctx = lib.Context(0)
    rng = np.random.default_rng(1)
    n = 6
    res = {"n_dof": n, "warmup": 1, "runs": 3, "nearest": [], "walk": [], "qs_walk": []}
    space = lib.SvpSpace(T.make_svp_space(n, [-2.0] * n, [2.0] * n, 0.05), ctx=ctx)
    for n_pts in (10000, 100000, 1000000):
        if n_pts > a.max_points:
            continue
        d_pts = DeviceArray(points(rng, n_pts, n))
        for B in (1, 64, 1024):
            d_q = DeviceArray(points(rng, B, n))
            for k in (1, 16):
                d_idx, d_dist = DeviceArray(np.zeros((B, k), dtype=np.uint32)), DeviceArray(np.zeros((B, k)))

                def call():
                    space.nearest_async(d_pts.ptr, n_pts, d_q.ptr, B, k, 0, d_idx.ptr, d_dist.ptr)
                    ctx.synchronize()
                lo, hi = timed(call)
                d_idx.free(), d_dist.free()
                res["nearest"].append({"points": n_pts, "queries": B, "k": k, "s_min": lo, "s_max": hi,
                                       "pairs_per_s": n_pts * B / lo})
            d_q.free()
        d_pts.free()
    scn = scenarios.make_c2(world_seed=1)
    scene = lib.Scene(ctx, scn)
    speed, accel = [1.0, 1.0, 1.5, 2.0, 2.0, 3.0], [2.0, 2.0, 3.0, 4.0, 4.0, 6.0]
    lower, upper = [-2.8 / s for s in speed], [2.8 / s for s in speed]
    walk = lib.SvpSpace(T.make_svp_space(n, lower, upper, 0.05, speed, accel), scene=scene)
    for B in (256, 16384):
        pa, pb = np.zeros((B, 2 * n)), np.zeros((B, 2 * n))
        pa[:, 0::2] = rng.uniform(0.5 * np.array(lower), 0.5 * np.array(upper), size=(B, n))
        pb[:, 0::2] = rng.uniform(np.array(lower), np.array(upper), size=(B, n))
        out = {}

        def call():
            out["r"] = walk.edge_check(pa, pb)
        lo, hi = timed(call)
        tested = int(out["r"][2].sum())
        res["walk"].append({"edges": B, "tested_points": tested, "reached": int(out["r"][3].sum()), "s_min": lo, "s_max": hi,
                            "edges_per_s": B / lo, "points_per_s": tested / lo})
        # the straight-line walk over the same joint positions, its interval chosen for about as many tested points
        qa, qb = pa[:, 0::2] * np.array(speed), pb[:, 0::2] * np.array(speed)
        length = float(np.linalg.norm(qb - qa, axis=1).sum())
        mi = length / max(tested, 1)
        ql, qu = [-2.8] * n, [2.8] * n

        def call_qs():
            out["q"] = scene.move_position_toward(ql, qu, mi, qa, qb)
        lo, hi = timed(call_qs)
        tq = int(out["q"][1].sum())
        res["qs_walk"].append({"edges": B, "min_interval": mi, "tested_points": tq, "s_min": lo, "s_max": hi,
                               "points_per_s": tq / lo})
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "svp_host_bench")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "cpp", "hip_host"),
                        os.path.join(ROOT, "tools", "svp_host_bench.cpp"), "-o", exe], check=True)
        runs = [json.loads(subprocess.run([exe, "1000000", "0.05"], check=True, capture_output=True, text=True).stdout)
                for _ in range(3)]
    res["host_one_core"] = {"pairs": runs[0]["pairs"], "pairs_per_s_best": max(r["pairs_per_s"] for r in runs),
                            "pairs_per_s_worst": min(r["pairs_per_s"] for r in runs), "walk_points": runs[0]["walk_points"],
                            "points_per_s_best": max(r["points_per_s"] for r in runs),
                            "points_per_s_worst": min(r["points_per_s"] for r in runs)}
    line = json.dumps(res)
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")
