#!/usr/bin/env python3
"""Time of rkh_shortcut_paths on random-walk paths over free points of the 40-obstacle C1 scene (the scene of the
scene-level test in tests/test_path_shortcut_gpu.py): B in {1, 64} paths of L in {33, 129} points, every pair tried.
Needs the GPU.

    python tools/measure_shortcut.py --out profiles/r19_path_shortcut.json

Per shape, after one warm-up, minimum and maximum of `runs` runs of
  call_ms          wall time of rkh_shortcut_paths (copies, the three launches, the wait)
  pairs_ms, walks_ms, search_ms   the three launches alone, between events (rkh_diag_shortcut_ms)
  edge_check_plus_host_dp_ms      what a caller could do without this entry: ONE rkh_edge_check call over the same pairs
                                  (verdict = the walk returns its target) and the search as a numpy loop on the host.
                                  The reference for the comparison, not code under test; the answers must agree.
walk_share = walks_ms / (pairs_ms + walks_ms + search_ms) of the fastest runs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_paths(sc, lo, hi, B, n_pts, rng, sigma=0.6):
    """B Gaussian random walks of n_pts free points (free: the device's distance query is above 1e-3)"""
    def free(p):
        x = np.zeros((len(p), 6))
        x[:, 0::2] = p
        return sc.min_distance(x) > 1e-3

    seeds = rng.uniform(lo, hi, (8 * B + 64, 3))
    seeds = seeds[free(seeds)][:B]
    paths = [[s] for s in seeds]
    while any(len(p) < n_pts for p in paths):
        todo = [p for p in paths if len(p) < n_pts]
        cand = np.array([p[-1] for p in todo]) + rng.normal(0.0, sigma, (len(todo), 3))
        good = free(cand) & (cand >= lo).all(axis=1) & (cand <= hi).all(axis=1)
        for p, c, g in zip(todo, cand, good):
            if g:
                p.append(c)
    return [np.array(p) for p in paths]


def host_way(sc, lo, hi, mi, paths):
    """one rkh_edge_check call for all pairs of all paths, then the double loop per path on the host (rows in numpy)"""
    a, b, rows = [], [], []
    for p in paths:
        n = len(p)
        i, j = np.triu_indices(n, 1)           # i ascending, then j ascending: the pair order
        a.append(p[i]), b.append(p[j]), rows.append(n)
    a, b = np.concatenate(a), np.concatenate(b)
    out, _ = sc.move_position_toward(lo, hi, mi, a, b, 1.0)
    d = a - b
    s = np.zeros(len(a))
    for k in range(d.shape[1]):
        s = s + d[:, k] * d[:, k]
    w = np.sqrt(s)
    ok = (w < mi) | (out.view(np.uint64) == b.view(np.uint64)).all(axis=1)
    keeps, costs, base = [], [], 0
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
        keep = [n - 1]
        while keep[-1] != 0:
            keep.append(int(pred[keep[-1]]))
        keeps.append(keep[::-1]), costs.append(dist[n - 1])
    return keeps, np.array(costs)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    from reak_amd import lib, scenarios

    scn = scenarios.make_c1(world_seed=1, n_obstacles=40)
    lo, hi, mi = np.asarray(scn.meta["lower"]), np.asarray(scn.meta["upper"]), scn.meta["min_interval"]
    sc = lib.Scene(lib.Context(0), scn)
    qs = lib.make_qs_space(3, lo, hi, mi)
    res = {"scene": "make_c1(world_seed=1, n_obstacles=40)", "max_span": 0, "warmup": 1, "runs": a.runs, "shapes": []}
    rng = np.random.default_rng(19)
    for B in (1, 64):
        for n_pts in (33, 129):
            paths = make_paths(sc, lo, hi, B, n_pts, rng)
            keep, cin, cout, nb = sc.shortcut_paths(qs, paths)          # warm-up, and the answer
            call = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                sc.shortcut_paths(qs, paths)
                call.append((time.perf_counter() - t0) * 1e3)
            ms = sc.shortcut_ms(qs, paths, runs=a.runs)
            hk, hc = host_way(sc, lo, hi, mi, paths)                    # warm-up
            host = []
            for _ in range(max(3, a.runs // 2 + 1)):
                t0 = time.perf_counter()
                hk, hc = host_way(sc, lo, hi, mi, paths)
                host.append((time.perf_counter() - t0) * 1e3)
            agree = all(list(k) == h for k, h in zip(keep, hk)) and np.array_equal(cout.view(np.uint64), hc.view(np.uint64))
            best = ms.min(axis=0)
            row = {"paths": B, "points_per_path": n_pts, "pairs": B * n_pts * (n_pts - 1) // 2,
                   "points_kept": [int(min(len(k) for k in keep)), int(max(len(k) for k in keep))],
                   "paths_with_blocked_hops": int((nb > 0).sum()),
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
