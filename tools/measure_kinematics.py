#!/usr/bin/env python3
"""Kernel times of the kinematics entries on C2 (6 revolute joints, 50 obstacles).  Needs the GPU.

    python tools/measure_kinematics.py --out profiles/r20_kinematics.json

Events around the launch on the context's stream, one warm-up, then `runs` runs (rkh_diag_kinematics_ms, rkh_diag_ik_ms,
rkh_diag_distance_query_ms); each figure is [minimum, maximum] in ms.  No copies are timed.
  frames_jacobians_ms   the launch that writes pose, twist, Jac and JacDot (with the clear of the two Jacobian arrays in
                        front of it) for 65 536 random states: the tool frame alone (F = 1), and every frame of the chain
  min_distance_ms       min_distance_kernel on the same states: the yardstick (one full proximity query per state)
  ik_solve_ms           kinematics_ik_kernel on 4096 targets x 16 seeds, seeds uniform in the joint box (far seeds: the solves
                        that do not converge run all 100 iterations), targets = tool poses of random configurations
  ik_distance_ms        the distance launch over the 65 536 results that follows it
Records only: no test depends on a time."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def span(v):
    return [float(np.min(v)), float(np.max(v))]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--states", type=int, default=65536)
    ap.add_argument("--targets", type=int, default=4096)
    ap.add_argument("--seeds", type=int, default=16)
    a = ap.parse_args()
    from reak_amd import lib, scenarios
    from reak_amd import types as T

    scn = scenarios.make_c2(world_seed=1)
    n = scn.n_dof
    sc = lib.Scene(lib.Context(0), scn)
    rng = np.random.default_rng(20)
    tool, frames = 2 * n, list(range(2 * n + 1))
    q, qd = rng.uniform(-2.5, 2.5, (a.states, n)), rng.uniform(-1.0, 1.0, (a.states, n))
    x = np.zeros((a.states, 2 * n))
    x[:, 0::2], x[:, 1::2] = q, qd
    res = {"scene": "make_c2(world_seed=1)", "n_dof": n, "proxy_pairs": sc.num_pairs, "warmup": 1, "runs": a.runs,
           "states": a.states}
    res["frames_jacobians_ms"] = {"tool_frame": span(sc.kinematics_ms(q, [tool], qd, runs=a.runs)),
                                  "all_%d_frames" % len(frames): span(sc.kinematics_ms(q, frames, qd, runs=a.runs))}
    res["min_distance_ms"] = span(sc.distance_query_ms(x, False, a.runs))
    # IK: targets are tool poses of random configurations, from the device's own direct kinematics
    lo, hi = np.full(n, -np.pi), np.full(n, np.pi)
    qt = rng.uniform(-2.5, 2.5, (a.targets, n))
    fk = sc.direct_kinematics(qt, [tool], want=("pos", "rot"))
    targets = [T.make_pose(p, r / np.linalg.norm(r)) for p, r in zip(fk["pos"][:, 0], fk["rot"][:, 0])]
    seeds = rng.uniform(lo, hi, (a.targets, a.seeds, n))
    prm = T.make_ik_params()
    ik = sc.inverse_kinematics(tool, targets, seeds, lo, hi, prm)
    ms = sc.ik_ms(tool, targets, seeds, lo, hi, prm, runs=a.runs)
    res["ik"] = {"targets": a.targets, "seeds_per_target": a.seeds, "seeds": "uniform in [-pi, pi]^6",
                 "params": {"damping": prm.damping, "max_step": prm.max_step, "max_iters": prm.max_iters,
                            "tol_pos": prm.tol_pos, "tol_rot": prm.tol_rot},
                 "solves_converged": int(ik["converged"].sum()), "solves": int(ik["converged"].size),
                 "mean_iterations": float(ik["iters"].mean()),
                 "targets_with_a_converged_seed": int(ik["converged"].any(axis=1).sum()),
                 "targets_with_a_converged_free_seed": int((ik["best"] >= 0).sum()),
                 "ik_solve_ms": span(ms[:, 0]), "ik_distance_ms": span(ms[:, 1])}
    text = json.dumps(res)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(text)
