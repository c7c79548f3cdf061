"""P copies of the C2 rest-to-rest problem of examples/plan_svp_rrt.py with different seeds, planned in ONE batch RRT over
the order-1 rate-limited joint space with SVP profiles (rkh_svp_rrt_*): trees, sample streams and all per-problem state
stay on the device, every launch serves all unfinished problems.

    python examples/plan_svp_rrt_batch.py [problems] [max_vertices]

Prints vertices, iterations and trajectory duration per problem, shortcuts all found solutions in one
rkh_svp_shortcut_paths call (duration before and after), then samples the shortest shortcut trajectory with
rkh_svp_interpolate.  (The sample stream is the library's own, std::mt19937 per problem: the trees are not those of the
host loop in plan_svp_rrt.py, which draws from numpy's generator.)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from plan_svp_rrt import ACCEL, GOAL, SPEED, c2_space, to_space  # noqa: E402


def main():
    from reak_amd import lib, scenarios
    from reak_amd import types as T

    P = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    max_vertices = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    scn = scenarios.make_c2(world_seed=1)
    ctx = lib.Context(0)
    scene = lib.Scene(ctx, scn)
    n, lower, upper, mi, speed, accel = c2_space()
    cs = T.make_svp_space(n, lower, upper, mi, speed, accel)
    start, goal = to_space(scn.start[0::2]), to_space(GOAL)
    params = [T.make_svp_rrt_params(start, goal, seed=1 + i, max_vertices=max_vertices, max_iterations=20000,
                                    max_edge_time=1.0, steer_tol=0.1) for i in range(P)]
    planner = lib.SvpRrt(scene, cs, params)
    stats = planner.solve()
    nv, it, gp = planner.status()
    print("%d problems in %d rounds: %d iterations, %d vertices, %d points tested" %
          (P, stats.rounds, stats.iterations, stats.vertices, stats.tested_points))
    cut = planner.shortcut_solutions()   # every found solution, all their vertex pairs walked, in one call
    best, best_dur = -1, np.inf
    for i in range(P):
        if i in cut:
            c = cut[i]
            print("problem %d (seed %d): vertices %d, iterations %d, path of %d edges, duration %.6f s; shortcut to %d edges, "
                  "%.6f s%s" % (i, 1 + i, nv[i], it[i], len(c["points"]) - 1, c["duration"], len(c["keep"]) - 1, c["time_out"],
                                " (%d hops fail the re-walk)" % c["n_blocked"] if c["n_blocked"] else ""))
            if c["time_out"] < best_dur:
                best, best_dur = i, c["time_out"]
        else:
            print("problem %d (seed %d): vertices %d, iterations %d, no path to the goal" % (i, 1 + i, nv[i], it[i]))
    if best < 0:
        return
    pts = cut[best]["points"][cut[best]["keep"]]
    space = lib.SvpSpace(cs, scene=scene)
    a, b = pts[:-1], pts[1:]
    times = space.reach_time(a, b, peaks=False)
    M = 50
    t = np.linspace(0.0, 1.0, M)[None, :] * times[:, None]
    traj, _ = space.interpolate(a, b, t)          # [edges][M][2n]: the trajectory, edge after edge
    q = traj[:, :, 0::2] * np.array(SPEED)        # joint positions [rad] and rates [rad/s] to execute
    qd = traj[:, :, 1::2] * np.array(ACCEL)
    print("best: problem %d, trajectory duration %.6f s, %d samples; peak |qd| %.3f rad/s" %
          (best, float(times.sum()), q.shape[0] * q.shape[1], float(np.abs(qd).max())))
    planner.close()


if __name__ == "__main__":
    main()
