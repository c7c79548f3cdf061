"""P copies of the C2 rest-to-rest problem of examples/plan_svp_rrt.py with different seeds, planned in ONE batch
bidirectional RRT over the order-1 rate-limited joint space with SVP profiles (rkh_svp_birrt_*): per problem a tree that
grows forward from the start and one that grows backward from the goal (every edge of it a profile that runs towards the
goal), all on the device.

    python examples/plan_svp_birrt_batch.py [problems] [max_vertices]

Prints both trees' sizes, iterations and trajectory duration per problem, then shortcuts all joined solutions in one
rkh_svp_shortcut_paths call (duration before and after).  max_vertices bounds each tree.  (This planner is not known to be
faster than rkh_svp_rrt on this scene: see DESIGN.md.)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from plan_svp_rrt import GOAL, c2_space, to_space  # noqa: E402


def main():
    from reak_amd import lib, scenarios
    from reak_amd import types as T

    P = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    max_vertices = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    scn = scenarios.make_c2(world_seed=1)
    ctx = lib.Context(0)
    scene = lib.Scene(ctx, scn)
    n, lower, upper, mi, speed, accel = c2_space()
    cs = T.make_svp_space(n, lower, upper, mi, speed, accel)
    start, goal = to_space(scn.start[0::2]), to_space(GOAL)
    params = [T.make_svp_rrt_params(start, goal, seed=1 + i, max_vertices=max_vertices, max_iterations=20000,
                                    max_edge_time=1.0, steer_tol=0.1) for i in range(P)]
    planner = lib.SvpBiRrt(scene, cs, params)
    stats = planner.solve()
    n0, n1, it, j0, j1 = planner.status()
    print("%d problems in %d rounds: %d iterations, %d vertices in both trees, %d points tested" %
          (P, stats.rounds, stats.iterations, stats.vertices, stats.tested_points))
    joined = [i for i in range(P) if j0[i] != planner.NO_INDEX]
    sols = {i: planner.solution(i) for i in joined}
    cut = {}
    if joined:   # every joined solution, all their vertex pairs walked, in one call
        keep, t_in, t_out, blocked = lib.SvpSpace(cs, scene=scene).shortcut_paths([sols[i][0] for i in joined])
        cut = {i: (keep[k], float(t_out[k]), int(blocked[k])) for k, i in enumerate(joined)}
    for i in range(P):
        head = "problem %d (seed %d): trees of %d + %d vertices, iterations %d" % (i, 1 + i, n0[i], n1[i], it[i])
        if i in cut:
            pts, dur = sols[i]
            keep, t_out, blocked = cut[i]
            print("%s, joined at (%d, %d): path of %d edges, duration %.6f s; shortcut to %d edges, %.6f s%s" %
                  (head, j0[i], j1[i], len(pts) - 1, dur, len(keep) - 1, t_out,
                   " (%d hops fail the re-walk)" % blocked if blocked else ""))
        else:
            print("%s, no join" % head)
    planner.close()


if __name__ == "__main__":
    main()
