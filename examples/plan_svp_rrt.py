"""A host-driven RRT over the order-1 rate-limited joint space with SVP profiles (rkh_svp_*), on BASELINE config C2's
arm and obstacles, from rest to rest.  The usage document of the entries, not a benchmark: every step is one small call.

    python examples/plan_svp_rrt.py [seed] [max_vertices]

A point is (p0, v0, p1, v1, ...) in space coordinates: p = q / speed_limit, v = qd / accel_limit.  The loop
  1. samples a point on the host and rejects it with rkh_svp_in_bounds (the point, and where it could stop or could have
     started from, inside the box);
  2. asks rkh_svp_nearest (direction 0: by d(vertex -> sample)) for the vertex to extend from;
  3. walks the time-optimal profile towards the sample with rkh_svp_edge_check, for at most `max_edge_time` of travel
     (the steer fraction), every min_interval of it tested for bounds and collision;
  4. accepts the point it got by the progress rule of the quasi-static RRT (planning_visitor_base::
     steer_towards_position: travelled > steer_tol x asked and < 2 x asked, travelled = d(vertex -> point));
  5. probes the goal from the new vertex with a whole edge (fraction 1.0);
and, once the goal is reached, samples the found path with rkh_svp_interpolate and prints the trajectory's duration.

`svp_rrt` takes the entries as an object (lib.SvpSpace, or anything with its in_bounds / nearest / edge_check /
reach_time), so that a test can run the same loop on a CPU model of them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPEED = (1.0, 1.0, 1.5, 2.0, 2.0, 3.0)   # rad/s
ACCEL = (2.0, 2.0, 3.0, 4.0, 4.0, 6.0)   # rad/s^2
NO_INDEX = 0xFFFFFFFF
GOAL = (-1.5, 2.21, -0.67, -1.97, 0.65, 2.14)   # rad, at rest: the direct profile from the upright start pose collides


def c2_space(min_interval=0.05, joint_range=2.8):
    """(n, lower, upper, min_interval, speed, accel): joints within +-joint_range rad, in space coordinates"""
    lower = [-joint_range / s for s in SPEED]
    upper = [joint_range / s for s in SPEED]
    return 6, lower, upper, min_interval, list(SPEED), list(ACCEL)


def to_space(q, qd=None):
    """model units (q [n], qd [n]) -> a point of the space"""
    x = np.zeros(2 * len(q))
    x[0::2] = np.asarray(q) / np.array(SPEED[:len(q)])
    if qd is not None:
        x[1::2] = np.asarray(qd) / np.array(ACCEL[:len(q)])
    return x


def svp_rrt(space, lower, upper, vm, start, goal, max_vertices=200, seed=1, max_edge_time=1.0, steer_tol=0.1,
            max_iterations=20000):
    """Returns {"vertices" [V][2n], "parent" [V], "goal_parent": vertex the goal was reached from or -1, "iterations"}.
    goal None: no goal probes, the tree grows to max_vertices."""
    rng = np.random.default_rng(seed)
    n = len(lower)
    lower, upper, vm = np.asarray(lower, dtype=float), np.asarray(upper, dtype=float), np.asarray(vm, dtype=float)
    verts, parent = [np.asarray(start, dtype=float)], [-1]
    goal_parent, it = -1, 0
    if goal is not None:
        goal = np.asarray(goal, dtype=float)
        if space.edge_check(verts[0], goal, 1.0)[3][0]:
            goal_parent = 0
    while goal_parent < 0 and len(verts) < max_vertices and it < max_iterations:
        it += 1
        q = np.zeros(2 * n)
        q[0::2], q[1::2] = rng.uniform(lower, upper), rng.uniform(-vm, vm)
        if not space.in_bounds(q)[0]:
            continue
        idx, dist = space.nearest(np.array(verts), q, 1, 0)
        if idx[0, 0] == NO_INDEX:
            continue
        near, asked = verts[int(idx[0, 0])], float(dist[0, 0])
        fraction = min(1.0, max_edge_time / asked) if asked > 0.0 else 1.0
        out, _, n_checked, _ = space.edge_check(near, q, fraction)
        if n_checked[0] == 0:
            continue
        travelled = float(space.reach_time(near, out[0], peaks=False)[0])
        best_case = asked * fraction
        if not (np.isfinite(travelled) and travelled < 2.0 * best_case and travelled > steer_tol * best_case):
            continue
        verts.append(out[0].copy())
        parent.append(int(idx[0, 0]))
        if goal is not None and space.edge_check(out[0], goal, 1.0)[3][0]:
            goal_parent = len(verts) - 1
    return {"vertices": np.array(verts), "parent": np.array(parent), "goal_parent": goal_parent, "iterations": it}


def solution_points(tree, goal):
    """the vertices from the start to the goal, the goal behind them"""
    chain, v = [], tree["goal_parent"]
    while v >= 0:
        chain.append(tree["vertices"][v])
        v = int(tree["parent"][v])
    return np.array(chain[::-1] + [np.asarray(goal, dtype=float)])


def main():
    from reak_amd import lib, scenarios
    from reak_amd import types as T

    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    max_vertices = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    scn = scenarios.make_c2(world_seed=1)
    ctx = lib.Context(0)
    scene = lib.Scene(ctx, scn)
    n, lower, upper, mi, speed, accel = c2_space()
    space = lib.SvpSpace(T.make_svp_space(n, lower, upper, mi, speed, accel), scene=scene)
    vm = np.array(speed) / np.array(accel)
    start, goal = to_space(scn.start[0::2]), to_space(GOAL)
    tree = svp_rrt(space, lower, upper, vm, start, goal, max_vertices=max_vertices, seed=seed)
    print("vertices %d, iterations %d" % (len(tree["vertices"]), tree["iterations"]))
    if tree["goal_parent"] < 0:
        print("no path to the goal within %d vertices" % max_vertices)
        return
    pts = solution_points(tree, goal)
    a, b = pts[:-1], pts[1:]
    times = space.reach_time(a, b, peaks=False)
    M = 50
    t = np.linspace(0.0, 1.0, M)[None, :] * times[:, None]
    traj, _ = space.interpolate(a, b, t)          # [edges][M][2n]: the trajectory, edge after edge
    q = traj[:, :, 0::2] * np.array(speed)        # joint positions [rad] and rates [rad/s] to execute
    qd = traj[:, :, 1::2] * np.array(accel)
    print("path of %d edges, trajectory duration %.6f s, %d samples; peak |qd| %.3f rad/s" %
          (len(a), float(times.sum()), q.shape[0] * q.shape[1], float(np.abs(qd).max())))


if __name__ == "__main__":
    main()
