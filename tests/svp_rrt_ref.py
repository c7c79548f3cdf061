"""Plain-Python twin of the batch RRT over the SVP space (reak_amd/csrc/svp_planner.hip, the loop include/rkh.h states): the
loop of examples/plan_svp_rrt.py::svp_rrt with the library's own sample stream instead of numpy's, on the twin of the
space (tests/svp_ref.py).  One problem at a time; the device is held to it bit for bit, problem by problem.

  Mt19937            std::mt19937: seeding, block regeneration, tempering (about 20 lines)
  candidate_stream   candidate k = draws k D .. k D + D - 1 as (p0, v0, p1, v1, ...), coordinate = lo + u (hi - lo)
  rrt                the loop; `walk(a, b, fraction)` is the collision-tested walk, so that a test chooses the predicate
"""
import math

import svp_ref as R

NO_INDEX = 0xFFFFFFFF
WINDOW = 64   # candidates per refill of a problem's sample window (kRl1Window, svp_planner.hip)
SLICE = 256   # vertices per block of the nearest sweep (kRl1Slice)


class Mt19937:
    def __init__(self, seed=5489):
        self.mt = [seed & 0xFFFFFFFF]
        for k in range(1, 624):
            prev = self.mt[-1]
            self.mt.append((1812433253 * (prev ^ (prev >> 30)) + k) & 0xFFFFFFFF)
        self.idx = 624

    def _regenerate(self):
        mt = self.mt
        for i in range(624):
            y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
            mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        self.idx = 0

    def next(self):
        if self.idx == 624:
            self._regenerate()
        y = self.mt[self.idx]
        self.idx += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y


def unit(y):
    return float(y) * (1.0 / 4294967296.0)


def coord_range(sp, c):
    i = c >> 1
    return (-sp.vm[i], sp.vm[i]) if c & 1 else (sp.lower[i], sp.upper[i])


def coord(lo, hi, u):
    return lo + u * (hi - lo)


def candidates(sp, rng, count):
    """the next `count` candidates of the stream `rng` is at"""
    D = 2 * sp.n
    out = []
    for _ in range(count):
        out.append([coord(*coord_range(sp, c), unit(rng.next())) for c in range(D)])
    return out


def fraction_of(asked, max_edge_time):
    return min(1.0, max_edge_time / asked) if asked > 0.0 else 1.0


def progress(travelled, asked, fraction, steer_tol):
    best = asked * fraction
    return math.isfinite(travelled) and travelled < 2.0 * best and travelled > steer_tol * best


def nearest1(sp, verts, q):
    """(index, distance) of the 1-nearest vertex by d(vertex -> q), a tie to the lower index; (NO_INDEX, inf) if none"""
    best, bi = math.inf, NO_INDEX
    for i, v in enumerate(verts):
        d = R.reach(sp, v, q)[0]
        if d < best:
            best, bi = d, i
    return bi, best


def rrt(sp, walk, start, goal, seed, max_vertices, max_iterations, max_edge_time=1.0, steer_tol=0.1):
    """walk(a, b, fraction) -> (out, T, n_checked, reached, ...) as svp_ref.edge_walk answers.  goal None: no probes.
    Returns the tree and `branches`, the count of every way an iteration ended (the tests' census)."""
    rng = Mt19937(seed)
    verts, parent, etime = [list(start)], [NO_INDEX], [0.0]
    goal_parent, it = NO_INDEX, 0
    br = {"out_of_bounds": 0, "no_neighbour": 0, "nothing_checked": 0, "no_progress": 0, "committed": 0}
    if goal is not None and walk(verts[0], list(goal), 1.0)[3]:
        goal_parent = 0
    while goal_parent == NO_INDEX and len(verts) < max_vertices and it < max_iterations:
        it += 1
        q = candidates(sp, rng, 1)[0]
        if not R.in_bounds(sp, q):
            br["out_of_bounds"] += 1
            continue
        idx, asked = nearest1(sp, verts, q)
        if idx == NO_INDEX:
            br["no_neighbour"] += 1
            continue
        near = verts[idx]
        fraction = fraction_of(asked, max_edge_time)
        w = walk(near, q, fraction)
        out, n_checked = w[0], w[2]
        if n_checked == 0:
            br["nothing_checked"] += 1
            continue
        travelled = R.reach(sp, near, out)[0]
        if not progress(travelled, asked, fraction, steer_tol):
            br["no_progress"] += 1
            continue
        br["committed"] += 1
        verts.append(list(out))
        parent.append(idx)
        etime.append(travelled)
        if goal is not None and walk(out, list(goal), 1.0)[3]:
            goal_parent = len(verts) - 1
    why = "goal" if goal_parent != NO_INDEX else ("max_vertices" if len(verts) >= max_vertices else "max_iterations")
    return {"vertices": verts, "parent": parent, "edge_time": etime, "goal_parent": goal_parent, "iterations": it,
            "branches": br, "why": why}


def solution(sp, tree, goal):
    """(points start ... goal, duration): the edges' reach times summed in path order; ([], 0.0) without a goal_parent"""
    if tree["goal_parent"] == NO_INDEX:
        return [], 0.0
    chain, v = [], tree["goal_parent"]
    while v != NO_INDEX:
        chain.append(v)
        v = tree["parent"][v]
    chain.reverse()
    total = 0.0
    for v in chain[1:]:
        total += tree["edge_time"][v]
    total += R.reach(sp, tree["vertices"][chain[-1]], list(goal))[0]
    return [tree["vertices"][v] for v in chain] + [list(goal)], total
