"""Plain-Python twin of the batch bidirectional RRT over the SVP space (reak_amd/csrc/svp_biplanner.hip, the loop
include/rkh.h states), on the twins of the space (tests/svp_ref.py), of the RRT's sample stream and scalar rules
(tests/svp_rrt_ref.py) and of the backward walk (tests/svp_back_ref.py).  One problem at a time; the device is held to it
bit for bit, problem by problem.

  birrt       the loop; `walk(a, b, fraction)` / `walk_back(a, b, fraction)` are the collision-tested walks, so that a test
              chooses the predicate
  solution    start ... join0, join1 ... goal and the duration summed in path order
  c2_inputs   the 36 shared C2 problems (12 seeds x rest / moving / tiny) and the free-space slice problem"""
import math
import os
import sys

import svp_back_ref as RB
import svp_ref as R
import svp_rrt_ref as RR

NO = RR.NO_INDEX
BRANCHES = ("out_of_bounds", "no_neighbour", "nothing_checked", "no_progress", "committed", "joined")


def nearest_dir(sp, verts, q, side):
    """(index, distance): side 0 by d(vertex -> q), side 1 by d(q -> vertex); a tie to the lower index; (NO, inf) if none"""
    best, bi = math.inf, NO
    for i, v in enumerate(verts):
        d = R.reach(sp, v, q)[0] if side == 0 else R.reach(sp, q, v)[0]
        if d < best:
            best, bi = d, i
    return bi, best


def birrt(sp, walk, walk_back, start, goal, seed, max_vertices, max_iterations, max_edge_time=1.0, steer_tol=0.1):
    """Returns the two trees as V / P / E [2], join (idx0, idx1) or None, join_time, iterations, why, and the census: `br`
    [2] the count of every way a half step ended per side, `walks` the set of (side, outcome) of the walks made."""
    rng = RR.Mt19937(seed)
    V = [[list(start)], [list(goal)]]
    P = [[NO], [NO]]
    E = [[0.0], [0.0]]
    target = [(list(goal), 0), (list(start), 0)]
    side, it, join, join_time = 0, 0, None, 0.0
    br = [dict.fromkeys(BRANCHES, 0), dict.fromkeys(BRANCHES, 0)]
    walks = set()
    half = 0
    while True:
        if len(V[0]) >= max_vertices or len(V[1]) >= max_vertices:
            why = "max_vertices"
            break
        tp, tv = target[side]
        if tv == NO:
            if it >= max_iterations:
                why = "max_iterations"
                break
            it += 1
            q = RR.candidates(sp, rng, 1)[0]
            if not R.in_bounds(sp, q):
                br[side]["out_of_bounds"] += 1
                continue
            tp = q
        half += 1
        moved, out = False, None
        idx, asked = nearest_dir(sp, V[side], tp, side)
        if idx == NO:
            br[side]["no_neighbour"] += 1
        else:
            near = V[side][idx]
            f = RR.fraction_of(asked, max_edge_time)
            w = walk(near, tp, f) if side == 0 else walk_back(tp, near, f)
            out, n_checked, reached = w[0], w[2], w[3]
            walks.add((side, w[4]))
            if tv != NO and f == 1.0 and reached:
                join = (idx, tv) if side == 0 else (tv, idx)
                join_time = asked
                br[side]["joined"] += 1
                why = "joined"
                break
            if n_checked == 0:
                br[side]["nothing_checked"] += 1
            else:
                travelled = R.reach(sp, near, out)[0] if side == 0 else R.reach(sp, out, near)[0]
                if not RR.progress(travelled, asked, f, steer_tol):
                    br[side]["no_progress"] += 1
                else:
                    br[side]["committed"] += 1
                    V[side].append(list(out))
                    P[side].append(idx)
                    E[side].append(travelled)
                    moved = True
        target[1 - side] = (list(out), len(V[side]) - 1) if moved else (None, NO)
        side = 1 - side
    return {"V": V, "P": P, "E": E, "join": join, "join_time": join_time, "iterations": it, "why": why, "br": br,
            "walks": walks, "half_steps": half}


def solution(t):
    """(points start ... join0, join1 ... goal, duration); ([], 0.0) without a join"""
    if t["join"] is None:
        return [], 0.0
    c0, v = [], t["join"][0]
    while v != NO:
        c0.append(v)
        v = t["P"][0][v]
    c0.reverse()
    pts = [t["V"][0][v] for v in c0]
    total = 0.0
    for v in c0[1:]:
        total += t["E"][0][v]
    total += t["join_time"]
    v = t["join"][1]
    while v != NO:
        pts.append(t["V"][1][v])
        if t["P"][1][v] != NO:
            total += t["E"][1][v]
        v = t["P"][1][v]
    return pts, total


# ---- the shared inputs ------------------------------------------------------------------------------------------------------
CONFIGS = ("rest", "moving", "tiny")
SEEDS = tuple(range(1, 13))


def c2_inputs():
    """(scenario, space, problems): the 36 C2 problems, seeds 1 .. 12 each as rest / moving / tiny, in that order"""
    from reak_amd import scenarios
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import plan_svp_rrt as E
    scn = scenarios.make_c2(world_seed=1)
    n, lower, upper, mi, speed, accel = E.c2_space()
    sp = R.Space(n, lower, upper, mi, speed, accel)
    rest = E.to_space(scn.start[0::2]).tolist()
    moving = list(rest)
    for i in range(n):
        moving[2 * i + 1] = (0.7 if i % 2 == 0 else -0.6) * sp.vm[i]
    goal = E.to_space(E.GOAL).tolist()
    conf = {"rest": (rest, 60, 400, 1.0), "moving": (moving, 40, 150, 0.5), "tiny": (moving, 40, 150, 0.04)}
    probs = []
    for seed in SEEDS:
        for name in CONFIGS:
            start, mv, mi_, met = conf[name]
            probs.append({"name": name, "seed": seed, "start": start, "goal": goal, "max_vertices": mv, "max_iterations": mi_,
                          "max_edge_time": met, "steer_tol": 0.1})
    return scn, sp, probs


def free_space_inputs():
    """(space, problem): three joints in the box [0, 400]^3 with unit limits, no collision test"""
    sp = R.Space(3, [0.0] * 3, [400.0] * 3, 0.05)
    return sp, {"name": "free", "seed": 11, "start": [0.5, 0.0] * 3, "goal": [399.5, 0.0] * 3, "max_vertices": 400,
                "max_iterations": 6000, "max_edge_time": 1.0, "steer_tol": 0.1}


def run(sp, walk, walk_back, p):
    return birrt(sp, walk, walk_back, p["start"], p["goal"], p["seed"], p["max_vertices"], p["max_iterations"],
                 p["max_edge_time"], p["steer_tol"])


def check_c2_conditions(want):
    """what the issue asks of the shared inputs, on the twin's values"""
    assert {t["why"] for t in want} == {"joined", "max_vertices", "max_iterations"}, {t["why"] for t in want}
    for side in (0, 1):
        assert sum(t["br"][side]["joined"] for t in want) >= 1, ("join on side", side)
        for key in ("out_of_bounds", "nothing_checked", "no_progress", "committed"):
            assert sum(t["br"][side][key] for t in want) >= 1, (key, side)
    assert sum(t["br"][0]["no_neighbour"] + t["br"][1]["no_neighbour"] for t in want) >= 1
    kinds = set().union(*(t["walks"] for t in want))
    for side in (0, 1):
        for why in ("completed", "collision", "bounds", "zero"):
            assert (side, why) in kinds, (side, why, sorted(kinds))
