"""Plain-Python reference of path shortcutting as include/rkh.h defines it at rkh_shortcut_paths: the pair order, the
hop weight, the sequential double loop of the search, the predecessor walk, and `reference()`, which takes the strict
verdicts from the oracle's quasi-static walk (OracleScene.qs_move with fraction 1 returns the target bit for bit).
Shared by tests/test_path_shortcut_cpu.py (which checks the loop against a brute force over all subsequences) and
tests/test_path_shortcut_gpu.py."""
import itertools
import math

import numpy as np

NIL = 0xFFFFFFFF
INF = float("inf")


def span_of(L, max_span):
    return L - 1 if (max_span == 0 or max_span > L - 1) else max_span


def pairs(L, max_span):
    """the candidate pairs of a path of L points in pair order: i ascending, then j ascending, 1 <= j - i <= span"""
    s = span_of(L, max_span)
    return [(i, j) for i in range(L) for j in range(i + 1, min(i + s, L - 1) + 1)]


def weight(a, b):
    """left-to-right fp64 euclidean norm of a - b (s = s + d * d in coordinate order, one correctly rounded sqrt)"""
    s = 0.0
    for x, y in zip(a, b):
        d = float(x) - float(y)
        s = s + d * d
    return math.sqrt(s)


def dp(L, max_span, ok, w):
    """The search on verdicts / weights given per candidate pair, in pair order.  Returns (keep, cost_out, n_blocked)."""
    s = span_of(L, max_span)
    idx = {p: k for k, p in enumerate(pairs(L, max_span))}
    dist = [INF] * L
    pred = [NIL] * L
    dist[0] = 0.0
    for i in range(L):
        for j in range(i + 1, min(i + s, L - 1) + 1):
            k = idx[(i, j)]
            if j == i + 1 or ok[k]:
                c = dist[i] + float(w[k])     # that one fp64 addition
                if c < dist[j]:               # strict <, i ascending: the lowest i wins ties
                    dist[j], pred[j] = c, i
    keep = [L - 1]
    while keep[-1] != 0:
        keep.append(pred[keep[-1]])
    keep.reverse()
    n_blocked = sum(1 for u, v in zip(keep[:-1], keep[1:]) if not ok[idx[(u, v)]])
    return keep, dist[L - 1], n_blocked


def dp_rows(L, max_span, ok, w):
    """dp() with the inner loop over j as one numpy row operation: for a fixed i the updates of different j are
    independent, so the result is the double loop's bit for bit (tests/test_path_shortcut_cpu.py compares them).  For the
    long paths of the GPU tests.  Returns (keep, cost_out, n_blocked)."""
    s = span_of(L, max_span)
    ok = np.asarray(ok, dtype=bool)
    w = np.asarray(w, dtype=np.float64)
    dist = np.full(L, INF)
    pred = np.full(L, NIL, dtype=np.int64)
    dist[0] = 0.0
    base = 0
    row_of = np.zeros(L, dtype=np.int64)
    for i in range(L - 1):
        n = min(s, L - 1 - i)
        row_of[i] = base
        allowed = ok[base:base + n].copy()
        allowed[0] = True                         # j == i + 1
        c = dist[i] + w[base:base + n]
        upd = allowed & (c < dist[i + 1:i + 1 + n])
        dist[i + 1:i + 1 + n][upd] = c[upd]
        pred[i + 1:i + 1 + n][upd] = i
        base += n
    keep = [L - 1]
    while keep[-1] != 0:
        keep.append(int(pred[keep[-1]]))
    keep.reverse()
    n_blocked = sum(1 for u, v in zip(keep[:-1], keep[1:]) if not ok[row_of[u] + (v - u - 1)])
    return keep, float(dist[L - 1]), n_blocked


def brute_force(L, max_span, ok, w):
    """(cost, keep) of the best subsequence 0 = v_0 < ... < v_m = L - 1 whose hops are all allowed: the cost is the
    left-to-right sum of the hop weights; among equal costs the subsequence the tie rule selects (the lowest predecessor
    at the goal, then at that predecessor, ...).  Exponential: L <= 10."""
    s = span_of(L, max_span)
    idx = {p: k for k, p in enumerate(pairs(L, max_span))}
    best = None
    for m in range(0, max(L - 1, 1)):
        for mid in itertools.combinations(range(1, L - 1), m):
            seq = (0,) + mid + ((L - 1,) if L > 1 else ())
            cost, fine = 0.0, True
            for u, v in zip(seq[:-1], seq[1:]):
                if v - u > s or not (v == u + 1 or ok[idx[(u, v)]]):
                    fine = False
                    break
                cost = cost + float(w[idx[(u, v)]])
            if not fine:
                continue
            key = (cost, tuple(reversed(seq)))   # lowest predecessor first, from the goal backwards
            if best is None or key < best:
                best = key
    return best[0], list(reversed(best[1]))


def strict_verdicts(osc, lower, upper, min_interval, path, max_span):
    """(ok, w) per candidate pair of `path` ([L][n] points): w the hop weight, ok the strict verdict of the walk
    p_i -> p_j: w < min_interval, or the oracle's full-fraction walk returns p_j bit for bit."""
    path = np.ascontiguousarray(path, dtype=np.float64)
    pr = pairs(len(path), max_span)
    if not pr:
        return np.zeros(0, dtype=np.uint8), np.zeros(0)
    a = np.array([path[i] for i, _ in pr])
    b = np.array([path[j] for _, j in pr])
    out, _ = osc.qs_move(lower, upper, min_interval, a, b, 1.0)
    w = np.array([weight(x, y) for x, y in zip(a, b)])
    arrived = (out.view(np.uint64) == b.view(np.uint64)).all(axis=1)
    return ((w < min_interval) | arrived).astype(np.uint8), w


def restrict(L, max_span, ok, w):
    """the entries of all-pairs arrays (max_span 0) that are candidates under max_span, in pair order"""
    idx = {p: k for k, p in enumerate(pairs(L, 0))}
    sel = np.array([idx[p] for p in pairs(L, max_span)], dtype=np.int64)
    return np.asarray(ok)[sel], np.asarray(w)[sel]


def reference(osc, lower, upper, min_interval, path, max_span, full=None):
    """What rkh_shortcut_paths must return for one path: dict(keep, cost_in, cost_out, n_blocked, ok, w).  full: the
    (ok, w) of strict_verdicts(..., max_span=0) for this path, if the caller has them already (the walks of a smaller
    span are a subset of them)."""
    path = np.ascontiguousarray(path, dtype=np.float64)
    L = len(path)
    if full is not None:
        ok, w = restrict(L, max_span, *full)
    else:
        ok, w = strict_verdicts(osc, lower, upper, min_interval, path, max_span)
    keep, cost_out, n_blocked = dp(L, max_span, ok, w)
    cost_in = 0.0
    for v in range(L - 1):
        cost_in = cost_in + weight(path[v], path[v + 1])
    return {"keep": keep, "cost_in": cost_in, "cost_out": cost_out, "n_blocked": n_blocked, "ok": ok, "w": w}
