"""Plain-Python twin of rkh_svp_shortcut_paths as include/rkh.h defines it: the pair order of tests/shortcut_ref.py, the
reach time and the walk of tests/svp_ref.py, and the sequential double loop of the search with weights that may be +inf
and a goal that may be out of reach (shortcut_ref.dp's predecessor walk would not end there).  Shared by
tests/test_svp_shortcut_cpu.py (which checks the loop against a brute force over all subsequences) and
tests/test_svp_shortcut_gpu.py."""
import itertools

import shortcut_ref as S
import svp_ref as R

NIL = S.NIL
INF = R.INF


def search(L, max_span, ok, w):
    """The search on verdicts / weights given per candidate pair, in pair order.  Returns (keep, time_out, n_blocked);
    ([], inf, 0) when no allowed hop sequence reaches the goal."""
    s = S.span_of(L, max_span)
    idx = {p: k for k, p in enumerate(S.pairs(L, max_span))}
    dist = [INF] * L
    pred = [NIL] * L
    dist[0] = 0.0
    for i in range(L):
        for j in range(i + 1, min(i + s, L - 1) + 1):
            k = idx[(i, j)]
            if j == i + 1 or ok[k]:
                c = dist[i] + float(w[k])     # that one fp64 addition; x + inf < y is never true
                if c < dist[j]:               # strict <, i ascending: the lowest i wins ties
                    dist[j], pred[j] = c, i
    if not (dist[L - 1] < INF):
        return [], INF, 0
    keep = [L - 1]
    while keep[-1] != 0:
        keep.append(pred[keep[-1]])
    keep.reverse()
    n_blocked = sum(1 for u, v in zip(keep[:-1], keep[1:]) if not ok[idx[(u, v)]])
    return keep, dist[L - 1], n_blocked


def time_in(L, max_span, w):
    """the left-to-right sum of the consecutive hops' weights"""
    idx = {p: k for k, p in enumerate(S.pairs(L, max_span))}
    t = 0.0
    for v in range(L - 1):
        t = t + float(w[idx[(v, v + 1)]])
    return t


def brute_force(L, max_span, ok, w):
    """(time, keep) of the best subsequence 0 = v_0 < ... < v_m = L - 1 whose hops are all allowed and finite in sum,
    with the key order of shortcut_ref.brute_force: the left-to-right sum, then the lowest predecessor from the goal
    backwards.  (inf, []) when there is none.  Exponential: L <= 10."""
    s = S.span_of(L, max_span)
    idx = {p: k for k, p in enumerate(S.pairs(L, max_span))}
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
            if not fine or not (cost < INF):
                continue
            key = (cost, tuple(reversed(seq)))
            if best is None or key < best:
                best = key
    if best is None:
        return INF, []
    return best[0], list(reversed(best[1]))


def pair_rows(path, max_span):
    """(a, b): the rows of the candidate pairs of `path` in pair order, as lists"""
    pr = S.pairs(len(path), max_span)
    return [list(path[i]) for i, _ in pr], [list(path[j]) for _, j in pr]


def from_walks(L, max_span, T, reached):
    """What the entry must return for one path, from the reach time and the `reached` byte of the walk of every candidate
    pair: dict(keep, time_in, time_out, n_blocked)."""
    keep, t_out, n_blocked = search(L, max_span, reached, T)
    return {"keep": keep, "time_in": time_in(L, max_span, T), "time_out": t_out, "n_blocked": n_blocked}


def reference(sp, path, max_span, is_free):
    """One path with the twin's own walk (svp_ref.edge_walk, fraction 1, is_free(x) the collision part)."""
    a, b = pair_rows(path, max_span)
    walks = [R.edge_walk(sp, x, y, 1.0, is_free) for x, y in zip(a, b)]
    return from_walks(len(path), max_span, [w[1] for w in walks], [w[3] for w in walks])
