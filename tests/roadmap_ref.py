"""Reference side of the roadmap queries (rkh_prm_shortest_paths, rkh_prm_get_solution, rkh_prm_query_paths, rkh_diag_sssp):
a plain-Python heapq Dijkstra over an edge list with seed lists, the predecessor rule of include/rkh.h applied as a pass
after the search, the predecessor walk, the goal-side rule of a multi-query, and a query's connections built from the
oracle's k-NN and quasi-static walk with can_be_connected and the edge weight restated here.  Also the graph families
the tests share and the numpy pull iteration the device kernel's argument rests on.  No GPU."""
import heapq
import math

import numpy as np

NIL = 0xFFFFFFFF
QUERY_POINT = 0xFFFFFFFE   # RKH_PRM_QUERY_POINT
INF = float("inf")


def adjacency(n, edge_u, edge_v, edge_w):
    adj = [[] for _ in range(n)]
    for u, v, w in zip(edge_u, edge_v, edge_w):
        u, v, w = int(u), int(v), float(w)
        adj[u].append((v, w))
        adj[v].append((u, w))
    return adj


def csr(n, edge_u, edge_v, edge_w):
    """(row_ptr, col, w) of the undirected graph, neighbours in edge-list order."""
    adj = adjacency(n, edge_u, edge_v, edge_w)
    row_ptr = np.zeros(n + 1, dtype=np.uint32)
    row_ptr[1:] = np.cumsum([len(a) for a in adj])
    col = np.array([v for a in adj for v, _ in a], dtype=np.uint32)
    w = np.array([x for a in adj for _, x in a], dtype=np.float64)
    return row_ptr, col, w


def dijkstra(adj, seeds):
    """dist from the seed list [(vertex, initial distance)]: left-to-right fp64 sums, strict comparisons."""
    d = [INF] * len(adj)
    pq = []
    for v, w in seeds:
        if w < d[v]:
            d[v] = w
            heapq.heappush(pq, (w, v))
    while pq:
        du, u = heapq.heappop(pq)
        if du > d[u]:
            continue
        for v, w in adj[u]:
            nd = du + w
            if nd < d[v]:
                d[v] = nd
                heapq.heappush(pq, (nd, v))
    return d


def predecessors(adj, seeds, d, mark):
    """The rule of include/rkh.h, from the distances alone: the lowest u among v's edges with d[u] + w == d[v]; a vertex
    whose seed is its distance gets `mark`; unreached vertices NIL."""
    pred = [NIL] * len(adj)
    for v in range(len(adj)):
        if d[v] == INF:
            continue
        for u, w in adj[v]:
            if u < pred[v] and d[u] + w == d[v]:
                pred[v] = u
    for v, w in seeds:
        if w == d[v]:
            pred[v] = mark
    return pred


def search(adj, seeds, mark):
    d = dijkstra(adj, seeds)
    return np.array(d, dtype=np.float64), np.array(predecessors(adj, seeds, d, mark), dtype=np.uint32)


def vertex_search(adj, s):
    return search(adj, [(int(s), 0.0)], NIL)


def walk(pred, last):
    """The predecessor walk from `last`, in travel order (ends at the vertex whose predecessor is NIL or QUERY_POINT)."""
    rev, v = [], int(last)
    while v < len(pred) and len(rev) < len(pred):
        rev.append(v)
        v = int(pred[v])
    return rev[::-1]


def goal_side(d, conns):
    """min over the accepted goal connections (v, w) of d[v] + w, the lowest v winning ties: (v or NIL, cost)."""
    best, cost = NIL, INF
    for v, w in conns:
        t = float(d[v]) + w
        if t == INF:
            continue
        if t < cost or (t == cost and v < best):
            best, cost = v, t
    return best, cost


def pull_iteration(n, adj, seeds):
    """The device kernel's relaxation as a numpy Jacobi iteration: every round v takes min(seed[v], min d[u] + w), strict <;
    stops at the round that changes nothing.  Returns (dist, rounds)."""
    d = np.full(n, np.inf)
    for v, w in seeds:
        d[v] = min(d[v], w)
    rounds = 0
    while True:
        nd = d.copy()
        for v in range(n):
            for u, w in adj[v]:
                c = d[u] + w
                if c < nd[v]:
                    nd[v] = c
        rounds += 1
        if np.array_equal(nd, d) or rounds > n:
            return nd, rounds
        d = nd


# ---- the connections of a multi-query, from the oracle
def _euclid(a, b):
    r = 0.0
    for x, y in zip(a, b):          # left-to-right sum of squares, as the kernels and the planners sum it
        df = float(x) - float(y)
        r += df * df
    return math.sqrt(r)


def connections(oracle_lib, osc, lower, upper, min_interval, conn_tol, pos, point, k, radius, towards_roadmap):
    """Accepted connections [(vertex, weight)] of one query point: its k nearest roadmap vertices strictly inside radius
    (ascending (distance, index)), each walked in the direction of travel -- point -> u (towards_roadmap) or u -> point --
    judged by can_be_connected (planning_visitors.hpp:385-395) and weighted |first point of the walk - its end|.  A
    coincident vertex connects with weight 0."""
    idx, dist, cnt = oracle_lib.knn(np.asarray(point, dtype=np.float64).reshape(1, -1), pos, k, radius)
    out = []
    for e in range(min(int(cnt[0]), k)):
        u = int(idx[0, e])
        if dist[0, e] == 0.0:
            out.append((u, 0.0))
            continue
        a, b = (point, pos[u]) if towards_roadmap else (pos[u], point)
        res, _ = osc.qs_move(lower, upper, min_interval, a, b)
        n_ar, n_rb = _euclid(a, res[0]), _euclid(res[0], b)
        if (not math.isinf(n_ar)) and n_rb < conn_tol * n_ar:
            out.append((u, n_ar))
    return out


def query(adj, start_conns, goal_conns):
    """(cost, path) of one multi-query from its accepted connections."""
    d, pred = search(adj, start_conns, QUERY_POINT)
    last, cost = goal_side(d, goal_conns)
    return (cost, walk(pred, last)) if last != NIL else (INF, [])


# ---- graph families (edge lists) shared by the CPU self-check and the GPU tests
def path_graph(n, rng=None):
    w = np.ones(n - 1) if rng is None else rng.uniform(0.1, 1.0, n - 1)
    return n, np.arange(n - 1), np.arange(1, n), w


def star_graph(n, rng):
    return n, np.full(n - 1, n - 1), np.arange(n - 1), rng.uniform(0.1, 1.0, n - 1)   # the centre is the last vertex


def two_components(rng):
    n1, u1, v1, w1 = path_graph(40, rng)
    n2, u2, v2, w2 = path_graph(33, rng)
    return n1 + n2, np.concatenate([u1, u2 + n1]), np.concatenate([v1, v2 + n1]), np.concatenate([w1, w2])


def zero_weight_graph(rng):
    """a ring of 70 with chords, where vertices 5 / 6 / 7 and 30 / 31 coincide (zero-weight edges)"""
    n = 70
    u = list(range(n)) + [0, 10, 20]
    v = [(i + 1) % n for i in range(n)] + [35, 45, 55]
    w = list(rng.uniform(0.1, 1.0, n)) + [0.7, 0.2, 0.9]
    for i in (5, 6, 30):
        w[i] = 0.0
    return n, np.array(u), np.array(v), np.array(w)


def duplicate_edge_graph(rng):
    n, u, v, w = path_graph(65, rng)
    du, dv = np.array([3, 3, 20, 20, 64]), np.array([4, 4, 40, 40, 0])
    dw = np.array([w[3] * 0.5, w[3] * 2.0, 0.3, 0.1, 5.0])
    return n, np.concatenate([u, du]), np.concatenate([v, dv]), np.concatenate([w, dw])


def knn_graph(n, k, rng, dim=3):
    """random k-NN graph (each of a vertex's k nearest kept with probability 0.7); vertices 3 and 5 coincide"""
    p = rng.uniform(0, 1, (n, dim))
    if n > 5:
        p[5] = p[3]
    eu, ev, ew = [], [], []
    for v in range(n):
        dd = np.sqrt(((p - p[v]) ** 2).sum(1))
        for u in np.argsort(dd, kind="stable")[1:k + 1]:
            if rng.uniform() < 0.7 and int(u) != v:
                eu.append(v), ev.append(int(u)), ew.append(float(dd[u]))
    return n, np.array(eu, dtype=int), np.array(ev, dtype=int), np.array(ew)


def planted_tie_graph(n, k, rng):
    """a k-NN graph of n - 4 vertices plus four vertices lo < a < b < hi with two equal-cost routes planted between a and
    b: a -0.25- hi -0.5- b and a -0.5- lo -0.25- b, through a higher and a lower id, so that the tie rule decides."""
    n0, eu, ev, ew = knn_graph(n - 4, k, rng)
    lo, a, b, hi = n0, n0 + 1, n0 + 2, n0 + 3   # lo < a < b < hi
    pu = [a, hi, a, lo, a]
    pv = [hi, b, lo, b, 0]
    pw = [0.25, 0.5, 0.5, 0.25, 0.125]           # and a bridge into the k-NN graph
    return n, np.concatenate([eu, pu]).astype(int), np.concatenate([ev, pv]).astype(int), np.concatenate([ew, pw]), (a, b, lo, hi)


def families(seed=7):
    """name -> (n, edge_u, edge_v, edge_w)"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in (2, 63, 64, 65, 257, 1000):
        out[f"path{n}"] = path_graph(n, rng)
    out["star300"] = star_graph(300, rng)
    out["two_components"] = two_components(rng)
    out["zero_weight"] = zero_weight_graph(rng)
    out["duplicate_edges"] = duplicate_edge_graph(rng)
    out["knn1500_tie"] = planted_tie_graph(1500, 8, rng)[:4]
    return out
