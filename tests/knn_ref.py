"""A plain k-NN reference for rkh_nn_queryk: pure numpy, no oracle, no device code.

The contract (reak_amd/csrc/nn_device.h, include/rkh.h): the squared distance is the left-to-right fp64 sum over the
coordinates of (q[d] - x[d])**2, every product and every sum rounded once; the distance is its correctly rounded square
root; a vertex qualifies with d < radius, strictly; the result is ordered by (distance, index) ascending, cut to k and
padded with 0xFFFFFFFF / +inf.  Removed rows (rkh_nn_remove) are dropped before the search and the indices mapped back.
"""
import numpy as np

PAD_IDX = np.uint32(0xFFFFFFFF)


def distances(q, pts):
    """[B][n] distances of the contract: a Python loop over the D columns with elementwise numpy operations, so every
    product and every sum is one IEEE rounding (no dot product, no fused multiply-add, no pairwise summation)."""
    q = np.asarray(q, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64)
    B, D = q.shape
    n = pts.shape[0]
    s = np.zeros((B, n))
    for d in range(D):
        df = q[:, d][:, None] - pts[:, d][None, :]
        s = df * df if d == 0 else s + df * df
    return np.sqrt(s)


def knn(q, pts, k, radius=np.inf, removed=None):
    """(idx [B][k] uint32, dist [B][k], cnt [B] uint32) of the k nearest rows of pts strictly inside radius.
    removed: indices of rows that were removed (they are never returned)."""
    q = np.asarray(q, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, q.shape[1])
    n = pts.shape[0]
    live = np.ones(n, dtype=bool)
    if removed is not None:
        live[np.asarray(removed, dtype=np.int64)] = False
    rows = np.nonzero(live)[0]  # ascending: the order of the live rows is the order of their indices
    B = q.shape[0]
    idx = np.full((B, k), PAD_IDX, dtype=np.uint32)
    dist = np.full((B, k), np.inf)
    cnt = np.zeros(B, dtype=np.uint32)
    if rows.size == 0:
        return idx, dist, cnt
    d_all = distances(q, pts[rows])
    for b in range(B):
        d = d_all[b]
        inside = np.nonzero(d < radius)[0]
        order = inside[np.lexsort((rows[inside], d[inside]))][:k]  # by distance, then by index
        m = order.size
        idx[b, :m] = rows[order]
        dist[b, :m] = d[order]
        cnt[b] = m
    return idx, dist, cnt
