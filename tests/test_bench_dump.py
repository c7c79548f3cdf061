"""bench.py --dump-outputs without a GPU: rrt_outputs / write_outputs on a stand-in for RrtPlannerPool with the C2
benchmark's sizes (512 problems x 100 001 vertices of 12-D states).  The files must be finite float64, within the 64 MB
limit, the same on every call, and the sampled rows must be the trees' own rows."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


class _Stats:
    def __init__(self, p, nv, it):
        self.num_vertices, self.iterations, self.edges_checked = nv, it, 2 * it
        self.num_solutions, self.best_cost = p % 3, (np.inf if p % 3 == 0 else 1.0 + p)
        self.edges_speculated, self.rounds, self.done = 3 * it, 7, 1


class _Pool:
    """RrtPlannerPool's read-back interface (P, D, all_stats, solution, tree); problem 0 is a tree of its root alone."""

    def __init__(self, P, nv, it, D=12):
        self.P, self.D = P, D
        self.all_stats = [_Stats(p, nv if p else 1, it if p else 0) for p in range(P)]

    def solution(self, p):
        return np.arange(5 * self.all_stats[p].num_solutions, dtype=np.uint32), 1.0

    def tree(self, p):
        nv, it = self.all_stats[p].num_vertices, self.all_stats[p].iterations
        rng = np.random.default_rng(p)
        parent = rng.integers(0, nv, nv).astype(np.uint32)
        parent[0] = 0xFFFFFFFF
        return {"pos": rng.random((nv, self.D)), "parent": parent, "nn_seq": rng.integers(0, nv, it).astype(np.uint32),
                "accept": rng.integers(0, 2, it).astype(np.uint8), "goal_dist": rng.random(nv - 1)}


def _dump(pool, d):
    bench.write_outputs(str(d), bench.rrt_outputs(pool))
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_at_benchmark_size_is_bounded_float64_and_repeatable(tmp_path):
    pool = _Pool(512, 100001, 180000)
    a, b = _dump(pool, tmp_path / "a"), _dump(pool, tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= bench.DUMP_LIMIT_BYTES
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in a.values())
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert len(a["num_vertices"]) == 512 and len(a["sample_problems"]) == bench.DUMP_PROBLEMS
    for p in a["sample_problems"].astype(int):
        t, rows, its = pool.tree(p), a["tree_problem"] == p, a["iter_problem"] == p
        v, i = a["tree_vertex"][rows].astype(int), a["iter_index"][its].astype(int)
        assert np.array_equal(a["tree_pos"][rows], t["pos"][v]) and np.array_equal(a["tree_parent"][rows], t["parent"][v])
        gd = np.concatenate([[np.nan], t["goal_dist"]])[v]
        assert np.array_equal(a["tree_goal_dist"][rows], np.nan_to_num(gd, nan=0.0))
        assert np.array_equal(a["tree_goal_dist_nonfinite"][rows], np.where(v == 0, 3.0, 0.0))
        assert np.array_equal(a["iter_nn"][its], t["nn_seq"][i]) and np.array_equal(a["iter_accept"][its], t["accept"][i])


def test_dump_of_small_runs(tmp_path):
    """Fewer problems than the sample, a tree of its root alone, problems without a solution."""
    a = _dump(_Pool(3, 50, 80), tmp_path)
    assert np.array_equal(a["sample_problems"], [0, 1, 2]) and np.array_equal(a["solution_length"], [0, 5, 10])
    assert a["solution_path"].shape == (3, 10) and (a["solution_path"][0] == -1).all()
    root = a["tree_vertex"] == 0
    assert (a["tree_goal_dist_nonfinite"][root] == 3).all() and (a["tree_goal_dist"][root] == 0).all()
    assert (a["iter_problem"] != 0).all()
    assert np.array_equal(a["best_cost"], [0.0, 2.0, 3.0]) and np.array_equal(a["best_cost_nonfinite"], [1.0, 0.0, 0.0])


def test_nonfinite_values_are_split_and_refused_unsplit(tmp_path):
    got = bench.split_nonfinite("x", [1.5, np.inf, -np.inf, np.nan])
    assert np.array_equal(got["x"], [1.5, 0, 0, 0]) and np.array_equal(got["x_nonfinite"], [0, 1, 2, 3])
    with pytest.raises(RuntimeError, match="non-finite"):
        bench.write_outputs(str(tmp_path), {"x": [1.0, np.inf]})
