"""round_begin_kernel keeps the inputs of the batch rule and its three prefix scans in LDS for up to 1024 problems; a
planner with more problems takes every value from global memory instead.  1025 problems of 24 vertices in C2 run those
rounds (about 8 k edges each: the whole-edge two-lanes launch), with the wave fit on and off.  Results do not depend on
the batches, so problems 0, 512 and 1024 must come out bit for bit as from a three-problem planner given the same three
parameter sets."""
import contextlib
import os

import numpy as np
import pytest

from reak_amd import scenarios

pytestmark = pytest.mark.gpu

_KNOBS = ("RKH_BATCH_MAX", "RKH_WAVE_FIT")
_PICK = (0, 512, 1024)


@contextlib.contextmanager
def _environment(env):
    saved = {k: os.environ.pop(k, None) for k in _KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in _KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _run(L, scene, prms, env, pick):
    with _environment(env):
        pl = L.RrtPlanner(scene, prms)
        pl.solve_planning_query()
        out = [((int(pl.all_stats[i].num_vertices), int(pl.all_stats[i].iterations)), pl.tree(i)) for i in pick]
        rounds = int(pl.all_stats[0].rounds)
        pl.close()
    return out, rounds


@pytest.fixture(scope="module")
def setup():
    from reak_amd import lib as L

    c2 = scenarios.make_c2(world_seed=1)
    scene = L.Scene(L.Context(0), c2)
    prms = [c2.rrt_params(seed=s, max_vertices=24) for s in range(1, 1026)]
    reference, _ = _run(L, scene, [prms[i] for i in _PICK], {"RKH_BATCH_MAX": "16"}, range(3))
    return L, scene, prms, reference


@pytest.mark.parametrize("fit", [None, "0"], ids=["wave fit on", "wave fit off"])
def test_more_problems_than_the_lds_cache_holds_give_the_same_trees(setup, fit):
    L, scene, prms, reference = setup
    env = {"RKH_BATCH_MAX": "16"} if fit is None else {"RKH_BATCH_MAX": "16", "RKH_WAVE_FIT": fit}
    got, rounds = _run(L, scene, prms, env, _PICK)
    print(f"1025 problems, fit {fit}: {rounds} rounds, problem 0: {got[0][0]}")
    for i, ((counts, tree), (ref_counts, ref_tree)) in enumerate(zip(got, reference)):
        assert counts == ref_counts, (_PICK[i], counts, ref_counts)
        assert counts[0] == 25  # the vertex budget and the root
        for key in ("parent", "nn_seq", "accept", "pos"):
            assert np.array_equal(tree[key], ref_tree[key]), (_PICK[i], key)
