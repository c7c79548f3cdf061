"""The fix-up that stages accepted end states in LDS (fixup_tiled_kernel, reak_amd/csrc/planner.hip) against the
one-wave-per-candidate kernel it replaces (RKH_FIXUP_TILED=0): the trees of a batch RRT are bit for bit the same.

A block of the tiled kernel takes 64 candidates and walks the rows below them in tiles of 256 (state dimensions up to
16).  The batch size of every round is forced (tests/fixup_worker.py) to the edges of both tiles: 63, 64, 65 candidates
(one tile less one, one tile, a second tile of one candidate) and 256, 257, 258 (255, 256, 257 rows below the last
candidate: a row tile less one, one tile, a second tile of one row), and to 1 -- no row below the only candidate, and
a round whose candidate is rejected is a round with no accepted candidate.  Three scenes, three problems each: C1 in
its quasi-static space (3 coordinates, rows padded to 4), the planar C1 arm with dynamics (6 state dimensions), C2 (12).
Every row is at most 16 coordinates wide, so the row tile is always 256: the 128-row tile of the kernel's forms for 24 and
32 coordinates (and its `tid < TR` guard) is NOT exercised here -- no scene of the project has a state that wide (the
dynamics kernels stop at 6 joints, the quasi-static ones at 12 coordinates).  That a round really takes B candidates is
checked on the planner's counter of speculated edges, less its goal probes: a round takes B unless the uploaded samples run short.
The planner reads its switches at creation, so each switch setting runs in a fresh child process (one per scene and
setting, all batch sizes in it).  The C2 runs are those of tests/golden/c2_golden.npz, problem 0 of the
C1 runs that of c1_golden.npz."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 63, 64, 65, 256, 257, 258)
SCENES = {"c1": 800, "c1_planar_dyn": 600, "c2": 1500}  # max_vertices
_KNOBS = ("RKH_FIXUP_TILED", "RKH_BATCH_FACTOR", "RKH_BATCH_MAX", "RKH_BATCH_MIN", "RKH_WAVE_FIT")


def _child(tmp, scene, tiled):
    out = os.path.join(tmp, f"{scene}_{tiled}.npz")
    env = {k: v for k, v in os.environ.items() if k not in _KNOBS}
    env["RKH_WAVE_FIT"] = "0"  # (the wave fit scales a round's batch: off, every round takes exactly B)
    if tiled is not None:
        env["RKH_FIXUP_TILED"] = tiled
    cmd = [sys.executable, os.path.join(ROOT, "tests", "fixup_worker.py"), scene, str(SCENES[scene]), out]
    run = subprocess.run(cmd + [str(b) for b in BATCHES], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("fixup"))
    return {(scene, tiled): _child(tmp, scene, tiled) for scene in SCENES for tiled in (None, "0")}


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("scene", list(SCENES))
def test_tiled_fixup_gives_the_same_trees(runs, scene, B):
    on, off = runs[(scene, None)], runs[(scene, "0")]
    for i in range(3):
        counts = on[f"b{B}_p{i}_counts"]
        assert np.array_equal(counts, off[f"b{B}_p{i}_counts"])
        assert counts[0] > SCENES[scene] // 2  # a tree was grown
        for key in ("nn_seq", "accept", "parent", "pos"):
            a, b = on[f"b{B}_p{i}_{key}"], off[f"b{B}_p{i}_{key}"]
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (scene, B, i, key)
        if B == 1:  # one candidate per round: a rejected one is a round without an accepted candidate
            assert counts[4] == counts[1] and np.count_nonzero(on[f"b{B}_p{i}_accept"] == 0) > 0
        else:
            assert counts[4] < counts[1]  # rounds < iterations: rounds did take several candidates
        # candidates steered = the sum of the rounds' batch sizes: B in every round but the few the sample stream cut
        # (edges_speculated also counts one goal probe per committed vertex)
        rounds, steered = int(counts[4]), int(counts[5]) - (int(counts[0]) - 1)
        print(f"{scene} B={B} problem {i}: {rounds} rounds, {steered} candidates, {steered / (rounds * B):.4f} of rounds x B")
        assert rounds >= 2 and (rounds - 2) * B < steered <= rounds * B


@pytest.mark.parametrize("B", BATCHES)
def test_c2_trees_are_the_sequential_planner_s(runs, B):
    g = np.load(os.path.join(ROOT, "tests", "golden", "c2_golden.npz"))
    for tiled in (None, "0"):
        run = runs[("c2", tiled)]
        for i, seed in enumerate((1, 2, 3)):
            assert list(run[f"b{B}_p{i}_counts"][:4]) == [int(v) for v in g[f"rrt{seed}_counts"]]
            for key in ("nn_seq", "accept", "parent"):
                assert np.array_equal(run[f"b{B}_p{i}_{key}"], g[f"rrt{seed}_{key}"]), (B, seed, key)
            assert np.allclose(run[f"b{B}_p{i}_pos"], g[f"rrt{seed}_pos"], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("B", BATCHES)
def test_c1_tree_is_the_sequential_planner_s(runs, B):
    g = np.load(os.path.join(ROOT, "tests", "golden", "c1_golden.npz"))
    for tiled in (None, "0"):
        run = runs[("c1", tiled)]
        assert list(run[f"b{B}_p0_counts"][:4]) == [int(v) for v in g["rrt_counts"]]
        for key in ("accept", "parent", "pos"):
            assert np.array_equal(run[f"b{B}_p0_{key}"], g[f"rrt_{key}"]), (B, key)
