"""The round-carry rule (reak_amd/csrc/round_carry.h): a round of the speculative-batch RRT driver reuses the steered edge
of a candidate the round before discarded when the fresh nearest neighbour is the vertex that edge started from.

tests/cpp/round_carry_test.cpp pins the header at its edges (slot mapping, carried count, clipping to the new batch, the
predicate with a changed index at slot 0 / in the middle / at the last carried slot, b_max, the gate) and the arena
layout's invariants with the stash ranges; it is compiled by the host compiler with AddressSanitizer and UBSan and run
directly.  The numpy test replays the round protocol over the sequential golden runs and checks the premise the feature
rests on: most discarded candidates' true nearest neighbour predates the round.  No GPU."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_round_carry_rule_under_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "round_carry_test.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "round_carry_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "reak_amd", "csrc"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "round carry ok:" in out.stdout


# ---- the header's rule, restated -----------------------------------------------------------------------------------
def carry_count(b_old, cut, valid=True):
    return b_old - cut if valid and cut < b_old else 0


def carry_usable(carried, b_new):
    return min(carried, b_new)


def simulate_rounds(nn_seq, accept, batch_factor, b_min=8, b_max=1024):
    """The driver's rounds over one sequential run (planner.hip): a round that starts with n vertices at sample s0 takes
    B = clamp(floor(batch_factor sqrt(n)), b_min, b_max) candidates (at most what the recorded run has left); candidate b
    is valid iff its true nearest neighbour nn_seq[s0 + b] is a snapshot vertex (< n); the round consumes the candidates
    before the first invalid one.  Returns (steered, discarded, certain, reused_lb):
      certain    discarded candidates whose true nearest neighbour predates the round that discarded them -- their
                 snapshot nearest neighbour is the true one in that round and in the next, so the predicate holds
      reused_lb  those of them the next round can look at (slot below min(carried, B_new)): a lower bound of what the
                 device reuses (it also reuses a candidate whose two snapshot neighbours agree without being the true one)
    """
    iterations = len(nn_seq)
    n, s0 = 1, 0
    steered = discarded = certain = reused_lb = 0
    carried, carried_n = 0, 0  # the stash: candidates [s0, s0 + carried) steered against a snapshot of carried_n vertices
    while s0 < iterations:
        B = min(max(int(np.float32(batch_factor) * np.float32(math.sqrt(n))), b_min), b_max, iterations - s0)
        nn = nn_seq[s0:s0 + B].astype(np.int64)
        usable = carry_usable(carried, B)
        reused_lb += int(np.count_nonzero(nn[:usable] < carried_n))
        invalid = np.nonzero(nn >= n)[0]
        cut = int(invalid[0]) if len(invalid) else B
        assert cut >= 1  # the first candidate of a round sees the whole tree
        steered += B
        carried, carried_n = carry_count(B, cut), n
        discarded += carried
        certain += int(np.count_nonzero(nn[cut:] < n))
        n += int(accept[s0:s0 + cut].sum())
        s0 += cut
    return steered, discarded, certain, reused_lb


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "c2_golden.npz"))


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("batch_factor", [1.25, 4.0])
def test_most_discarded_candidates_keep_their_nearest_neighbour(golden, seed, batch_factor):
    nn_seq, accept = golden[f"rrt{seed}_nn_seq"], golden[f"rrt{seed}_accept"]
    steered, discarded, certain, reused_lb = simulate_rounds(nn_seq, accept, batch_factor)
    print(f"seed {seed} factor {batch_factor}: steered {steered} discarded {discarded} "
          f"({discarded / steered:.3f}) certain {certain} ({certain / discarded:.3f}) "
          f"reused at least {reused_lb} ({reused_lb / discarded:.3f})")
    assert discarded > 0
    assert certain >= 0.8 * discarded
    # what the next round can look at of them (the surplus beyond a smaller batch is dropped): the condition
    # tests/test_round_carry_gpu.py sets for the device's counters at batch factor 4 has room below this
    assert reused_lb <= certain
    if batch_factor == 4.0:
        assert reused_lb >= 0.6 * discarded
