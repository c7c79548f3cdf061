"""The rules a planner round is planned by (reak_amd/csrc/round_plan.h): the batch rule with the host's bound of it, the
wave fit and the steer launch plan of an Auto round.

tests/cpp/round_plan_test.cpp checks that the batch the device chooses never exceeds the bound the host sizes the round's
grids by, pins the rule at its edges (the wave granule, the clamps and their order), runs the fit over synthetic monotone
wave counts, and walks the steer plan over a grid of thresholds: every edge count a round can have opens exactly one
launched gate, and the default configuration's plans are pinned.  It is compiled by the host compiler with
AddressSanitizer and UBSan and run directly.  No GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_round_plan_rules_under_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "round_plan_test.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "round_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "reak_amd", "csrc"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "round plan ok:" in out.stdout
