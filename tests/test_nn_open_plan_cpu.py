"""The open rule and the work items of the mirror sweep's second pass (reak_amd/csrc/nn_mirror.h: mirror_open,
mirror_open_item, mirror_open_entry, mirror_open_slot_live).

tests/cpp/nn_open_plan_test.cpp pins them at their edges -- list lengths 0, 1, 32, 33, 384, 385, the last block's group
count and pad slots, the rule at est == thr, +inf, -inf and NaN -- and replays the blocks of a slice over a list: every
entry taken exactly once, no slot reading outside its block's range.  It is compiled by the host compiler with
AddressSanitizer and UBSan and run directly.  No GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_open_plan_under_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "nn_open_plan_test.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "nn_open_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "reak_amd", "csrc"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "nn open plan ok:" in out.stdout
