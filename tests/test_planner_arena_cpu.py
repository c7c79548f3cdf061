"""The layout of a batch planner's arena (reak_amd/csrc/arena_layout.h) is a pure host function: tests/cpp/
arena_layout_test.cpp calls it for 1, 3 and 65 problems, mixed vertex budgets (1, 255, 256, 257, 2000), mirror and
profile on and off, 3, 6 and 12 dimensions, and checks alignment, disjointness, the guard tail, the total and
determinism.  The program is compiled by the host compiler with AddressSanitizer and UBSan and run directly.  No GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arena_layout_under_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "arena_layout_test.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "arena_layout_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "reak_amd", "csrc"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "arena layout ok: 72 shapes" in out.stdout
