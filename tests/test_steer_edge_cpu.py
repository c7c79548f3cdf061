"""The per-edge protocol of the steer and edge-walk kernels (reak_amd/csrc/steer_edge.h) is plain host-and-device code:
tests/cpp/steer_edge_test.cpp pins each rule at its edges with hand-worked values -- the gate, the segment bisection over
prefixes with empty segments, the source / target rows, the per-edge step count, the PD law's saturation, the hyperbox
test with both orders of the bounds, one RK4 step of rk4_stage against the unrolled expression, every accept rule at
its tolerance, and the two goal-probe rules at equality.  The program is compiled by the host compiler with
AddressSanitizer and UBSan and run directly.  No GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_steer_edge_protocol_under_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "steer_edge_test.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "steer_edge_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "reak_amd", "csrc"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "steer edge protocol ok:" in out.stdout
