"""StagedCall (reak_amd/csrc/staged_call.h) owns the transfers around the launch of every one-shot entry point.  tests/cpp/
staged_call_test.cpp runs a representative call over a fake HIP runtime (tests/cpp/hip_fake) that defers every asynchronous
copy and fill until the stream is waited for: once clean, once with the launcher refusing, then with each of its runtime
calls failing in turn.  It checks the outputs, the exact allocations and copies, the latched status, that nothing is
enqueued after a failure and that the stream is idle and nothing is live when the scope ends; a path that freed a buffer
or let host memory go with work queued would be a use-after-free.  The program is compiled by the host compiler with
AddressSanitizer and UBSan and run directly.  No GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_staged_call_under_sanitizers():
    src = os.path.join(ROOT, "tests", "cpp", "staged_call_test.cpp")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "staged_call_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tests", "cpp", "hip_fake"),
                        "-I", os.path.join(ROOT, "reak_amd", "csrc"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "staged call ok: 14 runtime calls, each failed once" in out.stdout
