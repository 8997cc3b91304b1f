"""
csrc/trace_math.h's next_up_f on the host: tests/next_up_host/next_up_main.cpp (its own main)
compiled with g++ and the address and undefined-behaviour sanitizers, and run.  The program compares
next_up_f(x) with std::nextafterf(x, +infinity) bit for bit: +-0, +-the smallest subnormal,
+-FLT_MIN, +-1, +-FLT_MAX, +-infinity, a NaN, and 10^6 random bit patterns.  No GPU.
(trace_math.h switches contraction off with a clang pragma that g++ does not know: hence
-Wno-unknown-pragmas and -ffp-contract=off, as in test_filter2d_host.py.)
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "next_up_host", "next_up_main.cpp")


def test_next_up_equals_nextafterf_towards_infinity(tmp_path):
    exe = tmp_path / "next_up_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, MAIN,
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
