"""
csrc/wave_schedule.h on the host: tests/wave_schedule_host/wave_schedule_main.cpp (its own main)
compiled with g++ and the address and undefined-behaviour sanitizers, and run.  The program checks
the schedule's definition -- a permutation of the groups, the heaviest class first, ascending
indices inside a class, equal to a stable sort by descending class -- on random count rows, equal
costs (the identity), rows that are all zero, one outlier cost, for 1, 63, 64, 65 and 15,625
wavefronts, one and two to a group.  No GPU.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "wave_schedule_host", "wave_schedule_main.cpp")


def test_wave_schedule_header_under_sanitizers(tmp_path):
    exe = tmp_path / "wave_schedule_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, MAIN,
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
