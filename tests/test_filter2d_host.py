"""
csrc/trace_filter2d.h on the host: tests/filter2d_host/filter2d_main.cpp (its own main) compiled
with g++ and the address and undefined-behaviour sanitizers, and run once per family.  The program
compares the float32 bounding-circle filter of the 2-D trace with the exact float64 test it stands
in front of (exact_segment / exact_arc_hit, which test_host_math.py pins to the oracle bit for
bit), with zero tolerance: a pair the exact test accepts passes `touches` for its entry and
`touches_cluster` for the full and the padded clusters that hold it; a lane without a valid ray
passes nothing.  Families: offsets up to 1e6 sizes, scales 1e-6 .. 1e6, grazing lines, the tangent
snap's miss distance, arc shapes, degenerate primitives, mixed clusters, float32 / float16 state,
and far ray starts.  No GPU.

(trace_math.h switches contraction off with a clang pragma that g++ does not know: hence
-Wno-unknown-pragmas and -ffp-contract=off next to the flags of test_wave_schedule_host.py.)
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorflowraytrace_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "filter2d_host", "filter2d_main.cpp")

FAMILIES = ("offset", "scale", "grazing", "tangent_snap", "arc_shapes", "degenerate",
            "mixed_clusters", "rounded_state", "far_start")
MIN_EXACT_VALID = 1000


def test_filter2d_never_rejects_what_the_exact_test_accepts(tmp_path):
    exe = tmp_path / "filter2d_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, MAIN, "-o", str(exe)], check=True)
    failures = []
    for family in FAMILIES:
        for seed in (1, 2):
            run = subprocess.run([str(exe), family, str(seed)], capture_output=True, text=True)
            print(run.stdout, run.stderr)
            m = re.search(r"^family (\S+) seed (\d+) pairs (\d+) exact_valid (\d+) .* violations (\d+)$",
                          run.stdout, re.M)
            if run.returncode != 0 or m is None:
                failures.append(f"{family} seed {seed}: exit {run.returncode}\n{run.stdout}{run.stderr}")
                continue
            assert m.group(1) == family and int(m.group(2)) == seed
            if int(m.group(5)) != 0:
                failures.append(f"{family} seed {seed}: {m.group(5)} violations\n{run.stdout}")
            if int(m.group(4)) < MIN_EXACT_VALID:
                failures.append(f"{family} seed {seed}: only {m.group(4)} exact-valid pairs")
    assert not failures, "\n".join(failures)


def test_filter2d_program_rejects_an_unknown_family(tmp_path):
    """The family name is checked: a typo must not pass as an empty, violation-free run."""
    exe = tmp_path / "filter2d_main"
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", CSRC,
                    MAIN, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe), "no_such_family", "1"], capture_output=True, text=True)
    assert run.returncode == 2 and "unknown family" in run.stderr
