"""The threshold walk's schedule is a pure function of plan constants (nmx_k_bursts.h: nmx_burst_walk_plan; nmx_k_burst_fill.h:
nmx_burst_walk_schedule).  tests/cpp/burst_walk_schedule.cpp carries a transliteration of the launch-time logic it replaced --
the predicate, the two search loops of run_chunk and the launchers' re-tests -- and compares the two segment for segment
over a grid of windows, overlaps, ring lengths, percentiles, selectors, stream ages and chunk sizes.  Host only."""

import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_schedule_equals_the_launch_time_logic(tmp_path):
    exe = tmp_path / "burst_walk_schedule"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "burst_walk_schedule.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
