"""nmx_merge_into_tiled (nmx_k_bursts.h: the in-place merge of a top-K list beyond 65 536 entries, tile by tile from the tail)
against std::merge + truncate.  tests/cpp/burst_tiled_merge.cpp compiles the kernel's source single-threaded (tiles of 8
entries) with the address and undefined-behaviour sanitizers: random lists, lists of equal values, new samples above the head /
below the tail / inside one tile, list lengths and capacities one below, at and one above a tile multiple, and merges that
cross the capacity.  Host only."""

import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_tiled_merge_equals_std_merge(tmp_path):
    exe = tmp_path / "burst_tiled_merge"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "burst_tiled_merge.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
