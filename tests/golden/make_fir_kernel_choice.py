"""Generate tests/golden/fir_kernel_choice.json: for every case of tests/fir_kernel_choice_cases.py the kernels a batch
launched in stages 1, 3 and 6 and the SHA-256 of the table it returned.

Runs on the GPU, at the commit whose kernel choice is to be kept (the parent of a change to how the one-wave FIR kernels
are chosen); tests/test_fir_kernel_choice_gpu.py compares a later build against the file.  Every case runs twice on fresh
engines and must repeat itself bit for bit before it is written.

    python tests/golden/make_fir_kernel_choice.py [output.json]
"""

from __future__ import annotations

import json
import os
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from py_neuromodulation_amd import _lib  # noqa: E402
from tests import fir_kernel_choice_cases as cases  # noqa: E402


def main(out: Path) -> None:
    lib = _lib.get_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    table = {}
    for name in cases.CASES:
        first = cases.run_case(lib, name, os.environ.__setitem__, os.environ.__delitem__)
        again = cases.run_case(lib, name, os.environ.__setitem__, os.environ.__delitem__)
        assert first == again, f"{name} does not repeat itself: {first} / {again}"
        table[name] = first
        print(name, json.dumps(first), flush=True)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(table, indent=1) + "\n")


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "fir_kernel_choice.json")
