"""Generate a kernel-choice fixture: for every case of a case module under tests/ what its run_case returns -- the kernels
the batches launched in the module's stages and the SHA-256 of the tables they returned.

    tests/fir_kernel_choice_cases.py (the default)  -> tests/golden/fir_kernel_choice.json    (one-wave FIR kernels)
    tests/burst_kernel_choice_cases.py              -> tests/golden/burst_kernel_choice.json  (bursts chain, sharp waves)
    tests/state_blob_cases.py                       -> tests/golden/state_blob.json           (state blobs; --emu: state_blob_emu.json)
    tests/prep_stage_cases.py                       -> tests/golden/prep_stage.json           (a chunk's launch sequence; --emu: prep_stage_emu.json)
    tests/chunk_schedule_cases.py                   -> tests/golden/chunk_schedule.json       (streams and events of a chunk and a batch; --emu: chunk_schedule_emu.json)

Runs on the GPU, at the commit whose kernel choice is to be kept (the parent of a change to how those kernels are chosen);
tests/test_fir_kernel_choice_gpu.py / tests/test_burst_kernel_choice_gpu.py compare a later build against the file.  Every
case runs twice on fresh engines and must repeat itself bit for bit before it is written.

    python tests/golden/make_fir_kernel_choice.py [--emu] [output.json | case module [output.json]]

--emu records with the logic emulator (tests/emu), on a machine without a GPU, into <name>_emu.json: what the CPU tier compares.
"""

from __future__ import annotations

import importlib
import json
import os
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from py_neuromodulation_amd import _lib  # noqa: E402


def main(out: Path, cases, emu: bool = False) -> None:
    if emu:
        import __graft_entry__ as ge

        lib = _lib.NmxLibrary(ge.build_emu())
    else:
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
    args = sys.argv[1:]
    emu = "--emu" in args
    args = [a for a in args if a != "--emu"]
    module = args.pop(0) if args and not args[0].endswith(".json") else "fir_kernel_choice_cases"
    main(Path(args[0]) if args else HERE / (module[:-len("_cases")] + ("_emu" if emu else "") + ".json"),
         importlib.import_module("tests." + module), emu)
