"""tests/golden/resample_auto_parent.npz: what the resampler with npad = "auto" stored BEFORE the fixed padding mode existed.

Run it on the emulator build of the commit in front of the one that adds ``resample_npad`` (the parent):

    python tests/golden/make_resample_auto_parent.py [path/to/libnmx_emu.so of the parent] [out.npz]

It sends the inputs of four resampler cases of tests/front_probe_cases.py (one-transform even and odd, forced and long
polyphase) through ``HotPathEngine.preprocess_window`` and keeps every output window as the float32 the library stored,
plus the kernel names ``nmx_last_kernels`` reports for stage 1 of such a plan and of a plan without a resampler.
tests/test_resample_npad_cpu.py asserts bit equality with it: an "auto" plan launches what it launched, same bytes out.
The script never names the new keyword, so it runs unchanged on either side of that commit.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

CASES = ["down_even", "up_odd", "poly_forced_40", "poly_8k"]


def auto_outputs(lib) -> dict:
    """{array name: array} of the fixture, computed with `lib` (an NmxLibrary on an emulator build)."""
    from py_neuromodulation_amd import NMSettings
    from tests import fir_sample_probe_cases as fir
    from tests import front_probe_cases as cases

    out: dict = {}
    names: dict = {}
    for name in CASES:
        sf_old, sf_new, Wr, env, _, _ = cases.RESAMPLE_CASES[name]
        p = cases.case_plan(name)
        eng = cases.resample_engine(lib, env, sf_old, sf_new, Wr, cases.RESAMPLE_C)
        try:
            rows = []
            for _cls, x in cases.resample_inputs(name, p):
                y = eng.preprocess_window(x.astype(np.float64))
                y32 = y.astype(np.float32)
                assert np.array_equal(y32.astype(np.float64), y), f"{name}: the library hands back widened float32"
                rows.append(y32)
            out[name] = np.stack(rows)
            names[name] = eng.kernels(1)
        finally:
            eng.close()
    eng = fir.build_engine(lib, {}, NMSettings.get_default(), ["c0", "c1", "c2"], 1000.0, features=["return_raw"], window=1000,
                           notch_taps=np.array([0.25, 0.5, 0.25]))
    try:
        eng.preprocess_window(np.random.default_rng(0).standard_normal((3, 1000)))
        names["no_resampler"] = eng.kernels(1)
    finally:
        eng.close()
    out["kernels_json"] = np.frombuffer(json.dumps(names, sort_keys=True).encode(), np.uint8)
    return out


def main() -> None:
    from py_neuromodulation_amd import _lib

    path = sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "tests" / "emu" / "libnmx_emu.so")
    dst = sys.argv[2] if len(sys.argv) > 2 else str(Path(__file__).with_name("resample_auto_parent.npz"))
    out = auto_outputs(_lib.NmxLibrary(path))
    np.savez_compressed(dst, **out)
    print(dst, {k: v.shape for k, v in out.items()}, Path(dst).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
