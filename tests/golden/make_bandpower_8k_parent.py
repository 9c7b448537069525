"""Record tests/golden/bandpower_8k_parent.npz: the rows of the 8 kHz / 8000-sample band-pass plan of
tests/bandpower_long_cases.rows_8k (the partitioned bank, activity + mobility + complexity, 2 ch x 3 hops) as the single-thread
emulator of ANOTHER build computes them: the last commit in which nmx_plan_create does not read NMX_LONG_BANDPOWER (the parent
of the commit that added this file).

The fixture CANNOT be regenerated from this tree alone.  The recipe: check that commit out into a second directory, build its
emulator there (`__graft_entry__.build_emu()` in that checkout returns the library's path), and hand the library to this script,
run from THIS tree:

    python tests/golden/make_bandpower_8k_parent.py <libnmx_emu.so of that build> [output.npz]

The emulator library is the one given; the package, the case and the recording are this tree's.  Run on this tree's own
emulator instead, the script must give the committed rows byte for byte -- which is what
test_bandpower_long_cpu.py::test_nothing_below_the_gate_moved asserts."""

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from py_neuromodulation_amd import _lib  # noqa: E402
from tests import bandpower_long_cases as cases  # noqa: E402

out = Path(sys.argv[2]) if len(sys.argv) > 2 else HERE / "bandpower_8k_parent.npz"
rows, _ = cases.rows_8k(_lib.NmxLibrary(Path(sys.argv[1]).resolve()))
assert np.isfinite(rows).all()
np.savez_compressed(out, rows=rows)
print("wrote", out, rows.shape, out.stat().st_size, "bytes")
