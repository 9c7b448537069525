"""Per-window probes of the time-domain statistics on the MI355X (libnmx.so): the packed register form at every length
where a 256-sample group fills or empties, the scalar DPP form, the three load variants of the W = 1000 kernels, the
persistent kernel's item loop iterating, the matrix-pipe kernel's single pass with its cancellation flag and redo -- none of
which the emulator runs --, each kernel asserted by name, every (window, channel) against the float64 restatement of the
reference on the float32 samples the kernel read.  Cases and policy: tests/timedomain_probe_cases.py; no miss is accepted,
no case is skipped; the figures observed are in profiles/timedomain_probes.md."""

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import timedomain_probe_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
SEEN: dict = {}


@pytest.fixture(scope="module", autouse=True)
def gpu_lib():
    from py_neuromodulation_amd import _lib

    lib = _lib.get_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    assert "libnmx.so" in str(lib.path)
    return lib


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case(name):
    """run_case asserts kernels(2) against the kernel the restated plan chooses, and for class d that the persistent
    kernel's first launch needs the passes the case is about, computed from this device's CU count."""
    rep = cases.run_case(None, name)
    c = cases.CASES[name]
    assert rep.n == c["C"] * c["hops"]
    if c["cls"] == "d":
        assert rep.launches[0][2] >= c["min_passes"]
    SEEN[name] = cases.kernel_name(c)


def test_every_kernel_of_the_table_was_seen():
    """The names asserted by the cases that ran (this module, run as a whole) are the table's, no more and no less."""
    assert set(SEEN) == set(cases.CASES), sorted(set(cases.CASES) - set(SEEN))
    assert set(SEEN.values()) == cases.KERNELS
