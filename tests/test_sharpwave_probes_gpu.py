"""Per-trough probes of the sharp-wave detector on the MI355X (libnmx.so): the device extrema forms (branch-free chunks of
16 and 8, the 64-bit mask form, the two-pass form), the register-resident selection, pairing and estimators at their 64 /
65 and 128 / 129 boundaries, the dense-first launch with its `todo` redo, the list kernel's blocked lf[] rewrite and the
slab layout -- none of which the emulator runs --, each kernel asserted by name, every output of every item against the
float64 restatement run on the series the kernel itself read.  Cases and policy: tests/sharpwave_probe_cases.py; no miss
is accepted, no case is skipped; the figures observed are in profiles/sharpwave_probes.md."""

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import sharpwave_probe_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu_lib():
    from py_neuromodulation_amd import _lib

    lib = _lib.get_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    assert "libnmx.so" in str(lib.path)
    return lib


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case(name):
    """run_case asserts kernels(5) against the kind the restated plan chooses (KERNELS)."""
    rep = cases.run_case(None, name)
    c = cases.CASES[name]
    assert rep.n == c["C"] * c["hops"] * len(c["taps"])


def test_every_kind_and_kernel_is_asserted_by_a_case():
    kinds = {cases.case_choice(n)["kind"] for n in cases.CASES}
    assert kinds == set(cases.KERNELS)
    assert set().union(*(cases.KERNELS[k] for k in kinds)) == {"nmx_kern_sharp", "nmx_kern_sharp_dense", "nmx_kern_sharp_todo",
                                                               "nmx_kern_sharp_slab"}


def test_noise_layer():
    """Default filters and settings, 64 channels x 2 seeds: at most 5 % of the (channel, filter) rows left out on a
    near-tie of their own read-out (printed), nothing else excused."""
    share = cases.run_noise(None)
    assert share <= cases.NOISE_LEFT_OUT
