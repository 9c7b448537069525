"""Probes of the bursts chain on the MI355X (libnmx.so): every Hilbert kernel (w500 / w1000 and their sparse forms, fixed128,
long), every threshold walk (the fill launches, the workgroup kernels thr<..>, thr_wide, thr_tiled, the one-wave walks
<2, true>, <2, false>, <4, false>, the list in LDS or L2) and every run-statistics kernel (LDS, registers <16> / <32> and their
sparse forms, the tiled scan) -- most of which the emulator does not run --, each asserted by name, the top-K list of the
state blob rank by rank and every output of every row against the float64 restatement.  Cases and policy:
tests/burst_probe_cases.py; no miss is accepted, no case is skipped; the figures observed are in profiles/burst_probes.md."""

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import burst_probe_cases as cases  # noqa: E402

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
    """run_case asserts kernels(4) against the case's table, the list after every batch and every row."""
    rep = cases.run_case(None, name)
    c = cases.CASES[name]
    assert rep.rows == c["C"] * 2 * cases.n_hops(c)
    if c["kind"] != "noise":
        assert rep.left == 0


def test_sparse_and_dense_rows_are_the_same_bytes():
    """Stream (b) with the sparse envelope storage on and off: both equal the reference (test_case); here their tables are
    compared byte for byte, batch by batch -- a row the sparse kernels answer with six zeros is a row without a sample at
    or above its threshold."""
    import numpy as np

    for a, b in (("quiet2", "quiet2_dense"), ("quiet5", "quiet5_dense")):
        ta, tb = cases.run_table(None, a), cases.run_table(None, b)
        assert ta.shape == tb.shape and ta.tobytes() == tb.tobytes(), f"{a} against {b}: {int((ta != tb).sum())} entries differ"
        assert np.any(ta[-5:] == 0)
