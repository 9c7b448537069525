"""Per-bin probes of the spectral kernels in the single-thread emulator (tests/emu/nmx_emu.cpp): the long-window item
(nmx_k_timeosc_long.h) at one length per class of the plan's split, and the generic LDS transform bin by bin.  Cases and
policy: tests/spectral_probe_cases.py.  The emulator tier accepts no miss in any family; the figures observed are in
profiles/spectral_probes.md."""

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import spectral_probe_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


def test_long_split_restatement_names_the_classes():
    """The table of lengths against the restated split and layout arithmetic; the restatement against the lengths the
    plan is known to accept (the fixture lengths) and to refuse (39 989, prime)."""
    for N in cases.LONG_LENGTHS:
        cases.check_class(N)
    assert [cases.long_split(n) for n in (16000, 20000, 24414, 30000, 40000, 39989)] == [1, 2, 3, 2, 4, 0]
    lengths = range(13655, 40001)
    D = [cases.long_split(n) for n in lengths]
    ok = [(n, d) for n, d in zip(lengths, D) if d]
    assert len(lengths) == 26346 and len(ok) == 18403 and max(D) == 61
    assert sum(1 for n, d in ok if (n // d) & 1) == 7991


def test_every_97th_length_builds_or_names_itself(emu_lib):
    built, refused = cases.sweep_construction(emu_lib)
    print(f"built {built}, refused {refused}")


@pytest.mark.parametrize("N", list(cases.LONG_LENGTHS))
def test_long_window_spread(emu_lib, N):
    acc, _ = cases.long_spread(emu_lib, N)
    assert acc == {}, acc


@pytest.mark.parametrize("N,which", cases.CLUSTERS)
def test_long_window_cluster(emu_lib, N, which):
    acc, _ = cases.long_cluster(emu_lib, N, which)
    assert acc == {}, acc


@pytest.mark.parametrize("N", cases.WIDE_LENGTHS)
def test_long_window_wide_band_beside_one_bin(emu_lib, N):
    acc, _ = cases.long_wide(emu_lib, N)
    assert acc == {}, acc


def test_long_window_two_seconds(emu_lib):
    acc, _ = cases.long_two_seconds(emu_lib)
    assert acc == {}, acc


@pytest.mark.parametrize("N", cases.SPECTRUM_LENGTHS)
def test_generic_transform_every_bin(emu_lib, N):
    acc, _ = cases.full_spectrum(emu_lib, N)
    assert acc == {}, acc


@pytest.mark.parametrize("which", list(cases.SPREAD_13000))
def test_generic_transform_13000_probes(emu_lib, which):
    """The largest generic layout keeps the generic item with single-bin bands at both ends of the grid."""
    acc, _ = cases.generic_13000(emu_lib, which)
    assert acc == {}, acc
