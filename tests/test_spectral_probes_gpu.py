"""Per-bin probes of the spectral kernels on the MI355X (libnmx.so): the persistent long-window kernel at one length per
class of the plan's split (slab and LDS forms), the wave-level kernels of the default shapes -- which the emulator never
runs -- bin by bin at their own switches, and the generic LDS transform through return_spectrum.  Cases and policy:
tests/spectral_probe_cases.py.  The module as a whole may accept no miss in the time-domain families and at most 2 in
fft + welch + stft, each on a conditioning report (the device's fast log10 / sqrt), the allowance of
test_timeosc_long_gpu.py; the figures observed are in profiles/spectral_probes.md."""

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import spectral_probe_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

_ACCEPTED = {"spectral": 0}


def _book(result):
    acc = result[0]
    assert set(acc) <= {"fft", "welch", "stft"}, acc
    _ACCEPTED["spectral"] += sum(acc.values())
    assert _ACCEPTED["spectral"] <= 2, f"spectral misses accepted by the probes so far: {_ACCEPTED}"


# ---- long-window kernel ---------------------------------------------------------------------------------------------
def test_every_97th_length_builds_or_names_itself():
    cases.sweep_construction(None)


@pytest.mark.parametrize("N", list(cases.LONG_LENGTHS))
def test_long_window_spread(N):
    _book(cases.long_spread(None, N))


@pytest.mark.parametrize("N,which", cases.CLUSTERS)
def test_long_window_cluster(N, which):
    _book(cases.long_cluster(None, N, which))


@pytest.mark.parametrize("N", cases.WIDE_LENGTHS)
def test_long_window_wide_band_beside_one_bin(N):
    _book(cases.long_wide(None, N))


def test_long_window_two_seconds():
    _book(cases.long_two_seconds(None))


# ---- wave-level kernels of the default shapes -------------------------------------------------------------------------
def test_w1000_low_band_form():
    _book(cases.w1000_low())


def test_w1000_full_form():
    _book(cases.w1000())


def test_w1000_with_stft():
    _book(cases.w1000_with_stft())


@pytest.mark.parametrize("window_ms", [600, 1500])
def test_stft500(window_ms):
    _book(cases.stft500(window_ms))


@pytest.mark.parametrize("part", [0, 1])
def test_w510_fft_at_30_khz(part):
    _book(cases.w510_fft_30k(part))


@pytest.mark.parametrize("part", [0, 1])
def test_w510_fft_and_stft(part):
    _book(cases.w510_fft_stft(part))


@pytest.mark.parametrize("start", cases.SPECMM_SPANS)
def test_matrix_pipe_single_bins(start):
    _book(cases.specmm(start))


def test_nine_bands_leave_the_wave_kernel():
    """The bins of test_w1000_full_form and one more band: past the wave kernels' eight."""
    _book(cases.w1000(extra_bins=[300], kernel=cases.GENERIC, tag="w1000 bins, 9 bands"))


def test_median_leaves_the_wave_kernel():
    _book(cases.w1000(estimators=("mean", "median"), kernel=cases.GENERIC, tag="w1000 bins, median"))


# ---- generic LDS transform ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", cases.SPECTRUM_LENGTHS)
def test_generic_transform_every_bin(N):
    _book(cases.full_spectrum(None, N, kernel=cases.GENERIC))


@pytest.mark.parametrize("which", list(cases.SPREAD_13000))
def test_generic_transform_13000_probes(which):
    _book(cases.generic_13000(None, which, kernel=cases.GENERIC))
