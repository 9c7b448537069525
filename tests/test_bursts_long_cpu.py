"""`bursts` on windows up to 40 000 samples in the single-thread emulator (tests/emu/nmx_emu.cpp): the partitioned band-pass
bank, nmx_hilbert_long_item (reached from nmx_hilbert_item, on slab 0), the threshold walk with bounded staging,
nmx_burst_stat_scan_item (reached from nmx_burst_stat_item) and the chunk cap, against the reference-generated fixture
(tests/golden/make_golden_bursts_long.py) and the float64 restatement.  Cases and policy: tests/bursts_long_cases.py.  The
seeds keep every `env >= thr` decision of the float64 oracle 1e-5 of the amplitude away from its threshold (asserted here,
from the oracle alone), so no `bursts` miss is accepted; the other families of defaults30k follow tests/parity.py.  At the
parent commit every positive case fails at plan construction (the variable is unknown there)."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import bursts_long_cases as cases  # noqa: E402


@pytest.fixture(autouse=True)
def _long_bursts(monkeypatch):
    """Bursts above 16 384 samples are opt-in (NMX_LONG_BURSTS): every plan of this file is built with it on."""
    monkeypatch.setenv("NMX_LONG_BURSTS", "1")


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


@pytest.mark.parametrize("tag", list(cases.CASES))
def test_seed_keeps_the_oracle_s_decisions_clear_of_the_threshold(tag):
    m = cases.oracle_margin(tag)
    print(f"{tag}: min |env - thr| / max |input row| = {m:.2e}")
    assert m >= cases.MARGIN, (tag, m)


@pytest.mark.parametrize("tag", list(cases.CASES))
def test_emulator_long_window_case(emu_lib, tag):
    acc = cases.run_case(emu_lib, tag)
    assert acc.get("bursts", 0) == 0, acc
    if tag != "defaults30k":
        assert acc == {}, acc


def test_list_entries_cross_what_the_cases_say():
    import py_neuromodulation_amd as nm

    k = {tag: cases.list_entries(p, cases.settings_of(nm, p).validate()) for tag, p in cases.CASES.items()}
    assert k["k9k"] == 3106 and k["w20k_f100"] == 5251 and k["w14k"] == 105001 and k["w40k"] == 300001, k
    assert k["odd16385"] > 65536 and k["defaults30k"] > 65536, k
    p = cases.CASES["k9k"]   # the ring fills within the hops
    assert p["window"] + (p["hops"] - 1) * (p["sfreq"] // 10) >= int(p["sfreq"] * p["time_duration_s"])


def test_fixture_taps_are_the_engine_s_design():
    """The band-pass FIRs the reference's Bursts object used (stored halves) against the engine's own design."""
    from py_neuromodulation_amd import fir_design

    for tag in cases.CASES:
        g, p, s, _, _, _ = cases.load_case(tag)
        want = cases.fixture_taps(g, tag)
        bands = list(s.bursts_settings.frequency_bands)
        assert len(bands) == len(want)
        for band, b in zip(bands, want):
            fr = s.frequency_ranges_hz[band]
            a = fir_design.band_pass_bank([(fr[0], fr[1])], float(p["sfreq"]))[0]
            np.testing.assert_allclose(np.asarray(a, np.float64), b, rtol=0, atol=1e-12)


def test_batching_gives_same_bytes(emu_lib):
    cases.batching_gives_same_bytes(emu_lib)


def test_state_travels(emu_lib):
    cases.state_travels(emu_lib)


def test_ragged_pair_of_long_lengths_hands_the_history_over(emu_lib):
    assert cases.ragged_pair(emu_lib) == [14000, 14001]


def test_chunk_cap(emu_lib, monkeypatch):
    cases.chunk_cap(emu_lib, monkeypatch.setenv, monkeypatch.delenv)


def test_window_above_the_limit_raises(emu_lib):
    cases.over_limit_raises(emu_lib)


def test_limited_features_raise_above_16384(emu_lib):
    cases.limited_features_raise(emu_lib)


def test_length_without_a_transform_split_raises(emu_lib):
    cases.no_split_raises(emu_lib)


def test_history_above_the_limit_fails_first(emu_lib):
    cases.history_limit_fails_first(emu_lib)


def test_gate_is_closed_without_the_opt_in(emu_lib, monkeypatch):
    cases.gate_is_closed_without_the_opt_in(emu_lib, monkeypatch.delenv)


def test_fill_is_scheduled_only_where_it_fits(emu_lib):
    cases.fill_only_where_it_fits(emu_lib)
