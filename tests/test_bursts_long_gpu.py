"""`bursts` on windows up to 40 000 samples on the MI355X (libnmx.so): nmx_kern_hilbert_long behind the partitioned band-pass
bank, the workgroup walks with bounded staging, nmx_kern_burst_stat_scan, against the reference-generated fixture
(tests/golden/make_golden_bursts_long.py) and the float64 restatement.  Cases and policy: tests/bursts_long_cases.py.  The
seeds keep every decision of the float64 oracle 1e-5 of the amplitude away from its threshold (test_bursts_long_cpu.py
asserts it), so no `bursts` miss is accepted; the other families of defaults30k follow tests/parity.py (counts observed:
profiles/bursts_long.md).  At the parent commit every positive case raises ValueError at plan construction (the variable is unknown there)."""

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

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", list(cases.CASES))
def test_long_window_case(tag):
    acc = cases.run_case(None, tag)
    assert acc.get("bursts", 0) == 0, acc
    if tag != "defaults30k":
        assert acc == {}, acc


def test_batching_gives_same_bytes():
    cases.batching_gives_same_bytes(None)


def test_state_travels():
    cases.state_travels(None)


def test_ragged_pair_of_long_lengths_hands_the_history_over():
    assert cases.ragged_pair(None) == [14000, 14001]


@pytest.mark.parametrize("tag", ["w14k", "odd16385", "w40k"])
def test_kernels_of_the_long_chain(tag):
    """From 13 651 samples on the new Hilbert kernel; beyond 16 384 the scan statistics.  A fresh five-hop batch that fits
    the sort-once fill (32 768 samples) is the fill's; w40k's first hop alone is longer: the tiled workgroup walk, staged."""
    (k,) = cases.kernels_of(None, tag)
    assert "nmx_kern_hilbert_long" in k and "nmx_kern_hilbert_fixed" not in k, k
    assert ("nmx_kern_burst_stat_scan" in k) == (tag != "w14k"), k
    if tag == "w40k":
        assert "nmx_kern_burst_thr_tiled" in k and "nmx_kern_burst_fill" not in k, k
    else:
        assert "nmx_kern_burst_fill" in k and "nmx_kern_burst_thr" not in k, k


@pytest.mark.parametrize("tag", ["k9k", "w14k"])
def test_staged_walk_gives_the_fill_s_bytes(tag):
    """A first batch of ONE hop is not the fill's: the workgroup walk absorbs the 9 000 / 14 000 samples in tiles of 4 096 --
    the register merge (K = 3 106) and the tiled merge (K = 105 001) -- and the four hops behind it one by one.  Same rows as
    the one-batch run, whose walk is the sort-once fill."""
    p = cases.CASES[tag]
    x32 = cases.recording(p).astype(np.float32)
    hop = p["sfreq"] // 10
    out = []
    for calls in ((5,), (1, 4)):
        eng = cases.engine_of(None, tag)
        try:
            out.append(cases.feed(eng, x32, 0, calls, p["window"], hop))
        finally:
            eng.close()
    (rows, kernels), (rows1, kernels1) = out
    assert "nmx_kern_burst_fill" in kernels[0], kernels
    for k in kernels1:
        assert "nmx_kern_burst_fill" not in k, kernels1
        assert ("nmx_kern_burst_thr_tiled" in k) if tag == "w14k" else ("nmx_kern_burst_thr<" in k or "nmx_kern_burst_thr_wide" in k), kernels1
    assert ("nmx_kern_hilbert_long" in kernels1[0]) == (tag == "w14k"), kernels1
    assert np.isfinite(rows).all() and rows.tobytes() == rows1.tobytes(), np.flatnonzero((rows != rows1).any(axis=1))


def test_kernels_w20k_f100():
    """The last of three batches starts on a full ring: a one-wave walk (200 samples per hop: four registers per lane)."""
    _, kernels = cases.f100_rows(None, cases.F100_THREE)
    assert "nmx_kern_burst_thr_wave<4, false>" in kernels[-1], kernels
    assert "nmx_kern_burst_thr<" not in kernels[-1] and "tiled" not in kernels[-1], kernels
    assert "nmx_kern_hilbert_long" in kernels[0] and "nmx_kern_burst_stat_scan" in kernels[0], kernels


@pytest.mark.parametrize("sfreq", [1000, 8000])
def test_short_plans_keep_their_kernels_and_bytes(sfreq):
    """Plans that build at the parent commit name exactly the kernels they named there and return the same bytes
    (tests/golden/bursts_8k_parent.npz: recorded on the MI355X with the parent's library, 2 ch x 5 hops)."""
    from tests.helpers import load_golden

    g = load_golden("bursts_8k_parent")
    rows, kernels = cases.plain_rows(None, sfreq)
    assert kernels == str(g[f"kernels_{sfreq}"]), kernels
    want = g[f"rows_{sfreq}"]
    assert rows.dtype == want.dtype and rows.shape == want.shape
    assert rows.tobytes() == want.tobytes(), f"rows that differ: {np.flatnonzero((rows != want).any(axis=1))}"


def test_window_above_the_limit_raises():
    cases.over_limit_raises(None)


def test_limited_features_raise_above_16384():
    cases.limited_features_raise(None)


def test_length_without_a_transform_split_raises():
    cases.no_split_raises(None)


def test_history_above_the_limit_fails_first():
    cases.history_limit_fails_first(None)


def test_gate_is_closed_without_the_opt_in(monkeypatch):
    cases.gate_is_closed_without_the_opt_in(None, monkeypatch.delenv)
