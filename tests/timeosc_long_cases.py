"""Time-domain, FFT and Welch features on windows beyond the generic kernel's LDS layout (FFT / Welch segments above
~13 650 samples, windows up to 40 000): the cases of tests/golden/timeosc_long.npz, shared by the emulator tier
(test_timeosc_long_cpu.py) and the MI355X tier (test_timeosc_long_gpu.py).  The recordings come from
tests/timeosc_long_recording.py (the fixture stores generator parameters, not recordings).

Each case: Stream.run on 2 channels x 5 hops, sampling_rate_features_hz = 10, no normaliser; the table is compared with
the reference's (the fixture) AND with oracle.run_stream under tests/parity.compare -- the 1e-5 policy, a miss accepted
only on the conditioning report of the float64 restatement (a PipelineVerifiers row), as
sharpwave_long_cases.run_case does.  Accepted misses are returned per family; the tiers cap them."""

from __future__ import annotations

import json

import numpy as np

from tests import parity
from tests.timeosc_long_recording import HOPS, case_recording  # noqa: F401
from tests.sharpwave_long_recording import recording  # noqa: F401

FIXTURE_TAGS = ["d30k", "e40k", "t24414", "seg20k", "wide20k"]


def load_case(tag):
    from tests.helpers import load_golden, settings_from_json

    g = load_golden("timeosc_long")
    p = json.loads(str(g["params_json"]))[tag]
    s = settings_from_json(g[f"{tag}_settings_json"])
    ch = json.loads(str(g[f"{tag}_channels_json"]))
    return p, s, ch, [str(c) for c in g[f"{tag}_columns"]], g[f"{tag}_values"]


def _kw(lib):
    return {} if lib is None else {"lib": lib}


def _accepted_since(before):
    after = parity.STATS["forgiven"]
    return {f: after.get(f, 0) - before.get(f, 0) for f in after if after.get(f, 0) != before.get(f, 0)}


def _against(tag, name, cols, got, ref, s, sfreq, x, W, pv, rows=None):
    amp = float(np.nanmax(np.abs(x)))
    for i in range(HOPS) if rows is None else rows:
        n_bad, rep, worst = parity.compare(cols[:-1], got[i, :-1], ref[i, :-1], s, sfreq, amp, W, verifier=pv.row(i))
        print(f"{tag} vs {name} hop {i}: {n_bad} bad, worst relative error {worst}")
        assert n_bad == 0, f"{tag} vs {name} hop {i}\n{rep}"


def _oracle_table(x, sfreq, s, ch, cols):
    from oracle import nm_oracle as orc

    rows = orc.run_stream(x, sfreq, s, ch, line_noise=50)
    assert [list(r) for r in rows] == [cols] * HOPS
    tab = np.array([[r[c] for c in cols] for r in rows])
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    return tab, starts, ends


def run_case(lib, tag, want_rows=False):
    """-> {family: misses accepted on a conditioning report} of this case (fixture and oracle comparisons together)."""
    from py_neuromodulation_amd.stream import Stream

    p, s, ch, cols, want = load_case(tag)
    sfreq = float(p["sfreq"])
    x = case_recording(p)
    W = int(sfreq * s.segment_length_features_ms / 1000)
    assert W == p["window"] > 13654
    df = Stream(sfreq, channels=ch, settings=s, line_noise=50, **_kw(lib)).run(x, save_csv=False)
    assert list(df.columns) == cols, tag
    got = df.to_numpy(float)
    assert got.shape == want.shape == (HOPS, len(cols)), tag
    np.testing.assert_array_equal(got[:, -1], want[:, -1])
    tab, starts, ends = _oracle_table(x, sfreq, s, ch, cols)
    pv = parity.PipelineVerifiers(s, ch, sfreq, x, starts, W, line_noise=50, ends=ends)
    before = dict(parity.STATS["forgiven"])
    _against(tag, "fixture", cols, got, want, s, sfreq, x, W, pv)
    _against(tag, "oracle", cols, got, tab, s, sfreq, x, W, pv)
    acc = _accepted_since(before)
    print(f"{tag}: accepted misses {acc}")
    return (acc, got) if want_rows else acc


def _oracle_only(lib, tag, s, ch, cols, sfreq, x, W, rows=None):
    from py_neuromodulation_amd.stream import Stream

    df = Stream(sfreq, channels=ch, settings=s, line_noise=50, **_kw(lib)).run(x, save_csv=False)
    if cols is None:
        cols = list(df.columns)
    assert list(df.columns) == cols, tag
    got = df.to_numpy(float)
    tab, starts, ends = _oracle_table(x, sfreq, s, ch, cols)
    pv = parity.PipelineVerifiers(s, ch, sfreq, x, starts, W, line_noise=50, ends=ends)
    before = dict(parity.STATS["forgiven"])
    _against(tag, "oracle", cols, got, tab, s, sfreq, x, W, pv, rows)
    acc = _accepted_since(before)
    print(f"{tag}: accepted misses {acc}")
    return acc, got, tab


def n16k_case(lib):
    """16 kHz, 16 000-sample windows (the 13 654 - 16 384 band: one 8000-point transform, no split) behind the default
    notch filter, a 50 Hz tone added, offsets +1000 / -1000 carried through the FIR stage: Stream.run against
    oracle.run_stream (no reference table, as sharpwave_long_cases.notch_case)."""
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd import channels as chmod

    s = NMSettings.get_default()
    s.reset()
    s.preprocessing = ["notch_filter"]
    s.postprocessing.feature_normalization = False
    for f in ("raw_hjorth", "return_raw", "linelength", "fft", "welch"):
        setattr(s.features, f, True)
    sfreq, W = 16000.0, 16000
    x = recording(1611, W, "walk")
    t = np.arange(x.shape[1]) / sfreq
    x = (x + 4 * np.sin(2 * np.pi * 50 * t) + np.array([[1000.0], [-1000.0]])).astype(np.float32).astype(np.float64)
    return _oracle_only(lib, "n16k", s, chmod.get_default_channels_from_data(x), None, sfreq, x, W)[0]


def nan30k_case(lib):
    """d30k with NaN samples in channel 0 of hops 1 - 2: the NaN-channel policy blanks that channel's columns in those
    rows, the other channel's values are the ones of the clean run; oracle only."""
    p, s, ch, cols, _ = load_case("d30k")
    sfreq, W = float(p["sfreq"]), p["window"]
    x = case_recording(p)
    hop = W // 10
    xn = x.copy()
    xn[0, W + hop + 100:W + hop + 140] = np.nan   # new samples of hop 2 (windows 2, 3, ... hold them); hop 1 below
    xn[0, W + 50:W + 60] = np.nan
    acc, got, tab = _oracle_only(lib, "nan30k", s, ch, cols, sfreq, xn, W)
    assert np.array_equal(np.isnan(got), np.isnan(tab)), "NaN pattern differs from the oracle's"
    assert np.isnan(got).any() and not np.isnan(got[0]).any()
    return acc


def process_equals_run(lib, run_rows):
    """DataProcessor.process window by window gives the Stream.run rows of d30k (1e-6 relative: the tolerance between
    call shapes used throughout tests/parity_cases.py)."""
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd.data_processor import DataProcessor

    p, s, ch, cols, _ = load_case("d30k")
    sfreq = float(p["sfreq"])
    x = case_recording(p)
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    dp = DataProcessor(sfreq=sfreq, settings=s, channels=ch, line_noise=50, **_kw(lib))
    feat = [c for c in cols if c != "time"]
    for i, (a, b) in enumerate(zip(starts, ends)):
        row = dp.process(x[:, a:b])
        assert list(row) == feat
        np.testing.assert_allclose(np.array(list(row.values()), float), run_rows[i, :len(feat)], rtol=1e-6, atol=0,
                                   err_msg=f"hop {i}")


# ---- a plan the generic kernel keeps ------------------------------------------------------------------------------
def settings_13k():
    """13 000-sample windows at 13 kHz: fft + welch with the four estimators and the time-domain features -- the generic
    kernel's layout still fits LDS (tests/golden/timeosc_13k_parent.npz: the emulator's rows at the parent commit)."""
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    for f in ("raw_hjorth", "return_raw", "linelength", "fft", "welch"):
        setattr(s.features, f, True)
    for o in (s.fft_settings, s.welch_settings):
        o.features.mean = o.features.median = o.features.std = o.features.max = True
    return s


def rows_13k(lib):
    from py_neuromodulation_amd.stream import Stream

    x = recording(4, 13000, "walk", hops=2)
    return Stream(13000.0, data=x, settings=settings_13k(), line_noise=50, **_kw(lib)).run(x, save_csv=False)


# ---- errors, all at plan construction -----------------------------------------------------------------------------
def _run(lib, sfreq, s, n=None):
    from py_neuromodulation_amd.stream import Stream

    n = int(sfreq) if n is None else n
    x = np.random.default_rng(1).standard_normal((2, n + n // 10)).astype(np.float32).astype(np.float64)
    Stream(float(sfreq), data=x, settings=s, line_noise=50, **_kw(lib)).run(x, save_csv=False)


def _plain(*features):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    for f in features:
        setattr(s.features, f, True)
    return s


def over_limit_raises(lib):
    import pytest

    with pytest.raises(ValueError, match="40 000 samples"):
        _run(lib, 40500, _plain("fft", "raw_hjorth"))


def short_only_features_raise(lib):
    """Above 16 384 samples every feature and pre-processor outside the long-window set is refused: the message names the
    limit and the features that do run up to 40 000."""
    import pytest

    def expect(s):
        with pytest.raises(ValueError) as e:
            _run(lib, 20000, s)
        msg = str(e.value)
        assert "16 384" in msg and "40 000" in msg, msg
        for f in ("raw_hjorth", "return_raw", "linelength", "fft", "welch", "sharpwave_analysis"):
            assert f in msg, msg

    for f in ("stft", "bandpass_filter", "bursts"):
        expect(_plain("fft", f))
    s = _plain("fft", "coherence")
    s.coherence_settings.channels = [["ch0", "ch1"]]
    s.frequency_ranges_hz["wide"] = [100, 400]   # (a band that holds a bin of the 65-bin grid at 20 kHz)
    s.coherence_settings.frequency_bands = ["wide"]
    expect(s)
    s = _plain("fft")
    s.preprocessing = ["raw_normalization"]
    expect(s)
    s = _plain("fft")
    s.preprocessing = ["raw_resampling"]
    s.raw_resampling_settings.resample_freq_hz = 19000
    expect(s)


def return_spectrum_raises(lib):
    import pytest

    for sfreq in (20000, 16000):   # above 16 384 samples, and in the band the generic layout does not fit
        s = _plain("fft")
        s.fft_settings.return_spectrum = True
        with pytest.raises(NotImplementedError, match="return_spectrum"):
            _run(lib, sfreq, s)


def refused_length_raises(lib):
    """39 989 is prime: no split into subsequences the LDS transforms take."""
    import pytest

    with pytest.raises(ValueError, match="39 989"):
        _run(lib, 39989, _plain("fft"))
