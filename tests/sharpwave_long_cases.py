"""Sharp waves on windows beyond 14 500 samples (up to the FIR limit): the cases of tests/golden/sharpwave_long.npz,
shared by the emulator tier (test_sharpwave_long_cpu.py) and the MI355X tier (test_sharpwave_long_gpu.py).  The
recordings come from tests/sharpwave_long_recording.py (the fixture stores seeds, not recordings).

Each case: Stream.run on 2 channels x 5 hops, sampling_rate_features_hz = 10, only sharpwave_analysis on, no
normaliser; the table is compared with the reference's (the fixture) AND with oracle.run_stream under
tests/parity.compare -- the 1e-5 policy, a miss accepted only on the per-entry decision-margin report of the float64
restatement.  The amplitude scale handed to that policy is the recording's own max |x| (amplitude-like features carry
an absolute fp32 error proportional to the input's scale; the existing long-window case passes 20 for a recording of
that size)."""

from __future__ import annotations

import json

import numpy as np

from tests import parity

from tests.sharpwave_long_recording import HOPS, recording  # noqa: F401


def load_case(tag):
    from tests.helpers import load_golden, settings_from_json

    g = load_golden("sharpwave_long")
    p = json.loads(str(g["params_json"]))[tag]
    s = settings_from_json(g[f"{tag}_settings_json"])
    ch = json.loads(str(g[f"{tag}_channels_json"]))
    return g, p, s, ch, [str(c) for c in g[f"{tag}_columns"]], g[f"{tag}_values"]


def fixture_taps(g, tag):
    """The reference's FIRs of a case, rebuilt from their stored first halves (centre included)."""
    out = []
    for name in g[f"{tag}_taps"]:
        h = np.asarray(g[str(name)], np.float64)
        out.append(np.concatenate([h, h[-2::-1]]))
    return out


def extrema_counts(s, ch, sfreq, pv, n_hops):
    """(maxima, minima) of every (hop, channel, filter) item's pre-filtered series, from the float64 restatement of the
    pre-filter on the pre-processed windows.  The kernels' rule is deterministic -- an item stays on the dense path iff
    it has at most 128 extrema of each kind -- so counts far from 128 say which path every item of a case takes."""
    from scipy.signal import find_peaks

    from oracle import nm_oracle as orc

    an = orc.SharpwaveAnalyzer(s, pv.names, sfreq)
    out = []
    for i in range(n_hops):
        y = an.filtered(pv.window(i))
        for c in range(y.shape[0]):
            for f in range(y.shape[1]):
                out.append((len(find_peaks(y[c, f])[0]), len(find_peaks(-y[c, f])[0])))
    return out


# which path the items of a case take: "dense" = every item has at most 100 extrema of a kind (none is flagged for the
# list code), "list" = every item has more than 1000 of each (all are flagged); all30k's settings rule the dense path out
PATHS = {"d30k": "dense", "d16k": "dense", "wide30k": "list", "all30k": None}


def run_case(lib, tag):
    """-> {family: misses accepted on a conditioning report} of this case (fixture and oracle comparisons together)."""
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd.stream import Stream

    g, p, s, ch, cols, want = load_case(tag)
    sfreq = float(p["sfreq"])
    x = recording(**p)
    W = int(sfreq * s.segment_length_features_ms / 1000)
    assert W > 14500
    kw = {} if lib is None else {"lib": lib}
    st = Stream(sfreq, channels=ch, settings=s, line_noise=50, **kw)
    df = st.run(x, save_csv=False)
    assert list(df.columns) == cols, tag
    got = df.to_numpy(float)
    assert got.shape == want.shape == (HOPS, len(cols)), tag
    np.testing.assert_array_equal(got[:, -1], want[:, -1])
    rows = orc.run_stream(x, sfreq, s, ch, line_noise=50)
    assert [list(r) for r in rows] == [cols] * HOPS
    orc_tab = np.array([[r[c] for c in cols] for r in rows])
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    pv = parity.PipelineVerifiers(s, ch, sfreq, x, starts, W, line_noise=50, ends=ends)
    counts = extrema_counts(s, ch, sfreq, pv, HOPS)
    print(f"{tag}: extrema per item: maxima {min(c[0] for c in counts)} - {max(c[0] for c in counts)}, "
          f"minima {min(c[1] for c in counts)} - {max(c[1] for c in counts)}")
    if PATHS[tag] == "dense":
        assert all(a <= 100 and b <= 100 for a, b in counts), counts
    elif PATHS[tag] == "list":
        assert all(a > 1000 and b > 1000 for a, b in counts), counts
    amp = float(np.abs(x).max())
    before = dict(parity.STATS["forgiven"])
    for name, ref in (("fixture", want), ("oracle", orc_tab)):
        for i in range(HOPS):
            n_bad, rep, worst = parity.compare(cols[:-1], got[i, :-1], ref[i, :-1], s, sfreq, amp, W, verifier=pv.row(i))
            print(f"{tag} vs {name} hop {i}: {n_bad} bad, worst relative error {worst}")
            assert n_bad == 0, f"{tag} vs {name} hop {i}\n{rep}"
    after = parity.STATS["forgiven"]
    acc = {f: after.get(f, 0) - before.get(f, 0) for f in after if after.get(f, 0) != before.get(f, 0)}
    print(f"{tag}: accepted misses {acc}")
    return acc


def over_limit_raises(lib):
    """One window above the limit (40 500 samples at 40.5 kHz): plan construction raises and names the limit."""
    import pytest

    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.stream import Stream

    s = NMSettings.get_default()
    s.reset()
    s.preprocessing = []
    s.postprocessing.feature_normalization = False
    s.features.sharpwave_analysis = True
    sfreq = 40500.0
    x = np.random.default_rng(1).standard_normal((2, 40500 + 4050)).astype(np.float32).astype(np.float64)
    kw = {} if lib is None else {"lib": lib}
    with pytest.raises(ValueError, match="40 000 samples"):
        Stream(sfreq, data=x, settings=s, line_noise=50, **kw).run(x, save_csv=False)


def notch_case(lib):
    """16 kHz, 16 000-sample windows behind the default notch filter (a 26 401-tap partitioned FIR stage in front of
    the sharp-wave pre-filters): Stream.run against oracle.run_stream under the same policy (no reference fixture)."""
    from oracle import nm_oracle as orc
    from py_neuromodulation_amd.stream import Stream

    _, p, s, ch, cols, _ = load_case("d16k")
    s.preprocessing = ["notch_filter"]
    sfreq, W = float(p["sfreq"]), int(p["sfreq"])
    x = recording(**p)
    t = np.arange(x.shape[1]) / sfreq
    x = (x + 4 * np.sin(2 * np.pi * 50 * t)).astype(np.float32).astype(np.float64)
    kw = {} if lib is None else {"lib": lib}
    df = Stream(sfreq, channels=ch, settings=s, line_noise=50, **kw).run(x, save_csv=False)
    assert list(df.columns) == cols
    got = df.to_numpy(float)
    rows = orc.run_stream(x, sfreq, s, ch, line_noise=50)
    tab = np.array([[r[c] for c in cols] for r in rows])
    starts, ends, _ = orc.window_schedule(x.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    pv = parity.PipelineVerifiers(s, ch, sfreq, x, starts, W, line_noise=50, ends=ends)
    before = sum(parity.STATS["forgiven"].values())
    for i in range(HOPS):
        n_bad, rep, worst = parity.compare(cols[:-1], got[i, :-1], tab[i, :-1], s, sfreq, float(np.abs(x).max()), W,
                                           verifier=pv.row(i))
        print(f"notch16k vs oracle hop {i}: {n_bad} bad, worst relative error {worst}")
        assert n_bad == 0, f"notch16k hop {i}\n{rep}"
    return sum(parity.STATS["forgiven"].values()) - before
