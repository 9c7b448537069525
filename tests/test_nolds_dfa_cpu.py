"""nolds detrended fluctuation analysis (features/nolds.py; nolds.dfa with its final fit "poly") without a GPU: the opt-in
(keyword and NMX_NOLDS_FIT), key layout, scale table and construction errors on dry_run plans; the float64 restatement
(tests/nolds_dfa_oracle.py) against the reference-generated fixture; and the kernel's item code in the single-thread
emulator (tests/emu/nmx_emu.cpp) on the cases of tests/nolds_dfa_cases.py -- the same cases tests/test_nolds_dfa_gpu.py
runs on the device."""

import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import nolds_dfa_cases as cases  # noqa: E402
from tests import nolds_dfa_oracle as oracle  # noqa: E402
from tests.helpers import load_golden, settings_from_json  # noqa: E402

DFA = cases.DFA


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


@pytest.fixture(autouse=True)
def no_variable(monkeypatch):
    monkeypatch.delenv("NMX_NOLDS_FIT", raising=False)


# ---- surface: the opt-in, keys, scale table (no device) --------------------------------------------------------------------
def test_poly_builds_a_plan_with_dfa():
    from py_neuromodulation_amd import _lib

    eng = cases.engine(None, names=["a", "b"], bands=["low_beta"], dry_run=True)
    d = eng.desc
    assert d.nolds_measures == 16 and d.nolds_dfa_fit == 1 and d.abi_version == _lib.NMX_ABI_VERSION
    assert [d.nolds_dfa_scales[k] for k in range(d.nolds_dfa_n_scales)] == oracle.scales(1000)
    assert eng.keys == [f"{ch}_nolds_{DFA}_{s}" for s in ("raw", "low_beta") for ch in ("a", "b")]
    assert (d.nolds_dfa_cols.base, d.nolds_dfa_cols.ch_stride, d.nolds_dfa_cols.a_stride) == (0, 1, 2)
    assert d.nolds_n_taps[0] == 999 and d.n_filters == 0   # (the band filters run exactly as for a sample-entropy plan)


@pytest.mark.parametrize("fit", [None, "RANSAC"])
def test_without_the_opt_in_dfa_raises_as_before(fit):
    with pytest.raises(NotImplementedError, match=DFA) as e:
        cases.engine(None, nolds_fit=fit, dry_run=True)
    assert "RANSAC" in str(e.value) and "only sample_entropy runs on the device" in str(e.value)


@pytest.mark.parametrize("fit", ["Poly", "ransac", "", 1, True, "lstsq"])
def test_a_bad_value_is_a_value_error(fit):
    with pytest.raises(ValueError, match="nolds_fit"):
        cases.engine(None, nolds_fit=fit, dry_run=True)


def test_the_variable_alone_enables_it(monkeypatch):
    monkeypatch.setenv("NMX_NOLDS_FIT", "poly")
    assert cases.engine(None, nolds_fit=None, dry_run=True).desc.nolds_dfa_fit == 1
    assert cases.engine(None, nolds_fit="poly", dry_run=True).desc.nolds_dfa_fit == 1
    with pytest.raises(NotImplementedError, match="RANSAC"):   # (the keyword wins)
        cases.engine(None, nolds_fit="RANSAC", dry_run=True)
    monkeypatch.setenv("NMX_NOLDS_FIT", "RANSAC")
    with pytest.raises(NotImplementedError, match=DFA):
        cases.engine(None, nolds_fit=None, dry_run=True)
    monkeypatch.setenv("NMX_NOLDS_FIT", "huber")
    with pytest.raises(ValueError, match="NMX_NOLDS_FIT"):
        cases.engine(None, nolds_fit=None, dry_run=True)


def test_the_variable_reaches_every_class(monkeypatch):
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.features import Nolds
    from py_neuromodulation_amd.sharding import MultiDeviceProcessor, ShardedStream

    g = load_golden("nolds_dfa")
    s = settings_from_json(g["b_settings_json"])
    ch = json.loads(str(g["b_channels_json"]))
    want = [str(c) for c in g["b_columns"] if str(c) != "time"]
    with pytest.raises(NotImplementedError, match=DFA):
        DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True)
    assert DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True, nolds_fit="poly").keys == want
    with pytest.raises(NotImplementedError, match=DFA):
        Nolds(s, [], 1000.0)
    assert Nolds(s, [], 1000.0, nolds_fit="poly").keys == []
    sh = ShardedStream(1000.0, ch, s, rank=0, world_size=1, local_input=True, nolds_fit="poly")
    assert sh._dp.keys == want
    monkeypatch.setenv("NMX_NOLDS_FIT", "poly")
    assert DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True).keys == want
    assert Nolds(s, [], 1000.0).keys == []
    assert callable(MultiDeviceProcessor)


@pytest.mark.parametrize("measure", ["correlation_dimension", "lyapunov_exponent", "hurst_exponent"])
def test_the_other_three_measures_keep_raising(measure):
    from py_neuromodulation_amd.engine import HotPathEngine

    s = cases.dfa_settings()
    s.nolds_settings.features = {DFA: True, measure: True}
    with pytest.raises(NotImplementedError, match=measure) as e:
        HotPathEngine(s, ["a"], 1000.0, dry_run=True, nolds_fit="poly")
    assert "RANSAC" in str(e.value) and DFA not in str(e.value)


@pytest.mark.parametrize("tag", ["a", "b", "c", "e"])
def test_pipeline_keys_in_reference_order(tag):
    """DFA alone (a, c), sample entropy and DFA together (b), raw off (e)"""
    from py_neuromodulation_amd.data_processor import DataProcessor

    g = load_golden("nolds_dfa")
    s = settings_from_json(g[f"{tag}_settings_json"])
    ch = json.loads(str(g[f"{tag}_channels_json"]))
    dp = DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True, nolds_fit="poly")
    assert dp.keys == [str(c) for c in g[f"{tag}_columns"] if str(c) != "time"]


@pytest.mark.parametrize("n", cases.TABLE_LENGTHS)
def test_scale_table_is_the_oracle_s(n):
    d = cases.engine(None, W=n, dry_run=True).desc
    got = [d.nolds_dfa_scales[k] for k in range(d.nolds_dfa_n_scales)]
    assert got == oracle.scales(n)
    facts = {71: [4, 5, 6], 1000: (17, 88), 16400: (32, 1367), 40000: (37, 3402), 4: [2, 3], 10: [8, 9], 11: [4, 5, 6, 7, 8, 9],
             70: [4, 5, 6, 7, 8, 9]}
    if n in facts:
        assert got == facts[n] if isinstance(facts[n], list) else (len(got), got[-1]) == facts[n]


@pytest.mark.parametrize("n", [1, 2, 3])
def test_lengths_below_four_raise(n):
    with pytest.raises(ValueError, match="nvals"):
        oracle.scales(n)
    with pytest.raises(ValueError, match="nvals"):
        cases.engine(None, W=n, dry_run=True)


def test_slope_weights_are_the_issue_s():
    for n, want in ((1000, 0.92), (40000, 0.44), (71, 5.1)):
        assert abs(np.sum(np.abs(oracle.slope_weights(oracle.scales(n)))) - want) < 0.05 * want


# ---- the float64 restatement -----------------------------------------------------------------------------------------------
def test_restatement_matches_a_plain_loop():
    x = np.random.default_rng(3).standard_normal(300) * 3 + 1
    nv = oracle.scales(300)
    walk = np.cumsum(x - np.mean(x))
    F = []
    for n in nv:
        fl = []
        for i in range(0, 300 - n, n // 2):
            c = walk[i:i + n]
            t = np.arange(n)
            fl.append(np.sqrt(np.sum((c - np.polyval(np.polyfit(t, c, 1), t)) ** 2) / n))
        F.append(np.sum(fl) / len(fl))
    assert np.allclose(oracle.fluctuations(x), F, rtol=1e-12, atol=0)
    assert abs(oracle.dfa(x) - np.polyfit(np.log(nv), np.log(F), 1)[0]) < 1e-12
    assert np.isnan(oracle.dfa(np.full(100, 2.0))) and oracle.series_value(np.tile([1.0, -1.0], 50)) == 0


@pytest.mark.parametrize("tag", ["a", "b", "c", "e"])
def test_fixture_is_the_oracle_on_the_float64_series(tag):
    cases.check_fixture_oracle(tag)


# ---- the kernel's item code in the emulator --------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(cases.GROUPS))
@pytest.mark.parametrize("W", cases.LENGTHS)
def test_kinds(emu_lib, W, group):
    cases.check_kinds(emu_lib, W, group, hops=2 if W <= 71 else 3)


@pytest.mark.parametrize("W", [1000, 1500])   # (from the filters' 999 taps on: the tests' float64 convolution is np.convolve(..., "same"))
def test_kinds_with_bands(emu_lib, W):
    cases.check_kinds(emu_lib, W, "a", hops=2, bands=["low_beta", "theta"])


def test_orientation_values(emu_lib):
    cases.check_orientation(emu_lib)


def test_long_window_bands(emu_lib):
    cases.check_long_window_bands(emu_lib)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_limit_length(emu_lib, kind):
    cases.check_limit_length(emu_lib, kind)


def test_refusals(emu_lib):
    cases.check_refusals(emu_lib)


def test_sampen_columns_unchanged_and_batch_equals_windows(emu_lib):
    cases.check_sampen_columns_unchanged(emu_lib)


@pytest.mark.parametrize("tag", ["a", "b", "c", "e"])
def test_fixture_pipeline(emu_lib, tag):
    cases.check_fixture_pipeline(emu_lib, tag)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_fixture_direct_and_fused(emu_lib, tag):
    cases.check_fixture_direct(emu_lib, tag)


def test_launch_sequence(emu_lib):
    """DFA adds one launch behind the sample entropy's (alone: in its place) and changes nothing else of the sequence."""
    import ctypes as C

    from tests import nolds_probe_cases as base

    end = emu_lib.lib.nmx_emu_trace_end
    end.restype, end.argtypes = C.c_longlong, [C.c_char_p, C.c_longlong]

    def trace(eng):
        x = base.noise(3, 2, 1200).astype(np.float32)
        buf = C.create_string_buffer(1 << 16)
        emu_lib.lib.nmx_emu_trace_begin()
        eng.process_batch(x, np.array([0, 100, 200]))
        n = end(buf, 1 << 16)
        return [" ".join(ln.split()[:2]) if ln.startswith("op") else ln.split()[0] for ln in buf.raw[:n].decode().splitlines()]

    sampen = trace(base.engine(emu_lib, names=["a", "b"], bands=["low_beta"]))
    both = trace(cases.engine(emu_lib, names=["a", "b"], bands=["low_beta"], sampen=True))
    alone = trace(cases.engine(emu_lib, names=["a", "b"], bands=["low_beta"]))
    at = sampen.index("op be_launch_nolds")
    assert "op be_launch_nolds_dfa" not in sampen
    assert both == sampen[:at + 1] + ["op be_launch_nolds_dfa"] + sampen[at + 1:]
    assert alone == sampen[:at] + ["op be_launch_nolds_dfa"] + sampen[at + 1:]
