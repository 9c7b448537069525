"""nolds Hurst exponent (features/nolds.py; nolds.hurst_rs with its final fit "poly") without a GPU: the per-measure opt-in
(keyword mapping and NMX_NOLDS_FIT), key layout, tables and construction errors on dry_run plans; the float64 restatement
(tests/nolds_hurst_oracle.py) against a plain loop and the reference-generated fixture; and the kernel's item code in the
single-thread emulator (tests/emu/nmx_emu.cpp) on the cases of tests/nolds_hurst_cases.py -- the same cases
tests/test_nolds_hurst_gpu.py runs on the device."""

import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import nolds_hurst_cases as cases  # noqa: E402
from tests import nolds_hurst_oracle as oracle  # noqa: E402
from tests.helpers import load_golden, settings_from_json  # noqa: E402

HURST, DFA, FIT = cases.HURST, cases.DFA, cases.FIT
MEASURES = ["sample_entropy", "correlation_dimension", "lyapunov_exponent", HURST, DFA]


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


@pytest.fixture(autouse=True)
def no_variable(monkeypatch):
    monkeypatch.delenv("NMX_NOLDS_FIT", raising=False)


# ---- surface: the per-measure opt-in, keys, tables (no device) -------------------------------------------------------------
def test_the_mapping_builds_a_plan_with_hurst():
    from py_neuromodulation_amd import _lib, plan_desc

    eng = cases.engine(None, names=["a", "b"], bands=["low_beta"], nolds_fit={HURST: "poly"}, dry_run=True)
    d = eng.desc
    assert d.nolds_measures == 8 and d.nolds_measures & 8 and d.nolds_hurst_fit == 1 and d.nolds_dfa_fit == 0
    assert d.abi_version == _lib.NMX_ABI_VERSION == 17
    assert cases.table(d) == cases.TABLE_FACTS[1000] == oracle.scales(1000) == plan_desc.hurst_scales(1000)
    log_e = [d.nolds_hurst_log_expected[k] for k in range(d.nolds_hurst_n_scales)]
    assert log_e == [math.log(oracle.expected_rs(n)) for n in cases.TABLE_FACTS[1000]]
    assert eng.keys == [f"{ch}_nolds_{HURST}_{s}" for s in ("raw", "low_beta") for ch in ("a", "b")]
    assert (d.nolds_hurst_cols.base, d.nolds_hurst_cols.ch_stride, d.nolds_hurst_cols.a_stride) == (0, 1, 2)
    assert d.nolds_n_taps[0] == 999 and d.n_filters == 0   # (the band filters run exactly as for a sample-entropy plan)


def test_three_measures_stand_in_get_enabled_order():
    eng = cases.engine(None, names=["a", "b"], bands=["low_beta"], sampen=True, dfa=True, dry_run=True)
    d = eng.desc
    assert d.nolds_measures == 1 | 8 | 16 and d.nolds_hurst_fit == 1 and d.nolds_dfa_fit == 1
    order = ["sample_entropy", HURST, DFA]
    assert eng.keys == [f"{ch}_nolds_{f}_{s}" for s in ("raw", "low_beta") for ch in ("a", "b") for f in order]
    for j, cols in enumerate((d.nolds_cols, d.nolds_hurst_cols, d.nolds_dfa_cols)):
        assert (cols.base, cols.ch_stride, cols.a_stride) == (j, 3, 6)


def test_expected_rs_facts():
    from py_neuromodulation_amd import plan_desc

    facts = {2: 0.75, 3: 1.1253953951963827, 13: 3.420392310521661, 340: 21.960745554092167, 341: 21.94626699311547}
    for n, want in facts.items():
        assert abs(oracle.expected_rs(n) - want) <= 1e-14 * want and plan_desc.hurst_expected_rs(n) == oracle.expected_rs(n)
    assert oracle.expected_rs(341) < oracle.expected_rs(340)   # (nolds' own switch is not continuous)


@pytest.mark.parametrize("n", sorted(cases.TABLE_FACTS))
def test_scale_table_is_the_issue_s(n):
    from py_neuromodulation_amd import plan_desc

    got = cases.table(cases.engine(None, W=n, dry_run=True).desc)
    assert got == oracle.scales(n) == plan_desc.hurst_scales(n) and 2 <= len(got) <= 15
    fact = cases.TABLE_FACTS[n]
    if isinstance(fact, list):
        assert got == fact
    else:
        count, first, before_last, last = fact
        assert (len(got), got[0], got[-1]) == (count, first, last) and before_last in (None, got[-2])


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_lengths_below_five_raise(n):
    from py_neuromodulation_amd import plan_desc

    with pytest.raises(ValueError):
        oracle.scales(n)
    with pytest.raises(ValueError, match="hurst_exponent"):
        plan_desc.hurst_scales(n)
    with pytest.raises(ValueError, match="hurst_exponent"):
        cases.engine(None, W=n, dry_run=True)


@pytest.mark.parametrize("fit", [None, "RANSAC", "poly", {}, {HURST: "RANSAC"}, {HURST: None}, {DFA: "poly"}])
def test_without_its_entry_hurst_raises_as_before(fit):
    with pytest.raises(NotImplementedError, match=HURST) as e:
        cases.engine(None, nolds_fit=fit, dry_run=True)
    assert str(e.value) == (
        f"nolds measures ['{HURST}'] are not implemented: the reference ends them in a line fit that defaults to "
        "fit='RANSAC' -- scikit-learn's RANSACRegressor without a seed -- so two runs of the reference do not agree "
        "with each other and no parity can be checked; only sample_entropy runs on the device")


def test_the_string_poly_still_means_dfa_alone():
    from tests import nolds_dfa_cases

    d = nolds_dfa_cases.engine(None, nolds_fit="poly", dry_run=True).desc
    assert d.nolds_measures == 16 and d.nolds_dfa_fit == 1 and d.nolds_hurst_fit == 0 and d.nolds_hurst_n_scales == 0
    same = nolds_dfa_cases.engine(None, nolds_fit={DFA: "poly"}, dry_run=True)
    assert same.desc.nolds_dfa_fit == 1 and same.keys == nolds_dfa_cases.engine(None, dry_run=True).keys
    with pytest.raises(NotImplementedError, match=DFA):
        nolds_dfa_cases.engine(None, nolds_fit={HURST: "poly"}, dry_run=True)


@pytest.mark.parametrize("fit", [{"hurst": "poly"}, {"Hurst_exponent": "poly"}, {1: "poly"}, {HURST: "Poly"}, {HURST: 1},
                                 {HURST: True}, {HURST: "lstsq"}, {HURST: "poly", "dfa": "poly"}, [HURST], (HURST, "poly")])
def test_a_bad_key_or_value_is_a_value_error(fit):
    with pytest.raises(ValueError, match="nolds_fit"):
        cases.engine(None, nolds_fit=fit, dry_run=True)


@pytest.mark.parametrize("measure", ["correlation_dimension", "lyapunov_exponent"])
def test_poly_parses_for_the_two_without_a_kernel_and_they_keep_raising(measure):
    from py_neuromodulation_amd.engine import HotPathEngine
    from py_neuromodulation_amd.plan_desc import nolds_fit_arg

    fit = {m: "poly" for m in MEASURES}
    assert nolds_fit_arg(fit) == fit and list(nolds_fit_arg(dict(reversed(list(fit.items()))))) == MEASURES
    s = cases.hurst_settings()
    s.nolds_settings.features = {HURST: True, measure: True}
    with pytest.raises(NotImplementedError, match=measure) as e:
        HotPathEngine(s, ["a"], 1000.0, dry_run=True, nolds_fit=fit)
    assert "RANSAC" in str(e.value) and HURST not in str(e.value)


def test_the_variable_takes_the_mapping_form(monkeypatch):
    monkeypatch.setenv("NMX_NOLDS_FIT", f"{HURST}:poly,{DFA}:poly")
    d = cases.engine(None, nolds_fit=None, dfa=True, dry_run=True).desc
    assert d.nolds_hurst_fit == 1 and d.nolds_dfa_fit == 1 and d.nolds_measures == 24
    monkeypatch.setenv("NMX_NOLDS_FIT", f" {HURST} : poly ")
    assert cases.engine(None, nolds_fit=None, dry_run=True).desc.nolds_hurst_fit == 1
    with pytest.raises(NotImplementedError, match=HURST):   # (the keyword wins, the empty mapping included)
        cases.engine(None, nolds_fit="RANSAC", dry_run=True)
    with pytest.raises(NotImplementedError, match=HURST):
        cases.engine(None, nolds_fit={}, dry_run=True)
    with pytest.raises(NotImplementedError, match=HURST):
        cases.engine(None, nolds_fit="poly", dry_run=True)
    monkeypatch.setenv("NMX_NOLDS_FIT", "poly")   # (the plain form keeps its meaning: DFA alone)
    with pytest.raises(NotImplementedError, match=HURST):
        cases.engine(None, nolds_fit=None, dry_run=True)
    assert cases.engine(None, nolds_fit={HURST: "poly"}, dry_run=True).desc.nolds_hurst_fit == 1
    monkeypatch.setenv("NMX_NOLDS_FIT", f"{HURST}:RANSAC")
    with pytest.raises(NotImplementedError, match=HURST):
        cases.engine(None, nolds_fit=None, dry_run=True)
    for bad in (f"{HURST}:huber", "hurst:poly", f"{HURST}:poly,", f"{HURST}:poly:x", f"{HURST}:poly,{HURST}:RANSAC",
                f"{HURST}:None", f"{HURST}=poly", "huber"):
        monkeypatch.setenv("NMX_NOLDS_FIT", bad)
        with pytest.raises(ValueError, match="NMX_NOLDS_FIT"):
            cases.engine(None, nolds_fit=None, dry_run=True)


def test_every_class_takes_the_mapping(monkeypatch):
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.features import Nolds
    from py_neuromodulation_amd.plan_desc import PlanBuilder
    from py_neuromodulation_amd.sharding import MultiDeviceProcessor, ShardedStream
    from py_neuromodulation_amd.stream import Stream

    g = load_golden("nolds_hurst")
    s = settings_from_json(g["b_settings_json"])
    ch = json.loads(str(g["b_channels_json"]))
    want = [str(c) for c in g["b_columns"] if str(c) != "time"]
    for fit in (None, "poly"):
        with pytest.raises(NotImplementedError, match=HURST):
            DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True, nolds_fit=fit)
    assert DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True, nolds_fit=FIT).keys == want
    with pytest.raises(NotImplementedError, match=HURST):
        Nolds(s, [], 1000.0, nolds_fit="poly")
    assert Nolds(s, [], 1000.0, nolds_fit=FIT).keys == []
    assert PlanBuilder(s, ["a"], 1000.0, features=["nolds"], nolds_fit=FIT).nolds_fit == FIT
    sh = ShardedStream(1000.0, ch, s, rank=0, world_size=1, local_input=True, nolds_fit=FIT)
    assert sh._dp.keys == want
    # (Stream builds its processor at once: tests/nolds_hurst_cases.py check_fixture_pipeline runs it with the mapping)
    with pytest.raises(ValueError, match="nolds_fit"):
        Stream(sfreq=1000.0, channels=ch, settings=s, line_noise=50, nolds_fit={"hurst": "poly"})
    import inspect

    assert "nolds_fit" in inspect.signature(MultiDeviceProcessor.__init__).parameters
    monkeypatch.setenv("NMX_NOLDS_FIT", f"{HURST}:poly,{DFA}:poly")
    assert DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True).keys == want
    assert Nolds(s, [], 1000.0).keys == []


@pytest.mark.parametrize("tag", ["a", "b", "c", "e"])
def test_pipeline_keys_in_reference_order(tag):
    """Hurst alone (a, c), all three measures (b), sample entropy and Hurst with raw off (e)"""
    from py_neuromodulation_amd.data_processor import DataProcessor

    g = load_golden("nolds_hurst")
    s = settings_from_json(g[f"{tag}_settings_json"])
    ch = json.loads(str(g[f"{tag}_channels_json"]))
    dp = DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True, nolds_fit=FIT)
    assert dp.keys == [str(c) for c in g[f"{tag}_columns"] if str(c) != "time"]


def test_slope_weights_are_the_issue_s():
    for n, want in ((5, 4.93), (1000, 1.72), (40000, 1.13)):
        assert abs(np.sum(np.abs(oracle.slope_weights(oracle.scales(n)))) - want) < 0.005 * want + 0.005
        assert abs(oracle.h_limit(oracle.scales(n)) - 1e-5 * want) < 1e-7


# ---- the float64 restatement -----------------------------------------------------------------------------------------------
def test_restatement_matches_a_plain_loop():
    x = np.random.default_rng(3).standard_normal(300) * 3 + 1
    x[100:140] = 2.5   # (constant chunks at the small scales)
    nv = oracle.scales(300)
    rs, kept = oracle.rs_values(x)
    plain = [oracle.rs_plain_loop(x, n) for n in nv]
    assert kept.tolist() == [p[1] for p in plain] and any(k < 300 // n for k, n in zip(kept, nv))
    assert np.allclose(rs, [p[0] for p in plain], rtol=1e-12, atol=0)
    y = np.log(rs) - np.log([oracle.expected_rs(n) for n in nv])
    assert abs(oracle.hurst(x) - (np.polyfit(np.log(nv), y, 1)[0] + 0.5)) < 1e-12
    w = oracle.slope_weights(nv)
    assert abs(oracle.hurst(x) - (float(np.dot(w, y)) + 0.5)) < 1e-12   # (the weights are the slope's exact sensitivities)
    assert math.isnan(oracle.hurst(np.full(100, 2.0))) and oracle.series_value(np.tile([1.0, -1.0], 50)) == 0


def test_orientation_values():
    """white noise near 0.5, its cumulative sum near 1 (the corrected R/S estimate; loose bands, one seed)"""
    n = np.random.default_rng(0).standard_normal(1000)
    assert 0.35 < oracle.hurst(n) < 0.7 and 0.85 < oracle.hurst(np.cumsum(n)) < 1.15


def test_constructed_series_on_the_oracle():
    cases.check_constructed_oracle()


@pytest.mark.parametrize("tag", ["a", "b", "c", "e"])
def test_fixture_is_the_oracle_on_the_float64_series(tag):
    cases.check_fixture_oracle(tag)


# ---- the kernel's item code in the emulator --------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(cases.GROUPS))
@pytest.mark.parametrize("W", cases.LENGTHS)
def test_kinds(emu_lib, W, group):
    cases.check_kinds(emu_lib, W, group, hops=2 if W <= 100 or W > 8000 else 3)


@pytest.mark.parametrize("W", [1000, 1500])   # (from the filters' 999 taps on: the tests' float64 convolution is np.convolve(..., "same"))
def test_kinds_with_bands(emu_lib, W):
    cases.check_kinds(emu_lib, W, "a", hops=2, bands=["low_beta", "theta"])


def test_six_hops_three_channels(emu_lib):
    cases.check_kinds(emu_lib, 1000, "a", hops=6)


def test_constructed_series(emu_lib):
    cases.check_constructed(emu_lib)


def test_two_sample_chunks(emu_lib):
    cases.check_two_sample_chunks(emu_lib)


def test_amplitudes(emu_lib):
    cases.check_amplitudes(emu_lib)


def test_long_window_bands(emu_lib):
    cases.check_long_window_bands(emu_lib)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_limit_length(emu_lib, kind):
    cases.check_limit_length(emu_lib, kind)


def test_refusals(emu_lib):
    cases.check_refusals(emu_lib)


def test_other_columns_unchanged_and_batch_equals_windows(emu_lib):
    cases.check_other_columns_unchanged(emu_lib)


@pytest.mark.parametrize("tag", ["a", "b", "c", "e"])
def test_fixture_pipeline(emu_lib, tag):
    cases.check_fixture_pipeline(emu_lib, tag)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_fixture_direct_and_fused(emu_lib, tag):
    cases.check_fixture_direct(emu_lib, tag)


def test_launch_sequence(emu_lib):
    """Hurst adds one launch to the DFA plan's sequence (between the sample entropy's and the DFA's) and changes nothing
    else; plans without Hurst contain no such launch."""
    import ctypes as C

    from tests import nolds_dfa_cases
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

    kw = dict(names=["a", "b"], bands=["low_beta"])
    sampen = trace(base.engine(emu_lib, **kw))
    dfa = trace(nolds_dfa_cases.engine(emu_lib, **kw))
    two = trace(nolds_dfa_cases.engine(emu_lib, sampen=True, **kw))
    op = "op be_launch_nolds_hurst"
    assert op not in sampen and op not in dfa and op not in two
    at = dfa.index("op be_launch_nolds_dfa")
    assert trace(cases.engine(emu_lib, dfa=True, **kw)) == dfa[:at] + [op] + dfa[at:]
    at = two.index("op be_launch_nolds_dfa")
    assert trace(cases.engine(emu_lib, sampen=True, dfa=True, **kw)) == two[:at] + [op] + two[at:]
    alone = trace(cases.engine(emu_lib, **kw))
    at = dfa.index("op be_launch_nolds_dfa")
    assert alone == dfa[:at] + [op] + dfa[at + 1:]
