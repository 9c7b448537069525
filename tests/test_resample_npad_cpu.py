"""The resampler's fixed padding mode (``resample_npad`` = n samples per side; 100 is what the reference's call of
``mne.filter.resample`` gets) in the single-thread emulator, and the ties that hold its references together: the float64
restatement with MNE's function signature against the independent scipy.signal.resample form and -- with npad = "auto" --
against oracle.mne_restated.resample; the plan arithmetic restated against the case table; the yardstick's chain in float64
against the restatement.  Plus: "auto" is what it was, bit for bit (tests/golden/resample_auto_parent.npz, made on the
parent commit's emulator build).  Cases and policy: tests/resample_npad_cases.py; figures: profiles/resample_npad.md."""

import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import front_probe_cases as fc  # noqa: E402
from tests import resample_npad_cases as cases  # noqa: E402
from tests import resample_npad_oracle as oracle  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


def _scale(y):
    return max(float(np.abs(y).max()), 1e-300)


# ---- ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_oracle_against_scipy_signal_resample(name):
    """resample(x, up, npad=n) == scipy.signal.resample(padded, n_new) * (ratio / (n_new / n_pad)), cropped, at 1e-12 of the
    row's scale -- an independent route through the same definition (scipy handles the Nyquist bin itself)."""
    import scipy.signal as ss

    sf_old, sf_new, Wr, npad, _, _ = cases.CASES[name]
    ratio = sf_new / sf_old
    L = oracle.lengths(Wr, ratio, npad)
    x = np.random.default_rng(Wr).standard_normal((2, Wr)) * 50 + np.array([[300.0], [0.0]])
    got = oracle.resample(x, up=ratio, down=1.0, npad=npad)
    padded = oracle.pad_reflect_limited(x, npad, npad)
    assert padded.shape[-1] == L["n_pad"] == Wr + 2 * npad
    want = ss.resample(padded, L["n_new"], axis=-1) * (ratio / (L["n_new"] / L["n_pad"]))
    want = want[:, L["crop_l"]:L["crop_l"] + L["W_new"]]
    assert got.shape == want.shape == (2, int(round(ratio * Wr)))
    for g, w in zip(got, want):
        assert np.abs(g - w).max() <= 1e-12 * _scale(w), (name, np.abs(g - w).max(), _scale(w))


def test_oracle_defaults_and_auto_is_the_projects_restatement():
    """The signature's default is npad=100; npad="auto" == oracle.mne_restated.resample at 1e-12."""
    import inspect

    from oracle import mne_restated

    sig = inspect.signature(oracle.resample)
    assert sig.parameters["npad"].default == 100 and sig.parameters["npad"].kind is inspect.Parameter.KEYWORD_ONLY
    for name, (sf_old, sf_new, Wr, *_r) in list(cases.CASES.items()) + list(fc.RESAMPLE_CASES.items()):
        x = np.random.default_rng(Wr + 1).standard_normal((2, Wr)) * 50 + 300.0
        got = oracle.resample(x, up=sf_new / sf_old, down=1.0, npad="auto")
        want = mne_restated.resample(x, up=sf_new / sf_old, down=1.0)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * _scale(want), name
    x = np.arange(8.0)[None, :]
    assert np.array_equal(oracle.resample(x, up=0.5), oracle.resample(x, up=0.5, npad=100))
    # reflect_limited: W = 4, npad = 100 -> 3 reflected samples and 97 zeros per side
    xe = oracle.pad_reflect_limited(np.array([[1.0, 2.0, 4.0, 8.0]]), 100, 100)[0]
    assert xe.shape == (204,) and not xe[:97].any() and not xe[-97:].any()
    assert np.array_equal(xe[97:100], [2 - 8, 2 - 4, 2 - 2]) and np.array_equal(xe[104:107], [16 - 4, 16 - 2, 16 - 1])
    for bad in ("foo", -1, 1.5, True):
        with pytest.raises(ValueError):
            oracle.lengths(100, 0.5, bad)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_restated_plan_and_chain_against_the_oracle(name):
    """npad_plan's lengths are the oracle's; resample64 on that plan and the yardstick's chain run in float64 equal the
    oracle at 1e-12; the yardstick itself within YARD_CAP eps32 of the row's scale (check_resampled asserts it)."""
    sf_old, sf_new, Wr, npad, _, _ = cases.CASES[name]
    p = cases.case_plan(name)
    L = oracle.lengths(Wr, sf_new / sf_old, npad)
    assert {k: p[k] for k in L} == L
    for cls, x in cases.inputs(name, p):
        xc = np.nan_to_num(x).astype(np.float64)
        want = oracle.resample(xc, up=sf_new / sf_old, down=1.0, npad=npad)
        got = cases.resample64(xc, p)
        assert got.shape == want.shape == (cases.C, p["W_new"])
        assert np.abs(got - want).max() <= 1e-12 * _scale(want), (name, cls, np.abs(got - want).max())
        ch = cases.chain(xc, p, np.float64)
        assert np.abs(ch - want).max() <= 1e-12 * _scale(want), (name, cls, np.abs(ch - want).max())
        y32 = cases.chain32(xc, p)
        cases.check_resampled(f"npad/{name}", cls + " (yardstick)", y32, got, y32, xc, p)
    fc.REPORT.flush(f"npad/{name}")


def test_case_table_reaches_every_form():
    plans = {n: cases.case_plan(n) for n in cases.CASES}
    forms = {(bool(p["poly_q"]), bool(p["fwd_full"]), bool(p["inv_full"])) for p in plans.values()}
    assert forms >= {(False, False, False), (False, False, True), (False, True, False), (False, True, True),
                     (True, False, False), (True, False, True)}
    assert any(p["poly_q"] % 2 for p in plans.values() if p["poly_q"]), "an odd q: the unpaired last component"
    assert any(p["poly_q"] and p["poly_q"] % 2 == 0 for p in plans.values())
    assert plans["tie_crop"]["crop_l"] == 12 == round(12.5)            # half-even
    assert len(cases.positions(plans["poly_forced_240"], every=True)) == 40
    for p in plans.values():   # (a few windows per case)
        assert len(cases.positions(p)) <= 30 and {0, p["W"] - 1, p["W"] // 2} <= set(cases.positions(p))
    api = (ROOT / "py_neuromodulation_amd" / "csrc" / "nmx_api.hip").read_text()
    assert f"if (A.gen) NMX_LAUNCH({cases.KERNEL}," in api and f"else NMX_LAUNCH({fc.RESAMPLE}," in api
    state = (ROOT / "py_neuromodulation_amd" / "csrc" / "nmx_engine_plan_state.inc").read_text()
    assert "if (n_pad % t == 0 && n_pad / t <= 2048 && layout(n_pad / t, 0)) q = t;" in state
    assert "const int n_fwd = (n_pad & 1) ? n_pad : n_pad / 2;" in state


# ---- the kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_fixed_pad_through_preprocess_window(emu_lib, name):
    worst = cases.run_case(emu_lib, name)
    assert {"impulse", "noise"} <= set(worst) and ("tone" in worst) == (cases.case_plan(name)["nyq_bin"] >= 0)


def test_both_modes_meet_the_same_series_at_the_shared_lengths(emu_lib):
    assert set(cases.both_modes_case(emu_lib)) == {"auto", 100}


@pytest.mark.parametrize("with_notch", [False, True])
def test_fixed_pad_in_a_batch_through_the_tap(emu_lib, with_notch):
    cases.batch_case(emu_lib, with_notch)


def test_required_windows_build(emu_lib):
    """Every raw window the issue names, brought to 1 kHz with npad = 100: the dry plan carries the mode, the restated
    arithmetic finds a form, and the library builds the plan."""
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    for W in cases.REQUIRED_WINDOWS:
        p = cases.npad_plan(float(W), 1000.0, W, 100)
        eng = HotPathEngine(NMSettings.get_default(), ["a", "b"], 1000.0, features=["return_raw"], resample_from=float(W),
                            raw_window=W, dry_run=True, resample_npad=100)
        assert (eng.W_in, eng.W, eng.desc.resample_npad_mode, eng.desc.resample_npad) == (W, 1000, 1, 100), W
        assert p["n_pad"] == W + 200 and (p["poly_q"] == 0 or p["n_pad"] % p["poly_q"] == 0 and p["poly_m"] <= 2048), W
        cases.engine(emu_lib, {}, float(W), 1000.0, W, 2, 100).close()


# ---- the keyword --------------------------------------------------------------------------------------------------------
def _dry(**kw):
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    return HotPathEngine(NMSettings.get_default(), ["a", "b"], 1000.0, features=["return_raw"], resample_from=2000.0,
                         raw_window=2000, dry_run=True, **kw)


def test_keyword_values_and_refusals(emu_lib, monkeypatch):
    from py_neuromodulation_amd.plan_desc import PlanBuilder, resample_npad_arg
    from py_neuromodulation_amd.processing import Resampler

    monkeypatch.delenv("NMX_RESAMPLE_NPAD", raising=False)
    assert resample_npad_arg() == resample_npad_arg("auto") == "auto" and resample_npad_arg(0) == 0
    assert resample_npad_arg(np.int64(100)) == 100
    for bad in ("foo", "100", -1, 1.5, True, [100], b"auto"):
        with pytest.raises(ValueError, match="resample_npad must be 'auto' or an int >= 0"):
            resample_npad_arg(bad)
        with pytest.raises(ValueError, match="resample_npad"):
            _dry(resample_npad=bad)
        with pytest.raises(ValueError):
            Resampler(2000.0, 1000.0, npad=bad)
    d = _dry().desc
    assert (d.resample_npad_mode, d.resample_npad) == (0, 0)                       # zero-initialised: "auto"
    d = _dry(resample_npad=0).desc
    assert (d.resample_npad_mode, d.resample_npad) == (1, 0)                       # npad = 0 is a fixed value
    from py_neuromodulation_amd import NMSettings

    assert PlanBuilder(NMSettings.get_default(), ["a"], 1000.0, ["return_raw"], resample_npad=7).resample_npad == 7
    # the padded limit, by the keyword and by the library itself
    with pytest.raises(ValueError, match=r"raw window 65336 \+ 2 x resample_npad 101 = 65538 samples exceeds the padded limit of 65 536"):
        cases.engine(None, {}, 65336.0, 1000.0, 65336, 1, 101, dry_run=True)
    eng = cases.engine(None, {}, 65336.0, 1000.0, 65336, 1, 100, dry_run=True)
    eng.desc.resample_npad = 101
    import ctypes as C

    plan = C.c_void_p()
    with pytest.raises(ValueError, match=r"raw window 65 336 \+ 2 x npad 101 = 65538 samples exceeds the padded limit of 65 536"):
        emu_lib.check(emu_lib.lib.nmx_plan_create(C.byref(eng.desc), C.byref(plan)))
    eng.desc.resample_npad, eng.desc.resample_npad_mode = 100, 2
    with pytest.raises(ValueError, match="resample_npad_mode must be 0"):
        emu_lib.check(emu_lib.lib.nmx_plan_create(C.byref(eng.desc), C.byref(plan)))
    # a padded length without a polyphase split: 2 x 8009 (prime) forced into the long form
    with pytest.raises(ValueError, match=r"no polyphase split of the padded window \(raw window 15 818, n_pad 16 018, n_new 1 013\)"):
        cases.engine(emu_lib, {}, 15818.0, 1000.0, 15818, 1, 100)
    with pytest.raises(ValueError):
        cases.npad_plan(15818.0, 1000.0, 15818, 100)


def test_environment_variable_supplies_the_keyword(monkeypatch):
    from py_neuromodulation_amd.processing import Resampler

    monkeypatch.setenv("NMX_RESAMPLE_NPAD", "100")
    assert (_dry().desc.resample_npad_mode, _dry().desc.resample_npad, _dry().resample_npad) == (1, 100, 100)
    assert _dry(resample_npad="auto").desc.resample_npad_mode == 0                 # the keyword wins
    assert _dry(resample_npad=3).desc.resample_npad == 3
    assert Resampler(2000.0, 1000.0).npad == 100 and Resampler(2000.0, 1000.0, npad="auto").npad == "auto"
    monkeypatch.setenv("NMX_RESAMPLE_NPAD", "auto")
    assert _dry().desc.resample_npad_mode == 0
    for bad in ("-1", "1.5", "yes"):
        monkeypatch.setenv("NMX_RESAMPLE_NPAD", bad)
        with pytest.raises(ValueError, match="NMX_RESAMPLE_NPAD must be 'auto' or an integer >= 0"):
            _dry()
    monkeypatch.delenv("NMX_RESAMPLE_NPAD")
    assert _dry().resample_npad == "auto"


def test_keyword_reaches_the_plan_through_every_class(emu_lib, monkeypatch):
    """Stream, DataProcessor (and its twin for another window length), MultiDeviceProcessor, ShardedStream: the plan
    description of each carries the mode; Stream's settings token tells the modes apart."""
    from py_neuromodulation_amd import NMSettings, Stream
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.sharding import MultiDeviceProcessor, ShardedStream

    monkeypatch.delenv("NMX_RESAMPLE_NPAD", raising=False)
    s = NMSettings.get_default()
    for f in s.features.get_enabled():
        setattr(s.features, f, False)
    s.features.raw_hjorth = True
    s.postprocessing.feature_normalization = False
    data = np.random.default_rng(0).standard_normal((3, 5200))

    def mode(engine):
        return (engine.desc.resample_npad_mode, engine.desc.resample_npad)

    st = Stream(sfreq=2000.0, data=data, settings=s, lib=emu_lib, resample_npad=100)
    assert mode(st.data_processor.engine) == (1, 100)
    auto = Stream(sfreq=2000.0, data=data, settings=s, lib=emu_lib)
    assert mode(auto.data_processor.engine) == (0, 0) and auto._processor_token() != st._processor_token()
    dp = DataProcessor(2000.0, s, st.channels, line_noise=50, lib=emu_lib, resample_npad=100, verbose=False)
    assert mode(dp.engine) == (1, 100) and mode(dp._twin(2001).engine) == (1, 100) and dp._twin(2001).engine.W_in == 2001
    md = MultiDeviceProcessor(2000.0, s, st.channels, line_noise=50, devices=[0, 0], lib=emu_lib, resample_npad=100)
    assert [mode(p.engine) for p in md.parts] == [(1, 100), (1, 100)]
    sh = ShardedStream(2000.0, st.channels, s, rank=0, world_size=1, device=0, lib=emu_lib, resample_npad=100)
    assert mode(sh._processor(None, dry_run=True).engine) == (1, 100)
    with pytest.raises(ValueError, match="resample_npad"):
        Stream(sfreq=2000.0, data=data, settings=s, lib=emu_lib, resample_npad=-3)


# ---- the stand-alone float64 Resampler ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,to,T,npad", cases.F64_SHAPES)
def test_standalone_float64(emu_lib, fs, to, T, npad):
    assert cases.standalone_case(emu_lib, fs, to, T, npad) <= 1.0


def test_standalone_auto_entry_forwards(emu_lib):
    """nmx_resample_f64 == nmx_resample_f64_npad(.., -1), byte for byte, and both are the "auto" restatement."""
    from oracle import mne_restated

    x = np.random.default_rng(5).standard_normal((2, 1375)) * 10 + 100
    want = mne_restated.resample(x, up=1000 / 1375, down=1.0)
    a, b = np.empty_like(want), np.empty_like(want)
    L, n = emu_lib, want.shape[1]
    L.check(L.lib.nmx_resample_f64(0, x.ctypes.data, 1375, 2, 1375, 1000 / 1375, a.ctypes.data, n, n))
    L.check(L.lib.nmx_resample_f64_npad(0, x.ctypes.data, 1375, 2, 1375, 1000 / 1375, b.ctypes.data, n, n, -1))
    assert np.array_equal(a, b) and np.abs(a - want).max() <= 1e-12 * _scale(want)


# ---- "auto" unchanged ---------------------------------------------------------------------------------------------------
def test_auto_is_bit_identical_to_the_parent_commit(emu_lib, monkeypatch):
    """tests/golden/resample_auto_parent.npz holds what the parent commit's emulator build stored for four "auto" cases, and
    the kernel names it reported (make_resample_auto_parent.py): same bytes, same names -- with no keyword, and with
    resample_npad="auto"."""
    sys.path.insert(0, str(GOLDEN))
    import make_resample_auto_parent as maker

    monkeypatch.delenv("NMX_RESAMPLE_NPAD", raising=False)
    want = np.load(GOLDEN / "resample_auto_parent.npz")
    got = maker.auto_outputs(emu_lib)
    assert set(got) == set(want.files) == set(maker.CASES) | {"kernels_json"}
    for name in maker.CASES:
        assert got[name].dtype == want[name].dtype == np.float32 and got[name].shape == want[name].shape, name
        assert got[name].tobytes() == want[name].tobytes(), f"{name}: {int((got[name] != want[name]).sum())} samples differ"
    assert json.loads(bytes(got["kernels_json"])) == json.loads(bytes(want["kernels_json"]))
    name = "up_odd"
    sf_old, sf_new, Wr, env, _, _ = fc.RESAMPLE_CASES[name]
    p = fc.case_plan(name)
    eng = cases.engine(emu_lib, env, sf_old, sf_new, Wr, fc.RESAMPLE_C, "auto")
    try:
        rows = np.stack([eng.preprocess_window(x.astype(np.float64)).astype(np.float32) for _, x in fc.resample_inputs(name, p)])
    finally:
        eng.close()
    assert rows.tobytes() == want[name].tobytes()


# ---- the reference's own tables -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", cases.STREAM_TAGS)
def test_stream_against_the_references_tables(emu_lib, tag):
    cases.stream_case(emu_lib, tag)


def test_reference_fixture_holds_data_only():
    g = np.load(GOLDEN / "resample_npad.npz", allow_pickle=False)
    assert sorted(g.files) == sorted(f"{t}_{k}" for t in cases.STREAM_TAGS
                                     for k in ("sfreq", "data", "settings_json", "columns", "values", "channels_json"))
    for t in cases.STREAM_TAGS:
        assert g[f"{t}_data"].shape == (3, int(2.6 * float(g[f"{t}_sfreq"]))) and g[f"{t}_values"].shape == (17, 40)
        assert json.loads(str(g[f"{t}_settings_json"]))["preprocessing"] == ["raw_resampling", "notch_filter", "re_referencing"]
    assert (GOLDEN / "resample_npad.npz").stat().st_size < 1 << 20 and (GOLDEN / "resample_auto_parent.npz").stat().st_size < 1 << 20
