"""Nothing is left behind: every device block and every page-locked block a plan, a feature normaliser or a grid projection
allocates is given back when it is destroyed (Plan::tables and the self-freeing Buf / HostBuf, nmx_engine.inc;
nmx_plan_destroy, nmx_engine_abi.inc).  The logic emulator counts the blocks its be_alloc / be_host_alloc have handed out and
its be_free / be_host_free have not taken back (nmx_emu_live_blocks, an export of the emulator library only): around each
plan below -- built, one host batch, closed -- the count returns to its value from before the engine was built.

3 channels, 1 kHz, 1000-sample windows, 20 hops of 100 samples unless a case says otherwise."""

import ctypes as C
import gc
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SFREQ, W, HOP, CH = 1000.0, 1000, 100, 3


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    lib = _lib.NmxLibrary(ge.build_emu())
    lib.lib.nmx_emu_live_blocks.restype = C.c_longlong
    return lib


@pytest.fixture(autouse=True)
def _no_garbage_of_earlier_tests():
    """The count is the library's, not this file's: an engine or normaliser of an earlier test that still waits for the
    garbage collector would give its blocks back in the middle of a test here."""
    gc.collect()


def _recording(channels, hops, offsets=False, dtype=np.float32):
    rng = np.random.default_rng(7)
    T = W + (hops - 1) * HOP
    x = rng.standard_normal((channels, T)) * 10 + 3 * np.sin(2 * np.pi * 17 * np.arange(T) / SFREQ)
    if offsets:
        x += np.linspace(-3000.0, 5000.0, channels)[:, None]
    return x.astype(dtype), np.arange(hops) * HOP


def _engine(lib, features, channels=CH, **kw):
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    s = NMSettings.get_default()
    s.bursts_settings.time_duration_s = 2
    s.bandpass_filter_settings.kalman_filter = True
    return HotPathEngine(s, [f"ch{i}" for i in range(channels)], SFREQ, lib=lib, features=list(features), window=W, **kw)


def _notch():
    from py_neuromodulation_amd import fir_design

    return fir_design.notch_bank(SFREQ, 50)


def _car(n):
    return np.eye(n) - np.full((n, n), 1.0 / n)


def _structured(n=7):
    """Six rows re-referenced to the average of the other five (a group sum), one bipolar row: taps + group sums, not a
    common average"""
    R = np.eye(n)
    R[:n - 1, :n - 1] -= (1.0 - np.eye(n - 1)) / (n - 2)
    R[n - 1, 0] = -1.0
    return R


def _dense(n=6):
    return np.random.default_rng(3).standard_normal((n, n))


def _run(eng, hops=20, channels=CH, offsets=False, **kw):
    x, starts = _recording(channels, hops, offsets)
    return eng.process_batch(x, starts, **kw)


def _pre_filter():
    from py_neuromodulation_amd import fir_design

    return [fir_design.band_pass_bank([(4.0, 80.0)], SFREQ)[0]]


# name -> (engine arguments, what runs on it)
PLANS = {
    "hjorth": (dict(features=["raw_hjorth"]), _run),
    "hjorth_400_hops": (dict(features=["raw_hjorth"]), lambda e: _run(e, hops=400)),   # both x_in2 buffers
    **{f"rawnorm_{m}": (dict(features=["return_raw", "raw_hjorth"], raw_norm=(m, 0, 700, HOP)), _run)
       for m in ("zscore", "median", "quantile", "power")},
    "bursts_sharpwaves": (dict(features=["bursts", "sharpwave_analysis"]), _run),
    "bandpass_kalman": (dict(features=["bandpass_filter"]), _run),
    "reref_car_notch": (dict(features=["raw_hjorth", "fft"], ref_matrix=_car(CH), notch_taps=_notch()), lambda e: _run(e, offsets=True)),
    "reref_structured_notch": (dict(features=["raw_hjorth", "fft"], channels=7, ref_matrix=_structured(), notch_taps=_notch()),
                               lambda e: _run(e, channels=7, offsets=True)),
    "reref_dense_notch": (dict(features=["raw_hjorth", "fft"], channels=6, ref_matrix=_dense(), notch_taps=_notch()),
                          lambda e: _run(e, channels=6, offsets=True)),
    "tap": (dict(features=["raw_hjorth"]), lambda e: _run(e, tap=True)),
    "nan_mask": (dict(features=["raw_hjorth"]), lambda e: _run(e, want_nan_mask=True)),
    "process_window": (dict(features=["raw_hjorth"]), lambda e: e.process_window(_recording(CH, 1, dtype=np.float64)[0])),
}


@pytest.mark.parametrize("name", list(PLANS))
def test_a_closed_plan_leaves_no_block(emu_lib, name):
    kw, run = PLANS[name]
    live = emu_lib.lib.nmx_emu_live_blocks
    before = live()
    eng = _engine(emu_lib, **kw)
    built = live()
    run(eng)
    eng.close()
    print(name, "blocks: before", before, "built", built, "closed", live())
    assert built > before
    assert live() == before


def test_in_plan_resampling(emu_lib):
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    live = emu_lib.lib.nmx_emu_live_blocks
    before = live()
    eng = HotPathEngine(NMSettings.get_default(), [f"ch{i}" for i in range(CH)], SFREQ, lib=emu_lib, features=["raw_hjorth"],
                        resample_from=2000.0)
    assert eng.W_in == 2000 and eng.W == 1000
    rng = np.random.default_rng(1)
    eng.process_batch(rng.standard_normal((CH, 2000 + 19 * 200)).astype(np.float32), np.arange(20) * 200)
    eng.close()
    assert live() == before


def test_preprocessing_filter_stage(emu_lib):
    live = emu_lib.lib.nmx_emu_live_blocks
    before = live()
    eng = _engine(emu_lib, ["raw_hjorth"], pre_taps=_pre_filter())
    assert eng.desc.n_pre_filters == 1
    _run(eng)
    eng.close()
    assert live() == before


def test_attached_normaliser_and_projection(emu_lib):
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.processing import DeviceFeatureNormalizer
    from py_neuromodulation_amd.projection import DeviceProjection

    live = emu_lib.lib.nmx_emu_live_blocks
    before = live()
    n_feat = 3   # Hjorth: activity, mobility, complexity
    eng = _engine(emu_lib, ["raw_hjorth"], extra_cols=2 * n_feat)
    F = eng.n_outputs
    assert F == CH * n_feat
    # two grid points over the three channels: columns F + p + 2 f behind the features
    gather = np.array([[eng.keys.index(k) for k in eng.keys if k.startswith(f"ch{c}_")] for c in range(CH)], np.int32)
    lay = SimpleNamespace(n_feat=n_feat, gather=gather, ptr=np.array([0, 2, 3], np.int32), idx=np.array([0, 1, 2], np.int32),
                          w=np.array([0.5, 0.5, 1.0]), out_col=np.array([F, F + 1], np.int32), out_stride=np.array([2, 2], np.int32),
                          group_chan=np.array([0, CH], np.int32), point_group=np.array([0, 0], np.int32))
    proj = DeviceProjection(lay, lib=emu_lib)
    norms = [DeviceFeatureNormalizer(_norm_settings(m), F, colmask=mask, lib=emu_lib)
             for m, mask in (("zscore", None), ("median", np.ones(F, np.uint8)), ("power", None))]
    for norm in norms:   # (mean family with its scan buffer, median family with its sorted copy and a column mask, "power")
        eng.attach_normalizer(norm)
        eng.attach_projection(proj)
        rows = _run(eng)
        assert rows.shape == (20, F + 2 * n_feat)
        np.testing.assert_allclose(rows[:, F], 0.5 * (rows[:, gather[0, 0]] + rows[:, gather[1, 0]]), rtol=1e-6, atol=1e-30)
        norm.process_batch(np.random.default_rng(2).standard_normal((12, F)).astype(np.float32))   # host rows: the staging block
    proj.process(np.zeros((4, F + 2 * n_feat), np.float32))
    eng.attach_normalizer(None)
    eng.attach_projection(None)
    eng.close()
    assert live() > before
    del norm, norms, proj, eng
    gc.collect()
    assert live() == before


def _norm_settings(method):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.feature_normalization_settings.normalization_method = method
    s.feature_normalization_settings.normalization_time_s = 10
    return s


def test_a_plan_whose_creation_fails_leaves_no_block(emu_lib):
    """bandpass_filter without a filter: refused at the end of nmx_plan_create, behind every build step (the time /
    oscillatory tables, the raw normaliser's rings and the offset tables exist by then).  A raw normaliser with N < 2 is
    refused by its own build step, behind the tables of the steps in front of it."""
    live = emu_lib.lib.nmx_emu_live_blocks
    for what, change, message in (
            ("no filter", lambda d: setattr(d, "n_filters", 0), "bandpass_filter enabled without filters"),
            ("N < 2", lambda d: setattr(d, "raw_norm_n", 1), "raw normalisation: need N >= 2")):
        eng = _engine(emu_lib, ["bandpass_filter", "raw_hjorth", "fft"], raw_norm=("median", 0, 700, HOP))
        d = eng.desc
        change(d)
        before = live()
        plan = C.c_void_p()
        rc = emu_lib.lib.nmx_plan_create(C.byref(d), C.byref(plan))
        assert rc != 0 and not plan.value, what
        assert message in emu_lib.lib.nmx_last_error().decode(), what
        assert live() == before, what
        eng.close()
