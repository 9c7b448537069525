"""Sharp waves on windows beyond 14 500 samples on the MI355X (libnmx.so): the dense-first launch with its compact LDS
layout, and the list kernel whose lists live in per-workgroup slabs of device memory (nmx_wave_slab.hip), against the
reference-generated fixture (tests/golden/make_golden_sharpwave_long.py) and the float64 restatement.  Cases and
policy: tests/sharpwave_long_cases.py.  The four positive cases together may accept at most 5 sharp-wave misses on
conditioning reports and none in another family (tests/accepted_miss_budget.json leaves that much room); the counts
observed are in profiles/sharpwave_long.md.  At the parent commit every positive case fails at plan construction."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import sharpwave_long_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

_ACCEPTED = {"sharpwave": 0}


@pytest.mark.parametrize("tag", ["d30k", "d16k", "wide30k", "all30k"])
def test_long_window_case(tag):
    acc = cases.run_case(None, tag)
    assert set(acc) <= {"sharpwave"}, acc
    _ACCEPTED["sharpwave"] += acc.get("sharpwave", 0)
    assert _ACCEPTED["sharpwave"] <= 5, f"sharp-wave misses accepted by the long-window cases so far: {_ACCEPTED}"


def test_notch_in_front_of_long_window_sharp_waves():
    _ACCEPTED["sharpwave"] += cases.notch_case(None)
    assert _ACCEPTED["sharpwave"] <= 5, _ACCEPTED


def test_window_above_the_limit_raises():
    cases.over_limit_raises(None)


def _engine(W, wide=False, all_features=False):
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    s = NMSettings.get_default()
    s.reset()
    s.features.sharpwave_analysis = True
    if wide:
        s.sharpwave_analysis_settings.filter_ranges_hz = [[5, 5000]]
    if all_features:
        sw = s.sharpwave_analysis_settings
        sw.sharpwave_features.enable_all()
        sw.estimator["mean"] = list(sw.sharpwave_features.to_dict())
        sw.estimator["median"] = ["prominence", "interval"]
        sw.estimator["var"] = ["interval", "width"]
    return HotPathEngine(s, ["a", "b"], float(W), features=["sharpwave_analysis"], window=W)


def _batch(e, W, kind, hops=9, seed=5):
    x = cases.recording(seed, W, kind, hops=hops)
    out = e.process_batch(x, np.arange(hops, dtype=np.int64) * (W // 10)).copy()
    return out, e.kernels(5)


def test_kernels_per_mode():
    """Plans that fit the LDS list layout launch what they launched before; longer ones the dense-first kernel plus the
    slab kernel, or the slab kernel alone when the settings rule the dense path out."""
    e = _engine(14000)
    _, k = _batch(e, 14000, "walk")
    e.close()
    assert "nmx_kern_sharp_dense" in k and "nmx_kern_sharp_todo" in k and "slab" not in k, k
    e = _engine(14000, all_features=True)
    _, k = _batch(e, 14000, "walk")
    e.close()
    assert "nmx_kern_sharp" in k and "dense" not in k and "todo" not in k and "slab" not in k, k
    e = _engine(16000)
    _, k = _batch(e, 16000, "walk")
    e.close()
    assert "nmx_kern_sharp_dense" in k and "nmx_kern_sharp_slab" in k and "todo" not in k, k
    e = _engine(16000, all_features=True)
    out, k = _batch(e, 16000, "walk")
    e.close()
    assert "nmx_kern_sharp_slab" in k and "dense" not in k, k
    assert np.isfinite(out).all()
