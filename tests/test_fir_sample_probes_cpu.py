"""Per-sample probes of the FIR kernels in the single-thread emulator (tests/emu/nmx_emu.cpp): the kinds it reaches -- the
one-channel M = 2048 item (bank and notch), the generic LDS kernel and the partitioned overlap-save form -- through
filter_window, preprocess_window and the tap; and the ties that hold the probes' references together: the float64 direct
convolution against the oracle on every tap set, the restated plan arithmetic, the table of kernels against the launchers'
source.  Cases and policy: tests/fir_sample_probe_cases.py; the figures observed are in profiles/fir_sample_probes.md."""

import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import fir_sample_probe_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


def _tap_sets():
    """{label: (taps, window)} of every filter the cases run: the banks' (a dry plan of each case), the notches', the
    pre-filters'."""
    from py_neuromodulation_amd import fir_design
    from py_neuromodulation_amd.engine import HotPathEngine

    out = {}
    for name, (_, sfreq, W, _, kind, bands, *_rest) in cases.BANK_CASES.items():
        eng = HotPathEngine(cases.bank_settings(kind, W, bands), ["a", "b"], sfreq, dry_run=True)
        for i, h in enumerate(eng.filter_taps):
            out.setdefault((sfreq, W, len(h), round(float(h[len(h) // 2]), 12)), (f"{name} filter {i}", h, W, False))
    for name, (_, sfreq, W, _, _, pre, *_rest) in cases.NOTCH_CASES.items():
        h = fir_design.notch_bank(sfreq, 50)
        out.setdefault(("notch", sfreq, W), (f"{name} notch", h, W, True))
        if pre:
            h = cases.pre_taps(pre, sfreq)
            out.setdefault(("pre", pre, sfreq, W), (f"{name} pre-filter", h, W, False))
    return list(out.values())


def test_direct_convolution_is_the_oracles_on_every_tap_set():
    """np.convolve on the explicitly padded window against oracle.nm_oracle.fir_bank_apply (zero padding) and
    mne_restated._overlap_add_filter (odd reflection), and the oaconvolve form of the large cases against both."""
    from oracle import mne_restated
    from oracle import nm_oracle as orc

    sets = _tap_sets()
    assert len(sets) >= 20
    rng = np.random.default_rng(7)
    for label, h, W, odd in sets:
        x = rng.standard_normal((3, W)) * 50 + np.array([[300.0], [0.0], [-20.0]])
        x[1, : W // 3] = 0.0
        want = mne_restated._overlap_add_filter(x, h) if odd else orc.fir_bank_apply(x, h[None, :])[:, 0, :]
        tol = 1e-12 * np.abs(want).max()
        hl = h if odd else cases.live_taps(h, W)
        for fn in (cases.conv64_direct, cases.conv64_bulk):
            got = fn(x, hl, odd)
            assert got.shape == want.shape and np.abs(got - want).max() <= tol, (label, fn.__name__, np.abs(got - want).max(), tol)


def test_the_yardstick_is_an_fp32_convolution():
    """On noise the yardstick's error is of the order of eps32 rms(x) -- not float64 by accident, not broken -- at every
    transform length the kinds use: 0.2 - 4 for a band-pass (4 Hz of 500 pass: most of the transform's rounding is
    filtered away), 0.2 - 10 for the notch, which passes all of it (two 2048-point transforms: 11 stages each way,
    the largest of 1000 samples).  On a unit impulse the output is the taps and the error the rounding of their
    spectrum: about eps32 |h|_2 (Parseval) over the samples, so below 2 eps32 |h|_2 at its largest."""
    from py_neuromodulation_amd import fir_design

    rng = np.random.default_rng(11)
    x = cases._f32(rng.standard_normal((4, 1000)) * 50)
    imp = np.zeros((1, 1000))
    imp[0, 500] = 1.0
    for h, odd, Ms, hi in ((fir_design.band_pass_bank([(4.0, 8.0)], 1000.0)[0], False, (1536, 2048, 1500, 0), 4.0),
                           (fir_design.notch_bank(1000.0, 50), True, (2048,), 10.0)):
        y64 = cases.conv64_direct(x, h, odd)
        for M in Ms:
            e32 = np.abs(cases.conv32(x, h, M, odd) - y64).max(axis=-1) / (cases.EPS32 * cases.rms(x))
            assert np.all((e32 > 0.2) & (e32 < hi)), (M, odd, e32)
            e_imp = np.abs(cases.conv32(imp, h, M, odd) - cases.conv64_direct(imp, h, odd)).max()
            assert 0 < e_imp < 2 * cases.EPS32 * np.sqrt(np.sum(h * h)), (M, odd, e_imp)


def test_restated_plan_arithmetic_and_inputs():
    assert [cases.choose_M(n) for n in (1499, 3998, 1598, 16000)] == [1500, 4000, 1600, 16000]
    for W, pad in ((1000, 499), (901, 499), (500, 0), (2500, 0), (8000, 0)):
        p = cases.positions(W, pad)
        assert p[0] == 0 and p[-1] == W - 1 and {1, W // 2, W - 2} <= set(p) and all(0 <= q < W for q in p)
        assert all({b - 1, b} <= set(p) for b in (24, 32, 64, 256) if b < W)
    x = cases.impulse_inputs(4099, 1000)[0]
    c = np.arange(4099)
    where = x.argmax(axis=1)
    for half in (0, 1):   # every position in either half of a channel pair
        assert set(where[c % 2 == half]) == set(range(1000))
    seen = set()
    for C in (2, 3, 5, 7, 4099):
        calls = cases.noise_inputs(C, 1000, 1)
        n_pairs = C // 2
        assert len(calls) * n_pairs >= len(cases.PAIR_PATTERNS)
        seen |= {bool(z.any()) for _, z in calls}
    assert seen == {True, False}


def test_every_one_wave_fir_kernel_is_asserted_by_a_case():
    """The names the launchers of nmx_w64.hip report (NMX_LAUNCH: the kernel expression, without the parentheses around a
    template-id with commas) and nmx_kern_bank against the kernels the case tables assert."""
    src = (ROOT / "py_neuromodulation_amd" / "csrc" / "nmx_w64.hip").read_text()
    assert "NMX_LAUNCH_AS(" not in src and "NMX_LAUNCH_QUIET(" not in src
    launched = set(re.findall(r"NMX_LAUNCH\(\(?(nmx_kern_\w+(?:<[^>]*>)?)\)?, ", src)) | {"nmx_kern_bank"}
    assert len(launched) == 17, sorted(launched)
    asserted = set()
    for table, col in ((cases.BANK_CASES, 6), (cases.NOTCH_CASES, 6), (cases.TAP_CASES, 4)):
        for row in table.values():
            asserted |= set(row[col].values())
    asserted |= {cases.ONE}   # (the pre-filter stages: notch_case asserts it next to the notch)
    assert launched <= asserted, sorted(launched - asserted)


@pytest.mark.parametrize("name", cases.EMU_BANK)
def test_bank_through_filter_window(emu_lib, name):
    worst = cases.bank_case(emu_lib, name)
    assert set(worst) == {"impulse", "noise", "constant"}


@pytest.mark.parametrize("name", cases.EMU_NOTCH)
def test_notch_and_pre_filters_through_preprocess_window(emu_lib, name):
    worst = cases.notch_case(emu_lib, name)
    assert set(worst) == {"impulse", "noise"}


def test_notch_in_a_batch_through_the_tap(emu_lib):
    """4 channels x 8 hops (the one-channel notch item), and 4 x 40 in chunks of 16 hops: the same bytes as one chunk."""
    cases.tap_case(emu_lib, "tap_4x8")
    cases.tap_case(emu_lib, "tap_4x40", same_as=("tap_chunks",))
