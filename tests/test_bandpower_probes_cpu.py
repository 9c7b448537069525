"""Per-entry probes of the band-pass power epilogues and the Kalman scan in the single-thread emulator
(tests/emu/nmx_emu.cpp): every case of tests/bandpower_probe_cases.py whose plan the emulator builds -- nmx_kern_bank in
LDS and partitioned form (1 kHz and the 8000-sample window), the one-wave item of the default shape (`one_emu`: its
register form is the skip / straddle one, not the device's branch-free masks) and the Kalman scan throughout -- under the
same references and limits as the MI355X tier: it proves the cases, the references and the expectations before any GPU
time is spent.  The channel-pair kernels, the M = 1024 / 4096 kernels and the persistent pipelined kernel are device only.
And the ties that hold the probes together: the tables against the kernels' source text, the emulator's single accumulator,
the redo condition's sides, the Kalman limit.  The figures observed are in profiles/bandpower_probes.md."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import bandpower_probe_cases as cases  # noqa: E402

CSRC = ROOT / "py_neuromodulation_amd" / "csrc"


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


EMU_IDENTITY = [k for k in cases.IDENTITY if cases.KINDS[k][7]]
EMU_DESIGNED = [k for k in cases.DESIGNED if cases.KINDS[k][7]]
EMU_D = [k for k in cases.D_KINDS if cases.KINDS[k][7]]
EMU_E = [k for k in cases.E_KINDS if cases.KINDS[k][7]]


@pytest.mark.parametrize("kind", EMU_IDENTITY)
def test_a_where_the_tail_starts(emu_lib, kind):
    cases.EMU_LEFT_OUT.pop(kind, None)
    n = cases.class_a(emu_lib, kind)
    left = cases.EMU_LEFT_OUT.get(kind, 0)
    print(f"BPPROBE {kind}: {left} impulse entries left to the device tier (one accumulator), {n} judged")
    assert n > 0 and left < n // 4
    if kind == "one_emu":
        assert left == 0


@pytest.mark.parametrize("kind", EMU_IDENTITY)
def test_b_cancellation_and_the_redo(emu_lib, kind):
    assert cases.class_b_identity(emu_lib, kind) > 0
    for log in (0, 1):
        past, n = cases.REDO_ROWS[(kind, f"b log={log}")]
        assert 0 < past < n


@pytest.mark.parametrize("kind", EMU_DESIGNED)
def test_b_designed_taps(emu_lib, kind):
    assert cases.class_b_designed(emu_lib, kind) > 0


@pytest.mark.parametrize("kind", EMU_DESIGNED)
def test_c_end_to_end_on_noise(emu_lib, kind):
    assert cases.class_c(emu_lib, kind) > 0
    print(f"BPPROBE {kind}: seed {cases.C_SEEDS[kind][0]}, conditioning {cases.C_SEEDS[kind][1]:.2e}")


@pytest.mark.parametrize("feats", cases.D_SUBSETS, ids="+".join)
@pytest.mark.parametrize("kind", EMU_D)
def test_d_mobility_and_complexity(emu_lib, kind, feats):
    assert cases.class_d(emu_lib, kind, feats) > 0


@pytest.mark.parametrize("kind", EMU_E)
def test_e_amplitudes_and_rails(emu_lib, kind):
    assert cases.class_e_amplitudes(emu_lib, kind) > 0


@pytest.mark.parametrize("kind", EMU_E)
def test_e_nan_samples_leave_the_neighbours_alone(emu_lib, kind):
    assert cases.class_e_bad_samples(emu_lib, kind, "nan") > 0


@pytest.mark.parametrize("kind", EMU_E)
def test_e_infinite_samples_leave_the_neighbours_alone(emu_lib, kind):
    """(The kinds of this tier hold one channel per transform.)"""
    assert cases.class_e_bad_samples(emu_lib, kind, "inf") > 0


@pytest.mark.parametrize("name", list(cases.KALMAN_CASES))
def test_f_kalman(emu_lib, name):
    assert cases.class_f(emu_lib, name) > 0
    assert cases.KALMAN_WORST[name][0] <= 1.0


def test_f_kalman_state_carry(emu_lib):
    assert cases.class_f_carry(emu_lib) > 0


def test_f_kalman_dead_channel(emu_lib):
    assert cases.class_f_dead(emu_lib) > 0


# ---- ties --------------------------------------------------------------------------------------------------------------------
def test_the_tables_name_every_kernel():
    """Every bank kernel is the expectation of a kind of class a or b; the emulator tier's kinds are the LDS forms and the
    one-wave item; the thread counts of the Kalman cases straddle the 64-thread block."""
    gpu_ab = {cases.KINDS[k][5] for k in cases.on_tier(None, cases.IDENTITY + cases.DESIGNED)}
    assert gpu_ab == cases.KERNELS
    assert {cases.KINDS[k][5] for k in cases.on_tier(None, cases.IDENTITY)} == cases.KERNELS - {cases.X21, cases.D1}   # (module docstring)
    assert {cases.KINDS[k][5] for k in EMU_IDENTITY + EMU_DESIGNED} == {cases.LDS, ""}
    assert {c["C"] * c["B"] for c in cases.KALMAN_CASES.values()} >= {63, 64, 65, 129}
    assert len(cases.D_SUBSETS) == 7
    for kind in cases.IDENTITY:
        W = cases.KINDS[kind][2]
        lens = cases.tail_lengths(kind)
        assert {W, W - 1, 2, 1} <= set(lens)
        for b in cases.KINDS[kind][6]:
            assert {W - b - 1, W - b, W - b + 1} & set(range(1, W + 1)) <= set(lens), (kind, b)


def test_the_register_forms_are_the_sources():
    """The five register forms hold the branch-free mask and the redo condition the cases are built around; nmx_hjorth's
    callers pass the tail's start and mode 1; build_kalman computes Q as the oracle does."""
    for f in ("nmx_k_bank_w64.h", "nmx_k_bank_w64c.h", "nmx_k_bank_w64d.h", "nmx_k_bank_w64x2.h", "nmx_k_bank_w64p.h"):
        src = (CSRC / f).read_text()
        assert "< span" in src and "> 4.f * t" in src, f
    for f in ("nmx_k_bank_w64.h", "nmx_k_bank.h"):
        assert "nmx_hjorth(y + (W - F.bp_seglen), F.bp_seglen, red, 1," in (CSRC / f).read_text(), f
    state = (CSRC / "nmx_engine_plan_state.inc").read_text()   # (kalman_state_reset: the P0 every plan starts from)
    assert "st[i] = 0.0; st[i + 1] = 1.0; st[i + 2] = 0.5; st[i + 3] = -0.5; st[i + 4] = -0.5; st[i + 5] = 0.5;" in state
    assert "K.q00 = sw2 * T * T * T / 3.0; K.q01 = sw2 * T * T / 2.0; K.q11 = sw2 * T;" in state


def test_tail_lengths_in_whole_milliseconds():
    for sfreq in (500.0, 600.0, 750.0, 1000.0):
        for n in (1, 2, 3, 63, 64, 65, 333, 499):
            assert int(np.floor(sfreq / 1000 * cases.ms_for(n, sfreq))) == n
    with pytest.raises(AssertionError):
        cases.ms_for(1, 2500.0)


def test_the_emulators_single_accumulator():
    """The impulse entries the emulator tier leaves to the device: an early impulse in a long tail.  One accumulator adds
    (a / n)^2 to (a - a / n)^2 a thousand times, every time rounded the same way, and misses the policy; 64 accumulators
    (the device kernels' order) meet it a decade under."""
    t = np.zeros(1000, np.float32)
    t[1] = 3.0
    want = float(np.var(t.astype(np.float64)))
    one, lanes = cases.var32_lanes(t, 1), cases.var32_lanes(t, 64)
    print(f"BPPROBE an impulse at sample 1 of 1000: relative error {abs(one - want) / want:.1e} with one accumulator, {abs(lanes - want) / want:.1e} with 64")
    assert abs(one - want) > 1e-5 * want and abs(lanes - want) < 1e-6 * want
    t = np.zeros(1000, np.float32)
    t[998] = 3.0   # (a late impulse: the large term comes last)
    assert abs(cases.var32_lanes(t, 1) - want) < 1e-6 * want


def test_redo_ratio_sides():
    """n mean^2 / (4 SS) of noise on an offset of d sigma is about d^2 / 4: 1.5 and 3 fall on either side with room."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((64, 333)) * 50
    lo, hi = cases.redo_ratio(x + 75.0), cases.redo_ratio(x + 150.0)
    print(f"BPPROBE redo ratio of a 333-sample tail: d = 1.5: {lo.min():.2f} .. {lo.max():.2f}, d = 3: {hi.min():.2f} .. {hi.max():.2f}")
    assert lo.max() <= 0.8 and hi.min() >= 1.25
    assert cases.redo_ratio(np.zeros((1, 5)))[0] == 0 and cases.redo_ratio(np.full((1, 5), 2.0))[0] == np.inf
    d = cases.offsets_b(cases.B_CHANNELS)
    pairs = [(d[i], d[i + 1]) for i in range(0, len(d) - 1, 2)]
    assert (3.0, 1.5) in pairs and (1.5, 3.0) in pairs and (3.0, 3.0) in pairs and len(d) % 2 == 1 and d[-1] == 3.0
    assert any(np.isnan(a) and b == 3.0 for a, b in pairs) and any(a == 3.0 and np.isnan(b) for a, b in pairs)


def test_kalman_limit_is_the_store():
    """The limit is one float32 spacing plus 1e-12 max(1, max|z|): a hundredth of what rtol 1e-5 allowed at order 1."""
    want, z = np.array([1.5, -3.25, 1000.0]), np.array([2.0, 1000.0])
    lim = cases.kalman_limit(want, z)
    assert np.allclose(lim, [2.0 ** -23 + 1e-9, 2.0 ** -22 + 1e-9, 2.0 ** -14 + 1e-9], rtol=1e-9)
    assert np.all(lim < 0.012 * (1e-5 * np.abs(want) + 2e-6))
    # ... and the oracle on a dead channel: -inf once, NaN (0 after nan_to_num) for ever
    w = cases.kalman_want(np.array([1.0, -np.inf, 1.0, 2.0]), cases.K_DEFAULT)
    assert w[1] < -1e300 and not w[2:].any()
