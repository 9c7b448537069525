"""Per-entry probes of the band-pass power epilogues and the Kalman scan on the MI355X (libnmx.so): the five register forms
of the tail variance with their branch-free masks and the one-pass sum with its redo -- which the emulator does not run --,
nmx_hjorth behind nmx_kern_bank in both forms and the MC path of the one-wave kernel, nmx_kern_kalman; every bank kernel
asserted by name.  Cases, references and limits: tests/bandpower_probe_cases.py; no verifier, nothing forgiven, no case
skipped; the figures observed are in profiles/bandpower_probes.md."""

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import bandpower_probe_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
IDENTITY = cases.on_tier(None, cases.IDENTITY)
DESIGNED = cases.on_tier(None, cases.DESIGNED)


@pytest.fixture(scope="module", autouse=True)
def gpu_lib():
    from py_neuromodulation_amd import _lib

    lib = _lib.get_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    assert "libnmx.so" in str(lib.path)
    cases.SEEN_KERNELS.clear()
    return lib


@pytest.mark.parametrize("kind", IDENTITY)
def test_a_where_the_tail_starts(kind):
    assert cases.class_a(None, kind) > 0
    assert cases.EMU_LEFT_OUT == {}


@pytest.mark.parametrize("kind", IDENTITY)
def test_b_cancellation_and_the_redo(kind):
    assert cases.class_b_identity(None, kind) > 0
    for log in (0, 1):
        past, n = cases.REDO_ROWS[(kind, f"b log={log}")]
        assert 0 < past < n


@pytest.mark.parametrize("kind", DESIGNED)
def test_b_designed_taps_reach_the_redo(kind):
    assert cases.class_b_designed(None, kind) > 0


def test_b_carried_offset_on_the_pair_kernel():
    assert cases.class_b_carried(None) > 0


@pytest.mark.parametrize("kind", DESIGNED)
def test_c_end_to_end_on_noise(kind):
    assert cases.class_c(None, kind) > 0
    print(f"BPPROBE {kind}: seed {cases.C_SEEDS[kind][0]}, conditioning {cases.C_SEEDS[kind][1]:.2e}")


@pytest.mark.parametrize("feats", cases.D_SUBSETS, ids="+".join)
@pytest.mark.parametrize("kind", cases.on_tier(None, cases.D_KINDS))
def test_d_mobility_and_complexity(kind, feats):
    assert cases.class_d(None, kind, feats) > 0


@pytest.mark.parametrize("kind", cases.on_tier(None, cases.E_KINDS))
def test_e_amplitudes_and_rails(kind):
    assert cases.class_e_amplitudes(None, kind) > 0


@pytest.mark.parametrize("kind", cases.on_tier(None, cases.E_KINDS))
def test_e_nan_samples_leave_the_neighbours_alone(kind):
    assert cases.class_e_bad_samples(None, kind, "nan") > 0


@pytest.mark.parametrize("kind", cases.on_tier(None, cases.E_KINDS))
def test_e_infinite_samples_leave_the_neighbours_alone(kind):
    """The case that found the split-pair bug (profiles/bandpower_probes.md, finding 1): before the pair kernels ran a pair
    whose scales lie more than 2^60 apart as two solo passes, the partner of a channel with an infinite sample came out as
    0.0 (nmx_kern_bank_w64c_rd64) or 23.34 (nmx_kern_bank_w64d_rd64<0>) where 3.8785 is right."""
    assert cases.class_e_bad_samples(None, kind, "inf") > 0


@pytest.mark.parametrize("name", list(cases.KALMAN_CASES))
def test_f_kalman(name):
    assert cases.class_f(None, name) > 0


def test_f_kalman_state_carry():
    assert cases.class_f_carry(None) > 0


def test_f_kalman_dead_channel():
    assert cases.class_f_dead(None) > 0


def test_every_kernel_of_the_table_was_seen():
    """The names asserted by the cases that ran (this module, run as a whole) are the table's, no more and no less."""
    kinds = set(IDENTITY) | set(DESIGNED)
    assert set(cases.SEEN_KERNELS) == kinds, sorted(kinds - set(cases.SEEN_KERNELS))
    assert set(cases.SEEN_KERNELS.values()) == cases.KERNELS
    assert {cases.KINDS[k][5] for k in kinds} == cases.KERNELS
    unresolved = {k: v for k, v in cases.UNRESOLVED.items() if v}
    print(f"BPPROBE entries below float32's resolution (judged as such): {unresolved}")
    print(f"BPPROBE entries past the redo condition: {cases.REDO_ROWS}")
    print(f"BPPROBE class c, worst relative error (own series, float64 convolution): {cases.C_ERRORS}")
