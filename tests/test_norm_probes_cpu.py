"""Per-hop probes of the feature normaliser in the single-thread emulator (tests/emu/nmx_emu.cpp): the scan kernels, the
column walk (naturally and with NMX_NORM_SCAN=0), the sorted-list family and the Yeo-Johnson fit against the float64
hop-by-hop oracle, at the histories, batch lengths, row counters and column counts where the code takes another path; and
the ties that hold the probes together: the restated scan / walk predicate against the launcher's source, the path of every
case, the constant of the tight gate against the oracle's own noise.  Cases and policy: tests/norm_probe_cases.py; no miss
is accepted; the figures observed are in profiles/norm_probes.md."""

import math
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import norm_probe_cases as cases  # noqa: E402

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")   # (the oracle's NumPy on all-NaN windows)


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


def host_pointers(dn, buf):
    dn.process_device(buf.ctypes.data, buf.shape[1], buf.shape[0], None)
    return buf


# ---- the ties -------------------------------------------------------------------------------------------------------------
def test_restated_predicate_is_the_launchers():
    rows, hist, cap, piece, pf, seg = cases.source_thresholds()
    assert (rows, hist, cap) == (cases.SCAN_MIN_ROWS, cases.SCAN_MIN_HIST, cases.SCAN_CAP_LIMIT)
    assert piece, "the piece length of nmx_norm_process is no longer min(n_rows, cap - 1)"
    assert (pf, seg) == (cases.NORM_PF, cases.NORM_SEG)
    assert cases.takes_scan("zscore", 65, 8) and not cases.takes_scan("zscore", 64, 8)
    assert not cases.takes_scan("mean", 65, 7) and not cases.takes_scan("mean", 65536, 8) and cases.takes_scan("mean", 65535, 8)
    assert not cases.takes_scan("median", 300, 64) and not cases.takes_scan("zscore", 300, 64, scan_on=False)
    assert [cases.piece_len(300, n) for n in (8, 299, 300, 601)] == [8, 299, 299, 299]


def test_every_scan_case_scans_and_every_walk_case_walks():
    for name in cases.SCAN_CASES:
        assert all(scan for _, _, scan in cases.case_paths(name)), name
    for name in cases.WALK_CASES:
        assert not any(scan for _, _, scan in cases.case_paths(name)), name
    # what the issue lists is there: histories, batch lengths (last pieces of 1 and 8 rows), row counters, widths
    sc = cases.SCAN_CASES
    assert {c[0] for c in sc.values()} >= {65, 66, 97, 300, 65535}
    assert {min(c[2], c[0] - 1) for c in sc.values()} >= {0, 1, 31, 32, 33, 298, 299}
    assert {c[2] for c in sc.values()} >= {2 ** 31 + 5, 2 ** 40 + 123}
    for N in (65, 66, 97, 300):
        got = set().union(*[set(c[3]) for c in sc.values() if c[0] == N])
        assert got >= {8, 31, 32, 33, N - 2, N - 1, N, N + 7, 2 * N + 1}, N
    assert {c[1] for c in sc.values()} >= {1, 63, 64, 65, 255, 256, 257}
    wk = cases.WALK_CASES
    assert {c[0] for c in wk.values()} >= {2, 3, 8, 9, 10, 64, 300, 65536}
    for N in (2, 3, 8, 9, 10, 64, 65536):
        assert set().union(*[set(c[3]) for c in wk.values() if c[0] == N]) >= {1, 7, 8, 9, 15, 16, 17}, N
    assert all(sc[n][0] == 300 for n in cases.SCAN_OFF_CASES) and len(cases.SCAN_OFF_CASES) >= 9


def test_every_default_layout_carries_every_column_kind():
    names = cases.layout(23, cases.KINDS)
    assert set(names) == set(cases.KINDS) | {"masked"} and names.count("masked") == 4
    for n in (64, 65, 257):
        m = cases.masked_columns(n)
        assert 0 in m and 63 in m and len(m) == 4
    assert cases.masked_columns(63)[0] == 0 and cases.masked_columns(63)[-1] == 62
    # the +-inf placements: one crosses a piece boundary inside a batch, the run enters in one batch and leaves in a later
    N, _, _, have, batches, _, stream, names, _ = cases.mz_inputs("n300_from_zero")
    j, k = names.index("pinf_ninf"), names.index("ninf_run")
    start = sum(batches[:7])                                           # the N + 7-row batch: pieces of 299 and 8 rows
    assert np.isposinf(stream[start + 298, j]) and np.isneginf(stream[start + 300, j])
    assert np.isneginf(stream[3:15, k]).all() and batches[0] == 8      # enters in the first two batches, leaves 299 hops on


# ---- mean / zscore --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SCAN_CASES))
def test_scan_geometry(emu_lib, monkeypatch, name):
    out = cases.mz_case(emu_lib, name, True, monkeypatch)
    print(name, out)


@pytest.mark.parametrize("name", list(cases.WALK_CASES))
def test_walk(emu_lib, monkeypatch, name):
    out = cases.mz_case(emu_lib, name, True, monkeypatch)
    print(name, out)


@pytest.mark.parametrize("name", cases.SCAN_OFF_CASES)
def test_walk_on_the_scan_inputs(emu_lib, monkeypatch, name):
    """NMX_NORM_SCAN=0: the walk on the inputs of the N = 300 scan cases, against the oracle on its own."""
    out = cases.mz_case(emu_lib, name, False, monkeypatch)
    print(name, out)


@pytest.mark.parametrize("first_scan", [True, False])
def test_state_crosses_between_scan_and_walk(emu_lib, monkeypatch, first_scan):
    cases.state_crossing_case(emu_lib, monkeypatch, first_scan)


@pytest.mark.parametrize("kind", ["scan", "walk", "power"])
def test_device_call_shape_with_guard_columns(emu_lib, monkeypatch, kind):
    cases.device_shape_case(emu_lib, monkeypatch, kind, host_pointers)


# ---- the order and scikit-learn family ------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", cases.ORDER_METHODS)
@pytest.mark.parametrize("name", list(cases.ORDER_CASES))
def test_order_family(emu_lib, name, method):
    print(name, method, cases.order_case(emu_lib, name, method))


@pytest.mark.parametrize("method,n_cols", cases.ORDER_WIDE)
def test_order_family_wide(emu_lib, method, n_cols):
    print(method, n_cols, cases.order_case(emu_lib, "o50", method, clips=(3,), n_cols=n_cols))


def test_quantile_interpolation_is_not_trivial_above_300_rows():
    """nq == 300 < n: the 300 quantiles fall between sorted values (the lerp's t != 0) at N = 301, 302, 450, 1000."""
    for N in (301, 302, 450, 1000):
        vi = (N - 1) * np.linspace(0, 1, 300)
        assert np.count_nonzero(np.abs(vi - np.round(vi)) > 1e-9) >= 290, N
    assert cases.ORDER_CASES["o301"][0] == 301 and min(cases.ORDER_CASES["o301"][2], 300) == 300


# ---- "power" --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.POWER_CASES))
def test_power(emu_lib, name):
    print(name, cases.power_case(emu_lib, name))


# ---- the constant of the tight gate (last: the oracle's rows are computed by then) ---------------------------------------
def test_tight_gate_constant_is_sixteen_times_the_oracles_own_noise():
    """K_TIGHT is 16 x the worst noise measured where the constant was set (15.5 units: the 65 536-row windows, whose NaN
    column sends the oracle through nanmean / nanstd), rounded up to a power of two.  The noise is re-measured here; the
    rule applied to it must give K_TIGHT again, or -- on a NumPy that sums in another order -- its neighbour."""
    worst = cases.oracle_noise(list(cases.SCAN_CASES) + list(cases.WALK_CASES))
    rule = 2.0 ** math.ceil(math.log2(16 * worst))
    print(f"oracle float64 noise, worst over the tight columns: {worst:.3f} units; the rule gives {rule:g}, K = {cases.K_TIGHT:g}")
    assert cases.K_TIGHT / 2 <= rule <= cases.K_TIGHT * 2, (worst, rule)
