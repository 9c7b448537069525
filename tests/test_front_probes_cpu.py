"""Per-sample probes of the front end and the resampler in the single-thread emulator (tests/emu/nmx_emu.cpp): the `_sample`
forms of the re-reference kernels, the shift, the NaN mask, the learned constants and the resample item in one-transform and
polyphase form; and the ties that hold the probes' references together: the restatements against the oracle and against the
matrices they decompose at 1e-12, the restated plan arithmetic against what the plans report, the case tables against the
launch conditions in the sources.  Cases and policy: tests/front_probe_cases.py; figures: profiles/front_probes.md."""

import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import front_probe_cases as cases  # noqa: E402

CSRC = ROOT / "py_neuromodulation_amd" / "csrc"


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


# ---- ties ---------------------------------------------------------------------------------------------------------------
def test_resampler_restatement_is_the_oracles_on_every_case():
    """resample64 (pad, rfft, bins, irfft) and the yardstick's chain run in float64 (packed transforms at the plan's lengths,
    polyphase sums) against oracle.mne_restated.resample at 1e-12 max|y|, on every case's inputs; the yardstick itself
    within YARD_CAP eps32 of it."""
    from oracle import mne_restated

    for name, (sf_old, sf_new, Wr, *_rest) in cases.RESAMPLE_CASES.items():
        p = cases.case_plan(name)
        for cls, x in cases.resample_inputs(name, p):
            xc = np.nan_to_num(x).astype(np.float64)
            want = mne_restated.resample(xc, up=sf_new / sf_old, down=1.0)
            got = cases.resample64(xc, p)
            assert got.shape == want.shape == (cases.RESAMPLE_C, p["W_new"]), (name, got.shape, want.shape)
            assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (name, cls, np.abs(got - want).max())
            chain = cases.resample_chain(xc, p, np.float64)   # the yardstick's code in float64: the same values
            assert np.abs(chain - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (name, cls, np.abs(chain - want).max())
            cases.check_resampled(name, cls + " (yardstick)", cases.resample32(xc, p), got, cases.resample32(xc, p), xc, p)
        cases.REPORT.flush(name)


def test_the_yardstick_is_an_fp32_resampler():
    """On noise the yardstick's error is of the order of eps32 rms(x): not float64 by accident, not broken -- in the
    one-transform, the forced and the long polyphase form."""
    for name in ("down_even", "down_odd", "up_odd", "poly_forced_4k", "poly_8k", "poly_24k"):
        p = cases.case_plan(name)
        x = cases.fir._f32(np.random.default_rng(3).standard_normal((4, p["W"])) * 50)
        e32 = np.abs(cases.resample32(x, p) - cases.resample64(x, p)).max(axis=-1) / (cases.EPS32 * cases.fir.rms(x))
        assert np.all((e32 > 0.1) & (e32 < cases.YARD_CAP)), (name, e32)


def test_structure_restatement_rebuilds_its_matrix():
    """struct_decompose (find_reref_structure restated): put together again == R at 1e-12; the group counts and sizes the
    case table names; the fp32 coefficients within eps32 of the exact ones."""
    want_groups = {"struct_sub40": [40], "struct_g1": [33], "struct_g2": [5, 6, 8], "struct_g3": [16, 17, 21],
                   "struct_g4": [5, 6, 16, 33], "struct_taps": []}
    for name, sizes in want_groups.items():
        R = cases.struct_matrix(name)
        rows = cases.struct_decompose(R)
        assert rows is not None, name
        assert np.abs(cases.struct_rebuilt(R) - R).max() <= 1e-12, name
        groups = sorted({g for _, g, _ in rows if g is not None}, key=lambda g: (len(g), g))
        assert sorted(len(g) for g in groups) == sorted(sizes), (name, [len(g) for g in groups])
        assert all(len(t) <= 4 for t, _, _ in rows)
        Ra, O = cases.uploaded(R, cases.STRUCT)
        assert np.all(np.abs(Ra - R) <= cases.EPS32 * (np.abs(R) + O)), name
    assert cases.struct_decompose(cases.struct_matrix("struct_g5")) is None          # a fifth group
    assert cases.struct_decompose(np.random.default_rng(1).standard_normal((3, 9))) is None   # no repeated value
    rows = cases.struct_decompose(cases.struct_matrix("struct_g2"))
    assert sum(len(t) == 3 and g is not None and len(g) == 8 for t, g, _ in rows) == 1, "the row of a group plus extra taps"
    assert sorted(len(t) for t, g, _ in cases.struct_decompose(cases.struct_matrix("struct_g1")) if g is None) == [1, 2, 3]
    assert cases.struct_matrix("struct_sub40").shape == (5, 40)
    assert {cases.struct_matrix(n).shape[0] for n in want_groups} >= {5, 7, 9}
    for C in (2, 17, 257):
        Ra, O = cases.uploaded(cases.car_matrix(C), cases.CAR)
        assert np.all(np.abs(Ra - cases.car_matrix(C)) <= cases.EPS32 * (np.abs(cases.car_matrix(C)) + O))


def test_case_tables_against_the_launch_conditions_in_the_sources():
    """be_launch_car's NW rule, build_front's order of kernels, build_resample's plan choice and the NaN mask's launcher, read
    from the sources; the case tables reach both sides of every condition."""
    api = (CSRC / "nmx_api.hip").read_text()
    m = re.search(r'if \(A\.T <= (\d+) && A\.C >= (\d+)\) NMX_LAUNCH_AS\("nmx_kern_car", nmx_kern_car<(\d+)>.*\n\s*else NMX_LAUNCH_AS\("nmx_kern_car", nmx_kern_car<(\d+)>', api)
    assert m and [int(g) for g in m.groups()] == [4096, 64, 16, 4], "be_launch_car's condition changed: the case table follows it"
    T = cases.W + (cases.HOPS - 1) * cases.HOP
    T_long, T_short = cases.W + (cases.LONG_HOPS - 1) * cases.HOP, cases.W + (cases.SHORT_HOPS - 1) * cases.HOP
    assert T_long > 4096 >= T_short and all(t % 64 and t % 256 for t in (T, T_long, T_short, cases.W))
    assert all(cases.car_waves(cases.REREF_CASES[n][0]().shape[0], T) == 4 for n in cases.CAR_NW4)
    assert all(cases.car_waves(cases.REREF_CASES[n][0]().shape[0], t) == 16 for n in cases.CAR_NW16 for t in (T, cases.W))
    assert all(cases.car_waves(cases.REREF_CASES[n][0]().shape[0], T_long) == 4 for n in cases.CAR_LONG)
    # NW = 4: j = q; loop while j + 12 < C; tails j < C, j + 4 < C, j + 8 < C -- per wave q the number of tail terms 0 .. 3
    def walk(C, q, stride, ahead):
        j, trips = q, 0
        while j + ahead < C:
            j, trips = j + stride, trips + 1
        return trips, j

    tails = set()
    for name in cases.CAR_NW4:
        C = cases.REREF_CASES[name][0]().shape[0]
        for q in range(4):
            trips, j = walk(C, q, 16, 12)
            tails.add((tuple(j + d < C for d in (0, 4, 8)), trips))
    assert {t for t, _ in tails} == {(False, False, False), (True, False, False), (True, True, False), (True, True, True)}
    assert {n for _, n in tails} == {0, 1, 2, 3, 4}
    nw16 = set()   # NW = 16: wave q owns class q: trips of the 64-stride loop, then terms of the 16-stride tail
    for name in cases.CAR_NW16:
        C = cases.REREF_CASES[name][0]().shape[0]
        for q in range(16):
            trips, j = walk(C, q, 64, 48)
            nw16.add((trips, len(range(j, C, 16))))
    assert {t for t, _ in nw16} == {1, 2, 4} and {n for _, n in nw16} == {0, 1, 2, 3}, sorted(nw16)
    # (the launch helper of nmx_common.h: NMX_LAUNCH reports the kernel's spelling, NMX_LAUNCH_AS the name it is given, NMX_LAUNCH_QUIET nothing)
    for name in ("nmx_kern_reref_struct", "nmx_kern_reref", "nmx_kern_shift", "nmx_kern_resample"):
        assert f"NMX_LAUNCH({name}," in api, name
    launcher = re.search(r"static void be_launch_nanmask\([^)]*\) \{\n(.*?)\n\}", api, re.S).group(1)
    assert launcher.lstrip().startswith("NMX_LAUNCH_QUIET(nmx_kern_nanmask,") and launcher.count("NMX_LAUNCH") == 1
    assert len(re.findall(r"NMX_LAUNCH\w*\([^;]*nmx_kern_nanmask\b", api)) == 1
    prep = (CSRC / "nmx_k_prep.h").read_text()
    assert "#define NMX_REREF_ROWS 16" in prep and "#define NMX_RS_TAPS 4" in prep and "#define NMX_RS_GROUPS 4" in prep
    assert "m + 12 < end" in prep and "j + 12 < A.C" in prep and "j + 48 < A.C" in prep
    state = (CSRC / "nmx_engine_plan_state.inc").read_text()
    assert 'if (Cin == C && C >= 2 && env_int("NMX_CAR_FAST", 1))' in state
    assert 'if (!F.car && env_int("NMX_REREF_STRUCT", 1)) return find_reref_structure(P);' in state
    assert 'if (n_pad <= 8192 && layout(n_pad / 2, 1) && !env_int("NMX_RESAMPLE_POLY", 0))' in state
    assert "const int m = std::min(2048, n_pad / 2);" in state and "const int min_add = std::min(W / 8, 100) * 2;" in state
    assert "return A.lds_floats * 4 <= 160 * 1024;" in state and "A.inv_full = n_new & 1;" in state
    dc = (CSRC / "nmx_engine_dc.inc").read_text()
    assert "const double ratio = 4.0;" in dc and "if (std::isfinite(v)) { sum += v; ++n; }" in dc
    # the tables: every kernel, every form
    kernels = {c[2] for c in cases.REREF_CASES.values()}
    assert kernels == {cases.CAR, cases.STRUCT, cases.DENSE}
    for name, (make, env, kernel, _) in cases.REREF_CASES.items():
        assert cases.front_kernel(make(), env) == kernel, name
    assert cases.front_kernel(cases._dense(5, 3), {}) == cases.STRUCT   # (why the C_in = 3 dense cases switch the search off)
    forms = {(bool(p["poly_q"]), bool(p["inv_full"])) for p in map(cases.case_plan, cases.RESAMPLE_CASES)}
    assert forms == {(False, False), (False, True), (True, False), (True, True)}
    assert {cases.case_plan(n)["poly_q"] for n in cases.RESAMPLE_CASES} == {0, 2, 4, 8, 16, 32}
    assert {c for c in {cases.REREF_CASES[n][0]().shape for n in cases.DENSE_CASES}} >= {(c, ci) for c in (1, 15, 16, 17, 33) for ci in (3, 300)}


def test_restated_plan_arithmetic_against_what_the_plans_report():
    """Window lengths of a dry plan of every resampler case (the library checks window == round(ratio x raw_window) itself
    when the plan is built: resample_case); inputs: the positions asked for, distinct impulses, the NaN placements."""
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    for name, (sf_old, sf_new, Wr, *_rest) in cases.RESAMPLE_CASES.items():
        p = cases.case_plan(name)
        eng = HotPathEngine(NMSettings.get_default(), ["a", "b"], sf_new, features=["return_raw"], resample_from=sf_old, raw_window=Wr,
                            dry_run=True)
        assert (eng.W_in, eng.W, eng.resample_ratio) == (Wr, p["W_new"], p["ratio"]), name
        pos = set(cases.resample_positions(p, every=name == "poly_forced_40"))
        edge = {0, 1, 2, Wr // 2, Wr - 2, Wr - 1, p["pad_l"], Wr - 1 - p["pad_r"]}
        assert {t for t in edge if 0 <= t < Wr} <= pos, (name, sorted(edge - pos))
        if p["poly_q"]:
            assert set(range(min(2 * p["poly_q"] + 2, Wr))) <= pos
    assert len(cases.resample_positions(cases.case_plan("poly_forced_40"), every=True)) == 40
    for Cin, T in ((5, 1300), (129, 4600), (300, 1300), (257, 200)):
        x = cases.recording(Cin, T, "impulse", 1)
        where = np.nanargmax(x, axis=1)
        assert len(set(where)) == min(Cin, T) or Cin > T, (Cin, T)
        nan_t = {t for _, t in cases.nan_places(Cin, T)}
        assert {t for t in cases.NAN_T if t < T} | {T - 1} <= nan_t and (T == 200 or {300, 499} <= nan_t)
        assert np.isnan(cases.recording(Cin, T, "noise", 1)).sum() == len(nan_t)
    sc = cases.row_scales(9)
    assert set(sc) == {1.0, 1e4, 1e-3, 0.0}
    x = cases.recording(9, 1300, "noise", 2, offsets=True).astype(np.float64)
    lvl = np.abs(np.nanmean(x, axis=1)) / np.where(sc > 0, sc, 1.0) / cases.SIGMA
    assert np.all(np.abs(lvl / cases.OFFSET - 1) < 1e-3), lvl


# ---- 1. re-reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CAR_NW4 + cases.CAR_NW16 + cases.CAR_LONG)
def test_common_average(emu_lib, name):
    out = cases.reref_case(emu_lib, name)
    assert set(out) - {"short"} == {"noise", "offsets", "impulse", "nosplit"} and ("short" in out) == (name in cases.CAR_LONG)
    assert set(out["nosplit"]) == {"b"} and set(out["offsets"]) == {"a", "b"}


@pytest.mark.parametrize("name", cases.STRUCT_CASES)
def test_structured_matrices(emu_lib, name):
    out = cases.reref_case(emu_lib, name)
    assert set(out) == {"noise", "offsets", "impulse", "nosplit"}


@pytest.mark.parametrize("name", cases.DENSE_CASES)
def test_dense_product(emu_lib, name):
    out = cases.reref_case(emu_lib, name)
    assert set(out) == {"noise", "offsets", "impulse", "nosplit"}


@pytest.mark.parametrize("C", [65, 129])
def test_average_of_a_window_and_of_its_stream_same_bytes(emu_lib, C):
    cases.car_bytes_case(emu_lib, C)


@pytest.mark.parametrize("name", ["car_c13", "struct_g2"])
def test_three_chunks_store_the_bytes_of_one(emu_lib, name):
    cases.chunks_case(emu_lib, name)


def test_shift_in_front_of_the_notch(emu_lib):
    assert set(cases.shift_case(emu_lib)) == {"tap", "window"}


# ---- 2. learned constants, NaN mask ---------------------------------------------------------------------------------------
def test_learned_constants_are_the_rule_restated(emu_lib):
    cases.learned_case(emu_lib)


def test_nan_mask(emu_lib):
    cases.nanmask_case(emu_lib)


# ---- 3. resampler ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.EMU_RESAMPLE)
def test_resampler_through_preprocess_window(emu_lib, name):
    worst = cases.resample_case(emu_lib, name)
    assert {"impulse", "noise"} <= set(worst)


@pytest.mark.parametrize("with_notch", [False, True])
def test_resampler_in_a_batch_through_the_tap(emu_lib, with_notch):
    cases.batch_resample_case(emu_lib, with_notch)
