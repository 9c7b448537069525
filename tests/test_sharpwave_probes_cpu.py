"""Per-trough probes of the sharp-wave detector in the single-thread emulator (tests/emu/nmx_emu.cpp): every case of
tests/sharpwave_probe_cases.py on the kind the emulator reaches (LIST with the host extrema walk, the value-list
estimators), which validates the inputs (margin and sensitivity conditions on every row), the oracle glue and the limits
before any GPU time is spent; and the ties that hold the probes together: the glue against oracle.SharpwaveAnalyzer, the
restated plan choices against the source text, the coverage of every branch class the case table names.  The figures
observed are in profiles/sharpwave_probes.md."""

import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import sharpwave_probe_cases as cases  # noqa: E402

CSRC = ROOT / "py_neuromodulation_amd" / "csrc"


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_on_the_emulator(emu_lib, name):
    rep = cases.run_case(emu_lib, name)
    c = cases.CASES[name]
    assert rep.n == c["C"] * c["hops"] * len(c["taps"])


def test_noise_layer_on_the_emulator(emu_lib):
    """One seed, 16 channels (the emulator filters 1651 taps in one thread)."""
    cases.run_noise(emu_lib, seeds=(1,), C=16)


def test_glue_is_the_oracles_analyzer():
    """reference_row against oracle.nm_oracle.SharpwaveAnalyzer.calc_feature handed the series instead of filtering it:
    the same keys, the same values (the glue restates the estimator table and the between-polarity step)."""
    from oracle import nm_oracle as orc

    for name in ("est_vals", "nobetween", "troughs_only", "x450", "sharp_250"):
        c = cases.CASES[name]
        X = cases.case_rows(name)[0]
        ch = [f"ch{i}" for i in range(c["C"])]
        an = orc.SharpwaveAnalyzer(cases.case_settings(c), ch, c["sfreq"], taps=[np.array([1.0])])
        an.filtered = lambda data: np.asarray(data)[:, None, :]
        want = an.calc_feature(X)
        got = {}
        for ci in range(c["C"]):
            got.update({k: v for k, (v, _) in cases.reference_row(X[ci], c, ch[ci], "range_5_80").items()})
        assert set(got) == set(want), name
        for k in want:
            assert got[k] == pytest.approx(float(want[k]), rel=1e-13, abs=1e-300), (name, k)


def test_limits_hold_for_a_float32_restatement():
    """The limits against arithmetic done the plain way in float32 (sequential sums): a limit that a correct single
    precision evaluation misses would be a wrong derivation.  Series: the estimator rows."""
    from oracle import nm_oracle as orc

    c = cases.CASES["est_vals"]
    f32 = np.float32
    for y in cases.case_rows("est_vals")[0]:
        Y = float(np.abs(y).max())
        r = orc.analyze_waveform(y, c["sfreq"], *c["dist"], {f for f, _ in c["combos"]})
        for f in ("interval", "prominence", "width", "sharpness"):
            v = np.asarray(r[f], np.float64)
            if v.size == 0:
                continue
            v32 = v.astype(f32)
            acc = f32(0)
            for t in v32:
                acc = f32(acc + t)
            m32 = f32(acc / f32(v.size))
            want, lim = cases.estimate("mean", v, cases.value_err(f, v, Y))
            assert abs(float(m32) - want) <= lim, (f, float(m32), want, lim)
            acc = f32(0)
            for t in v32:
                acc = f32(acc + f32((t - m32) * (t - m32)))
            var32 = f32(acc / f32(v.size))
            want, lim = cases.estimate("var", v, cases.value_err(f, v, Y))
            assert abs(float(var32) - want) <= lim, (f, float(var32), want, lim)


def test_restated_plan_choices_are_the_sources():
    """plan_choice against the text of build_sharp and nmx_extrema, the kernels per kind against be_launch_sharp and the
    launchers' names."""
    plan = (CSRC / "nmx_engine_plan_state.inc").read_text()
    for line in ('A.sharp_off = (int)(5.0 * (1000.0 / d.sfreq));',
                 'A.dense_ok = env_int("NMX_SW_DENSE", 1) && A.fast_estimators && A.dist_peaks <= 10 && A.dist_troughs <= 10;',
                 'if (!(e == NMX_SWE_MEAN || e == NMX_SWE_MAX || e == NMX_SWE_MIN)) A.fast_estimators = 0;',
                 'if (f == NMX_SW_RISE_STEEPNESS || f == NMX_SW_DECAY_STEEPNESS || f == NMX_SW_SLOPE_RATIO) A.fast_estimators = 0;',
                 'const int pm = d.window / 2 + 2;', 'const int lw = al4((pm + 1) / 2);', 'A.off_emax = al4(d.window);',
                 'A.off_selp = A.off_rt + lw;', 'const int tail = std::max(lw + al4((2 * pm + 3) / 4), al4(pm));',
                 'A.off_res = A.off_selp + tail;', 'A.off_red = A.off_res + al4(2 * d.sw_n_combos + 2);',
                 'A.lds_floats = A.off_red + 64;', 'if ((size_t)A.lds_floats * 4 > 160 * 1024) {',
                 'P.sharp.kind = A.slab_mode ? (dense ? NMX_SHARP_DENSE_SLAB : NMX_SHARP_SLAB) : (dense ? NMX_SHARP_DENSE_LIST : NMX_SHARP_LIST);'):
        assert line in plan, line
    # (five lists between off_emax and off_selp)
    assert [m for m in re.findall(r"A\.off_(\w+) = A\.off_\w+ \+ lw;", plan)] == ["emin", "selt", "lf", "rt", "selp", "st"]
    kern = (CSRC / "nmx_k_sharpwave.h").read_text()
    for line in ('const int chunk = n_idx > 0 ? (n_idx + NMX_NT - 1) / NMX_NT : 0;', 'if ((chunk == 16 || chunk == 8) && NMX_NT == 64) {',
                 'if (chunk > 64) {', 'const bool dense = A.dense_ok && n_max <= 128 && n_min <= 128;',
                 'const bool one = n_max <= 64 && n_min <= 64;', 'if (nT <= 128 && n_pairs <= 128) {',
                 'if (nT <= 64 && n_pairs <= 64) nmx_sw_fast_est<1>', 'for (int base = 0; base < n_pairs; base += 1024) {',
                 'while (2 * step0 <= nPk) step0 *= 2;'):
        assert line in kern, line
    api = (CSRC / "nmx_api.hip").read_text()
    launch = {"LIST": "nmx_wave_launch_sharp(&A", "SLAB": "nmx_wave_launch_sharp_slab(&A", "DENSE_LIST": "", "DENSE_SLAB": ""}
    for kind, names in cases.KERNELS.items():
        row = re.search(rf"case NMX_SHARP_{kind}: (.*?) return;", api).group(1)
        called = set(re.findall(r"nmx_wave_launch_(sharp\w*)\(", row))
        assert {"nmx_kern_" + n for n in called} == names, (kind, row)
        assert launch[kind] in row
    noted = set(re.findall(r"NMX_LAUNCH\((nmx_kern_sharp\w*),", (CSRC / "nmx_wave.hip").read_text() +   # (reports the kernel's spelling)
                           (CSRC / "nmx_wave_slab.hip").read_text()))
    assert noted == set().union(*cases.KERNELS.values()), noted
    assert cases.plan_choice(1000, 1000.0, 5, 10, cases.DEFAULT_COMBOS) == \
        {"kind": "DENSE_LIST", "chunk": 16, "dense_ok": True, "fast_estimators": True, "sharp_off": 5}
    assert cases.plan_choice(14000, 14000.0, 5, 10, cases.DEFAULT_COMBOS)["kind"] == "DENSE_LIST"     # (test_sharpwave_long_gpu.py)
    assert cases.plan_choice(16000, 16000.0, 5, 10, cases.DEFAULT_COMBOS)["kind"] == "DENSE_SLAB"
    assert cases.plan_choice(250, 250.0, 5, 10, cases.ALL_VALS) == \
        {"kind": "LIST", "chunk": 4, "dense_ok": False, "fast_estimators": False, "sharp_off": 20}


def test_every_branch_class_of_the_table_is_reached():
    """From the reference's own counts on the constructed rows (the read-out takes the same decisions: check_inputs):
    every class the case table names is reached by at least one item of a case whose plan, on the MI355X, takes that
    branch."""
    seen = set()
    items = [(name, cases.case_choice(name), cases.analyze_row(x, cases.CASES[name]))
             for name in cases.CASES for x in cases.case_rows(name).reshape(-1, cases.CASES[name]["W"])]
    for name, ch, an in items:
        c = cases.CASES[name]
        n_max, n_min = an["Peak"]["_n_raw"]
        dense_kind = ch["kind"].startswith("DENSE")
        seen.add(("form", cases.chunk_form(ch["chunk"])))
        seen.add(("chunk", ch["chunk"]))
        if not dense_kind and n_max + n_min > 0:
            seen.add(("list form", cases.chunk_form(ch["chunk"])))
        seen.add(("kind", ch["kind"]))
        seen.add(("sharp_off", ch["sharp_off"]))
        if dense_kind:
            nsl = 1 if max(n_max, n_min) <= 64 else 2 if max(n_max, n_min) <= 128 else "overflow"
            seen.add(("nsl", nsl))
            seen.add(("raw", n_max, n_min))
            if nsl == "overflow":
                seen.add(("todo", ch["kind"]))
        for p in ("Peak", "Trough"):
            r = an[p]
            nT, n_pairs = r["_nT"], r["_n_pairs"]
            listed = not dense_kind or max(n_max, n_min) > 128
            if ch["fast_estimators"]:
                seen.add(("fast_est", 1 if max(nT, n_pairs) <= 64 else 2 if max(nT, n_pairs) <= 128 else "strided"))
            else:
                seen.add(("vals", "median" if any(e == "median" for _, e in c["combos"]) else "plain"))
            if listed and n_pairs > 1024:
                seen.add(("blocks", -(-n_pairs // 1024), "first_valid >= 50" if r["_first_valid"] >= 50 else ""))
            if listed and r["_nPk"] >= 2048:
                seen.add("step0 > 1024")
            if nT > 0 and n_pairs != nT:
                seen.add("nPT = 0")
            if nT == 1 and n_pairs == 0:
                seen.add("nT = 1, n_pairs = 0")
            if n_max + n_min == 0:
                seen.add("no extrema")
            if r["_first_valid"] > 1:
                seen.add(("first_valid > 1", "dense" if not listed else "list"))
            if r["_behind"] > 1:
                seen.add(("behind > 1", "dense" if not listed else "list"))
            if r["_nPk"] == 0 and nT == 0 and n_max + n_min > 0:
                seen.add("one kind only")
    want = [("form", "branchfree16"), ("form", "branchfree8"), ("form", "mask64"), ("form", "twopass"), ("list form", "branchfree16"),
            ("list form", "mask64"), ("list form", "twopass"), ("chunk", 1), ("chunk", 7),
            ("chunk", 15), ("chunk", 17), ("chunk", 64), ("chunk", 65), ("kind", "LIST"), ("kind", "DENSE_LIST"), ("kind", "SLAB"),
            ("kind", "DENSE_SLAB"), ("sharp_off", 0), ("sharp_off", 5), ("sharp_off", 20), ("nsl", 1), ("nsl", 2), ("nsl", "overflow"),
            ("raw", 64, 64), ("raw", 64, 65), ("raw", 65, 64), ("raw", 65, 65), ("raw", 128, 128), ("raw", 128, 129), ("raw", 129, 128),
            ("todo", "DENSE_LIST"), ("todo", "DENSE_SLAB"), ("fast_est", 1), ("fast_est", 2), ("fast_est", "strided"),
            ("vals", "median"), ("blocks", 4, ""), ("blocks", 4, "first_valid >= 50"), "step0 > 1024", "nPT = 0",
            "nT = 1, n_pairs = 0", "no extrema", ("first_valid > 1", "dense"), ("first_valid > 1", "list"), ("behind > 1", "dense"),
            ("behind > 1", "list"), "one kind only"]
    missing = [w for w in want if w not in seen]
    assert not missing, missing


def test_raw_maxima_and_minima_alternate_in_every_constructed_row():
    """nmx_dense_pair falls back to a bisection when the raw maxima and minima of a window do not alternate.  They always
    do (between two strict maxima of a sequence lies a minimum, plateaus included), so no constructed series reaches that
    branch: it is unreachable by construction, and NOT tested."""
    from oracle import nm_oracle as orc

    for name in cases.CASES:
        for y in cases.case_rows(name).reshape(-1, cases.CASES[name]["W"]):
            a, b = orc.find_peaks_distance(y, None), orc.find_peaks_distance(-y, None)
            kinds = np.concatenate([np.zeros(len(a), int), np.ones(len(b), int)])[np.argsort(np.concatenate([a, b]), kind="stable")]
            assert np.all(np.diff(kinds) != 0), name
