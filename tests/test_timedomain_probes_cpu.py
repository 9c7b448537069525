"""Per-window probes of the time-domain statistics in the single-thread emulator (tests/emu/nmx_emu.cpp): every case of
tests/timedomain_probe_cases.py on the item the emulator runs for its plan -- the two-pass LDS item (every length of
classes a, b, e; the two-pass kernels of c, d, f), the long-window item (c_long13655) and the restatement of the
matrix-pipe kernel's single-pass arithmetic with its flag protocol (c_specmm, f_specmm_*) -- against the same float64
reference and under the same policy as the MI355X tier: it proves the cases, the reference and the expectations before any
GPU time is spent.  And the ties that hold the probes together: the conditioning of every white-noise recording, the
vectorised reference against oracle.Hjorth / LineLength / Raw, the restated plan choices against the source text, the
coverage of every kernel and load variant the table names, the matrix-pipe kernel's cancellation flag on clean
recordings.  The figures observed are in profiles/timedomain_probes.md."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import timedomain_probe_cases as cases  # noqa: E402

CSRC = ROOT / "py_neuromodulation_amd" / "csrc"


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_on_the_emulator(emu_lib, name):
    """Every case; of the two degenerate cases of 1000 samples every row but the two of cases.EMU_CANNOT."""
    rep = cases.run_case(emu_lib, name)
    c = cases.CASES[name]
    assert rep.left_out == len(cases.EMU_CANNOT.get(name, ())) and rep.n == c["C"] * c["hops"] - rep.left_out


@pytest.mark.parametrize("name", [n for n, c in cases.CASES.items() if c["white"]])
def test_white_noise_cases_are_well_conditioned(name):
    """draw() redraws until +-1 ulp on every float32 sample moves every reference entry by less than 1e-6 relative; the
    seed it settles on is the case's own (no redraw is needed for the table as it stands: a redraw is printed)."""
    c = cases.CASES[name]
    x, seed, k = cases.draw(name)
    assert k < cases.COND_RTOL
    if seed != c["seed"]:
        print(f"TDPROBE {name}: seed {c['seed']} redrawn as {seed}")


def test_the_conditioning_check_can_fail():
    """A window whose first differences all but cancel moves mobility far beyond 1e-6 under +-1 ulp."""
    W = 64
    bad = (np.full((1, W), 1000.0) + 1e-4 * np.random.default_rng(1).standard_normal((1, W))).astype(np.float32)
    assert cases.conditioning(bad, [0], W) > cases.COND_RTOL


@pytest.mark.parametrize("name", list(cases.CASES))
def test_reference_is_the_oracles(name):
    """The vectorised float64 restatement against oracle.Hjorth / LineLength / Raw .calc_feature on the first, the last and
    three windows between of every case: exactly equal."""
    c = cases.CASES[name]
    x, _, _ = cases.draw(name)
    x32 = cases.split(x, cases.host_offsets(x))
    st = cases.starts_of(c)
    pick = sorted({0, len(st) // 3, len(st) // 2, (2 * len(st)) // 3, len(st) - 1})
    ref = cases.reference(x32, st[pick], c["W"])
    ch = [f"ch{i}" for i in range(c["C"])]
    rows = cases.oracle_rows(x32, st[pick], c["W"], ch, cases.TD)
    for i, row in enumerate(rows):
        assert len(row) == 5 * c["C"]
        for key, v in row.items():
            cname, what = cases.td_key(key)
            assert float(v) == ref[what][i, ch.index(cname)], (name, key, float(v), ref[what][i, ch.index(cname)])


def test_restated_plan_choices_are_the_sources():
    cases.source_ties(CSRC)
    c = cases.CASES
    assert cases.timeosc_kind(c["a_W1024"]) == "SCAN" and cases.timeosc_kind(c["a_W1028"]) == "GENERIC"
    assert cases.timeosc_kind(c["c_long13655"]) == "LONG" and cases.timeosc_kind(c["c_specmm"]) == "SPECMM"
    assert cases.persistent_launches(256, 7, 1100, c["d_c7"]["env"]) == [(7168, 3066, 3), (532, 532, 1)]
    assert cases.persistent_launches(256, 1, 3100, c["d_c1"]["env"]) == [(3100, 3072, 2)]
    assert cases.persistent_launches(256, 7, 1100, {}) == [(896, 896, 1), (3584, 3066, 2), (3220, 3066, 2)]   # (the defaults)


def test_the_table_names_every_kernel_and_load_variant():
    """Every kernel name and every nmx_td_* load variant of the table is the expectation of at least one case, every class
    has its cases, and classes c and f run every W = 1000 kernel."""
    assert {cases.kernel_name(c) for c in cases.CASES.values()} == cases.KERNELS
    assert {cases.variant(c) for c in cases.CASES.values()} == cases.VARIANTS
    assert {c["cls"] for c in cases.CASES.values()} == set("abcdef")
    w1000 = {cases.kernel_name(c) for c in cases.CASES.values() if c["cls"] == "c" and c["W"] == 1000}
    assert w1000 == cases.KERNELS - {"nmx_kern_timeosc", "nmx_kern_timeosc_long", "nmx_kern_timeosc_w510<4>"}
    for where in cases.ART_SETS:
        assert {cases.kernel_name(c) for c in cases.CASES.values() if c["cls"] == "f" and c["where"] == where} == w1000
    assert {c["W"] for c in cases.CASES.values() if c["cls"] == "a" and cases.variant(c) == "td_emit<0>"} == set(cases.PACKED_W)
    assert {c["W"] for c in cases.CASES.values() if c["cls"] == "a" and cases.variant(c) == "scan"} == set(cases.SCALAR_W)
    for c in cases.CASES.values():
        if c["cls"] == "b":   # every residue of the window starts mod 4
            assert set((cases.starts_of(c) % 4).tolist()) == {0, 1, 2, 3}


def test_bad_sample_positions_and_degenerate_rows():
    assert cases.bad_positions(1000) == [0, 255, 256, 768, 999] and cases.bad_positions(260) == [0, 255, 256, 259]
    rows = cases.degenerate_rows(1000)
    for r in rows:
        assert np.array_equal(r, r.astype(np.float32))
    ref = cases.reference(np.stack(rows).astype(np.float32), [0], 1000)
    assert ref["RawHjorth_Mobility"][0, 0] == 0 and ref["RawHjorth_Mobility"][0, 1] == 0 and ref["RawHjorth_Mobility"][0, 2] > 1
    assert cases.zero_mobility_bound(0.5, float(ref["RawHjorth_Activity"][0, 1])) < 1e-9


def test_degenerate_rows_need_the_kernels_summation_order():
    """The two rows the emulator tier leaves out of the degenerate cases of 1000 samples (cases.EMU_CANNOT): the two-pass
    formulas meet the policy on every row with 128 accumulators and a tree (the device kernel's order); with one accumulator
    (the emulator's) they miss it on exactly those two rows -- the miss is the stand-in's, and says nothing about a kernel."""
    rows = np.stack(cases.degenerate_rows(1000)).astype(np.float32)
    ref = cases.reference(rows, [0], 1000)
    worst, missing = {1: 0.0, 128: 0.0}, set()
    for lanes in worst:
        for i, r in enumerate(rows):
            got = cases.two_pass_f32(r, lanes)
            for g, nm in zip(got, ("RawHjorth_Activity", "RawHjorth_Mobility", "RawHjorth_Complexity")):
                w = float(ref[nm][0, i])
                if w != 0:
                    worst[lanes] = max(worst[lanes], abs(g - w) / abs(w))
                    if lanes == 1 and abs(g - w) > 1e-5 * abs(w):
                        missing.add(divmod(i, 4))   # (hop, channel) of row i in the cases: C = 4
    assert missing == set(cases.EMU_CANNOT["e_degenerate_scan1000"]) == set(cases.EMU_CANNOT["e_degenerate_w1000"]), missing
    print(f"TDPROBE degenerate rows, two-pass float32: worst relative error {worst[128]:.1e} with 128 accumulators, {worst[1]:.1e} with one")
    assert worst[128] < 1e-6 and worst[1] > 1e-5


# ---- the matrix-pipe kernel's single pass -----------------------------------------------------------------------------------
def test_specmm_flag_derivation_and_clean_recordings():
    """nmx_k_specmm.h flags a window for the two-pass redo when q0 > NMX_SMM_CANCEL (q0 - s0^2 / W): the restated numbers
    against the source, the threshold against the error model, and white noise with offsets up to +-500 (the existing
    tests' recordings) never trips it."""
    src = (CSRC / "nmx_k_specmm.h").read_text()
    assert f"#define NMX_SMM_CANCEL {cases.SMM_CANCEL:.1f}f" in src
    # the error model: ratio x 2^-24 x roundings a decade under the policy
    assert cases.SMM_CANCEL * 2.0 ** -24 * cases.SMM_ROUNDINGS <= 1e-6
    worst = 0.0
    for seed in range(40):
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal((64, 1000)) * 50 + rng.uniform(-500, 500, (64, 1))).astype(np.float32)
        worst = max(worst, float(cases.specmm_cancellation(x).max()))
    print(f"TDPROBE specmm cancellation ratio of 2560 clean windows: at most {worst:.2f} (flag at {cases.SMM_CANCEL})")
    assert worst < cases.SMM_CANCEL
    # ... and every artifact of class f on the pivot's samples reaches the flag, the control does not
    def ratios(name):
        c = cases.CASES[name]
        x = cases.data_artifacts(c, c["seed"]).astype(np.float32)
        return cases.specmm_cancellation(np.stack([x[ch, h * 1000:(h + 1) * 1000] for h in range(c["hops"]) for ch in range(c["C"])]))

    for where in ("centre", "ends", "all4", "burst"):
        assert ratios(f"f_specmm_{where}").min() > cases.SMM_CANCEL, where
    assert ratios("f_specmm_control").max() < cases.SMM_CANCEL
    for line in ("const float p = 0.25f * ((x[0] + x[999]) + (x[499] + x[500]));", "if (!(q0 <= NMX_SMM_CANCEL * cw)) return true;",
                 "if (!(q0 <= NMX_SMM_CANCEL * cw)) dirty = true;",
                 "N.pilot = 0.25f * ((at(cur + L.opilot) + at(cur + 6144 + L.opilot7)) + (at(cur + 2048 + L.opilot7) + at(cur + 4096 + L.opilot)));"):
        assert line in src, line
