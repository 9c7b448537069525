"""Probes of the bursts chain in the single-thread emulator (tests/emu/nmx_emu.cpp): every case of tests/burst_probe_cases.py on
the forms the emulator reaches (the workgroup walk -- tiled beyond 65 536 entries --, the generic Hilbert item, the LDS run
statistics), which validates inputs, glue and limits before any GPU time is spent; and the conditions the probes rest on,
asserted on the reference alone: margins, decisions and sensitivity of every constructed row, the yardstick's cap, the share
of noise rows the reference leaves out, the run-edge classes reached, the restated plan choices and walk schedule against
the source text, and the kernel set the cases assert against every name the launchers can report.  The figures observed
are in profiles/burst_probes.md."""

import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import burst_probe_cases as cases  # noqa: E402

CSRC = ROOT / "py_neuromodulation_amd" / "csrc"
_B = "nmx_kern_burst_"


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


@pytest.mark.parametrize("name", cases.EMU_CASES)
def test_case_on_the_emulator(emu_lib, name):
    rep = cases.run_case(emu_lib, name)
    c = cases.CASES[name]
    assert rep.rows == c["C"] * 2 * cases.n_hops(c)
    assert rep.table.shape[0] == cases.n_hops(c)


@pytest.mark.parametrize("name", cases.CONSTRUCTED)
def test_conditions_of_a_constructed_case(name):
    """Every row: the yardstick within its cap (env_limits), margin >= 1e-3 max env, the decisions of stream (a) equal to the
    pattern, and one run boundary moved by one sample moves duration_mean, duration_max or amplitude_mean by >= 10 limits."""
    worst = cases.check_conditions(name)
    print(f"BURSTPROBE {name:14s} smallest margin {worst:.4f} max env")
    assert worst >= cases.MARGIN


@pytest.mark.parametrize("name", [n for n, c in cases.CASES.items() if c["kind"] == "noise"])
def test_noise_rows_the_reference_alone_leaves_out(name):
    share = cases.noise_left_out(name)
    print(f"BURSTPROBE {name:14s} reference alone leaves out {100 * share:.2f} %")
    assert share <= cases.NOISE_LEFT_OUT


def test_quieter_stream_does_what_it_was_built_for():
    """Stream (b): the threshold steps once when the ring is full, into the gap between the new highs and the old ones; the
    windows straddling the ramp hold 225, 200, .. 25 samples above it, the rows behind them none."""
    for name, full in (("quiet2", 11), ("quiet5", 41)):
        hops = cases.reference(name)["hops"]
        for ci in range(3):
            thr = np.array([h["thr"][ci, 0] for h in hops]) / cases.SCALES[ci]
            n = [int((h["env"][ci, 0] >= h["thr"][ci, 0]).sum()) for h in hops]
            assert np.ptp(thr[:full]) < 1e-6 * thr[0] and cases.LO + 10 < thr[0] < cases.HI - 10
            assert np.all(thr[full:] > thr[0] + 10) and np.all(thr[full:] < cases.HI - 10) and np.all(np.diff(thr) >= 0)
            assert n[:full] == [250] * full and n[full:full + 9] == list(range(225, 0, -25)) and not any(n[full + 9:]), (name, ci, n)
            assert len(n) - (full + 9) >= 5


def test_convolution_is_the_oracles_bank():
    """The float64 direct convolution against oracle.nm_oracle.fir_bank_apply at 1e-12 max|y|, and the whole reference of a
    noise case against oracle.nm_oracle.Bursts fed the same windows (thresholds and six outputs)."""
    from oracle import nm_oracle as orc

    for name in ("ring2", "rate2000"):
        c = cases.CASES[name]
        x, _ = cases.case_input(name)
        ref = cases.reference(name)
        taps = np.stack(ref["taps"])
        ob = orc.Bursts(cases.case_settings(c), ["ch0", "ch1"], c["sfreq"], taps=taps)
        for h in range(0, cases.n_hops(c), 7 if name == "ring2" else 29):
            xw = x[:, h * c["hop"]:h * c["hop"] + c["W"]].astype(np.float64)
            y64, _ = cases.band_series(xw, ref["taps"], c["M"])
            want = orc.fir_bank_apply(xw, taps)
            assert np.abs(y64 - want).max() <= 1e-12 * np.abs(want).max()
        for h in range(12):
            got = ob.calc_feature(x[:, h * c["hop"]:h * c["hop"] + c["W"]].astype(np.float64))
            hp = ref["hops"][h]
            assert np.allclose(ob.last_thr, hp["thr"], rtol=1e-11, atol=0)
            for ci in range(2):
                for bi, band in enumerate(cases.BANDS):
                    if hp["margin"][ci, bi] < 1e-9 * hp["emax"][ci, bi]:
                        continue
                    st = cases.stats_of(hp["env"][ci, bi], hp["env"][ci, bi] >= hp["thr"][ci, bi], c["sfreq"], ref["seg_s"], 0.0)
                    for s in cases.SLOTS:
                        assert st[s][0] == pytest.approx(float(got[f"ch{ci}_bursts_{band}_{s}"]), rel=1e-9, abs=1e-300), (name, h, ci, band, s)


def test_run_statistics_are_the_oracles():
    """stats_of (from decisions, run by run) against oracle.nm_oracle.burst_stats on every row of four cases."""
    from oracle import nm_oracle as orc

    for name in ("w1000", "w901", "quiet2", "ring2"):
        c, ref = cases.CASES[name], cases.reference(name)
        for hp in ref["hops"]:
            want = orc.burst_stats(hp["env"], hp["thr"], c["sfreq"], ref["seg_s"])
            for ci in range(c["C"]):
                for bi in range(2):
                    got = cases.stats_of(hp["env"][ci, bi], hp["env"][ci, bi] >= hp["thr"][ci, bi], c["sfreq"], ref["seg_s"], 0.0)
                    for s in cases.SLOTS:
                        assert got[s][0] == pytest.approx(float(want[s][ci, bi]), rel=1e-13, abs=1e-300), (name, s)


def test_limits_hold_for_a_float32_restatement():
    """The output limits against the statistics done the plain way in float32 on the float32-rounded float64 envelope
    (sequential sums, true divisions): a limit a correct single-precision evaluation misses would be a wrong derivation."""
    f32 = np.float32
    for name in ("w1000_q50", "w2500", "ring2"):
        c, ref = cases.CASES[name], cases.reference(name)
        L = cases.env_limits(name, ref)
        for h, hp in enumerate(ref["hops"][:8]):
            for ci in range(c["C"]):
                env, b = hp["env"][ci, 0], hp["env"][ci, 0] >= hp["thr"][ci, 0]
                want = cases.stats_of(env, b, c["sfreq"], ref["seg_s"], L[h, ci, 0])
                e32 = env.astype(f32)
                starts, ends, n_trans = cases.runs_of(b)
                nb = n_trans // 2
                dmean = f32(f32(f32(b.sum()) / f32(nb)) / f32(c["sfreq"])) if nb else f32(0)
                got = {"duration_mean": dmean, "burst_rate_per_s": f32(dmean / f32(ref["seg_s"])), "in_burst": f32(b[-1]),
                       "amplitude_max": (e32 * b).max(), "duration_max": f32(0), "amplitude_mean": f32(0)}
                if len(ends):
                    got["duration_max"] = f32(f32((ends - starts[:len(ends)]).max()) / f32(c["sfreq"]))
                    acc = f32(0)
                    for s, e in zip(starts, ends):
                        run = f32(0)
                        for v in e32[s:e]:
                            run = f32(run + v)
                        acc = f32(acc + f32(run / f32(e - s)))
                    got["amplitude_mean"] = f32(acc / f32(len(ends)))
                for s, (v, lim) in want.items():
                    assert abs(float(got[s]) - v) <= lim, (name, h, ci, s, float(got[s]), v, lim)


def test_run_edge_classes_reached():
    """From the reference's own decisions on the constructed rows (the kernels take the same: the margins): every class of run
    position the case table names is reached in a case whose plan, on the MI355X, runs that statistics kernel."""
    seen = set()
    for name in cases.CONSTRUCTED:
        seen |= cases.edge_classes(name)
    common = ["run from 0", "run ending at W - 1", "odd transitions", "four lanes", "runs"]
    want = []
    for kind, ch in (("stat_reg<16>", 16), ("stat_reg<32>", 32)):
        want += [(kind, w) for w in common + ["run ending at W - 2", "two runs in one lane", "start in the last partly filled lane",
                                             "end in the last partly filled lane"]]
        want += [(kind, e, r) for e in ("start", "end") for r in range(ch)]   # (every residue: both sides of every lane boundary)
    want += [("stat", w) for w in common + ["run ending at W - 2", "two runs in one lane", "end in the last partly filled lane"]]
    want += [("stat", "seam", "across")]   # (W = 2500: the LDS form has no tiles; a run across sample 2048 all the same)
    want += [("stat_scan", w) for w in common] + [("stat_scan", "seam", w) for w in ("start at it", "end before it", "across")]
    want += [("stat_scan", e, r) for e in ("start", "end") for r in (0, 31)]
    want += [("stat_reg<16>", "no run")]
    missing = [w for w in want if w not in seen]
    assert not missing, missing
    assert {cases.lane_width(n) for n in ("w901", "w2500", "w14000")} == {15, 40, 219}


def test_restated_plan_choices_are_the_sources():
    """plan_choice and walk_kernels against the text of build_bursts, build_hilbert, nmx_burst_walk_plan, nmx_burst_walk_schedule
    and the launchers; the cases' `walk` tables against the restated schedule."""
    plan = (CSRC / "nmx_engine_plan_bursts.inc").read_text()
    for line in ('*K = std::min((int)std::floor((1.0 - q) * (double)(*n_ring - 1)) + 2, *n_ring);',
                 '*n_ring = (int)(d.sfreq * d.burst_time_duration_s);',
                 'T.overlap = (int)(d.sfreq * seg_s / d.feat_hz);',
                 'if (T.overlap == 0 || T.overlap > d.window) T.overlap = d.window;',
                 'if ((size_t)(H.hil_full ? 2 * al4(2 * d.window) : 2 * al4(d.window + 2) + al4(d.window)) * 4 > 160 * 1024)',
                 'const bool wave = env_int("NMX_HILBERT_W500", 1) != 0;', 'if (d.window == 2000) {',
                 'P.bursts.hil_kind = wave && d.window == 1000 ? NMX_HIL_W500 : wave && H.w1000_tab ? NMX_HIL_W1000 : NMX_HIL_FIXED128;',
                 'B.sparse = sparse != 0 && B.own_hilbert && (B.hil_kind == NMX_HIL_W500 || B.hil_kind == NMX_HIL_W1000);',
                 'S.scan_tile = d.window > 16384 ? NMX_BSTAT_TILE : 0;',
                 'B.stat_kind = S.scan_tile ? NMX_BSTAT_SCAN : (d.window & 3) || d.window > 2048 ? NMX_BSTAT_GENERIC',
                 ': d.window <= 1024 ? (B.sparse ? NMX_BSTAT_REG16_SPARSE : NMX_BSTAT_REG16)',
                 'if (nmx_burst_thr_tiled(T.K)) B.nt_thr = NMX_THR_TILE_NT;',
                 'else if ((T.K + B.nt_thr - 1) / B.nt_thr > 128) B.nt_thr = 1024;',
                 'B.fill_split = env_int("NMX_FILL_SPLIT", 1) != 0;', 'bool wave = env_int("NMX_THR_WAVE", 1) != 0;',
                 'B.walk = nmx_burst_walk_plan(T, env_int("NMX_THR_FILL", 1) != 0, wave, env_int("NMX_THR_LIST_LDS", 1) != 0);',
                 'be_d2h_sync(q + P.bursts.top_bytes, P.bursts.d_counts, P.bursts.counts_bytes);',
                 'be_memset_sync(B.d_top, 0, B.top_bytes);', 'B.top_bytes = n_state * T.K * sizeof(float);',
                 'B.counts_bytes = n_state * 2 * sizeof(long long);'):
        assert line in plan, line
    assert "int nt_thr = 256;" in (CSRC / "nmx_engine.inc").read_text()
    assert 'P->chunk_windows = env_int("NMX_CHUNK_WINDOWS", 1024);' in (CSRC / "nmx_engine_abi.inc").read_text()
    # (the bursts' section is the blob's first)
    assert re.search(r"kStateSections\[\] = \{\s*\{burst_state_bytes,", (CSRC / "nmx_engine_abi.inc").read_text())
    kern = (CSRC / "nmx_k_bursts.h").read_text()
    for line in ('#define NMX_THR_REG_MAX 65536', 'static inline bool nmx_burst_thr_tiled(int K) { return K > NMX_THR_REG_MAX; }',
                 'static inline int nmx_burst_thrw_nr(const NmxBurstThrArgs& A) { return A.overlap <= 128 ? 2 : 4; }',
                 'if (A.overlap < 1 || A.overlap > 256 || A.overlap + 8 >= 192 * nr) return NMX_WALK_NEVER;',
                 'if (!(A.K > 2 * 256 * nr && ia_ring >= A.K - 3 && ia_ring < A.K)) return NMX_WALK_NEVER;',
                 'return short_of <= 0 ? 1 : 1 + (short_of + A.overlap - 1) / A.overlap;',
                 'return (size_t)(f + K / 64 + 4) * 4 + (list ? (size_t)K * 4 : 0);',
                 'const long long per_round = 256LL * (long long)((160 * 1024) / K.lds_list), n_seq = (long long)A.n_channels * A.n_bands;',
                 'K.list_lds_until = list_lds && K.nr == 2 && K.lds_list <= 80 * 1024 && n_seq <= 2 * per_round ? 4096 : 0;',
                 '#define NMX_THRW_I 256', '#define NMX_THRW_PF_LL 8', '#define NMX_THR_P 1024', '#define NMX_BSTAT_TILE 2048',
                 '#define NMX_THRW_LDS_FLOATS_OF(NR, LL) (2 * 256 * (NR) + 3 * ((NR) == 2 ? NMX_THR_P : 512) + NMX_THRW_I + '
                 'NMX_THRW_PF_OF(NR, LL) * 64 * (NR))',
                 'const int chunk = (W + NMX_NT - 1) / NMX_NT;'):
        assert line in kern, line
    assert 2 * 256 * 2 + 3 * 1024 + 256 + 8 * 64 * 2 == 5376   # NMX_THRW_LDS_FLOATS_OF(2, true), as plan_choice has it
    fill = (CSRC / "nmx_k_burst_fill.h").read_text()
    for line in ('#define NMX_FILL_MAX 32768', 'if (K.fill && seen == 0 && nw >= 2) {', 'if (done < nw && K.wave_from > seen + done) {',
                 'const long long maxn = ((long long)NMX_FILL_MAX - A.W) / A.overlap + 1;',
                 'if (done < nw) seg[n_seg++] = NmxBurstWalkSeg{done, nw - done, NMX_WALK_WAVE, seen + done < K.list_lds_until};'):
        assert line in fill, line
    api = (CSRC / "nmx_api.hip").read_text()
    for line in ('else if (nt > 256) NMX_LAUNCH(nmx_kern_burst_thr_wide, dim3(n_items), dim3(1024), lds, s, A);',
                 'else if (chunk <= 32) NMX_LAUNCH(nmx_kern_burst_thr<32>, dim3(n_items), dim3(nt), lds, s, A);',
                 'else if (chunk <= 64) NMX_LAUNCH(nmx_kern_burst_thr<64>, dim3(n_items), dim3(nt), lds, s, A);',
                 'if (split && lds_walk <= 48 * 1024) {'):
        assert line in api, line
    wave = (CSRC / "nmx_wave.hip").read_text()
    for line in ('if (nr == 2 && list_lds) NMX_LAUNCH((nmx_kern_burst_thr_wave<2, true>), dim3(n_items), dim3(64), lds, s, *A);',
                 'else if (nr != 2) NMX_LAUNCH((nmx_kern_burst_thr_wave<4, false>), dim3(n_items), dim3(64), lds, s, *A);',
                 'if (A->full) NMX_LAUNCH(nmx_kern_hilbert_w500_sparse,', 'if (A->full) NMX_LAUNCH(nmx_kern_hilbert_w1000_sparse,'):
        assert line in wave, line
    # a few choices by value
    ch = cases.plan_choice(1000, 1000.0, 30.0, 75.0)
    assert (ch["K"], ch["overlap"], ch["hilbert"], ch["stat"], ch["thr"], ch["wave_from"], ch["wave"]) == \
        (7501, 100, "nmx_kern_hilbert_w500_sparse", _B + "stat_reg_sparse<16>", _B + "thr<32>", 291, _B + "thr_wave<2, true>")
    assert cases.case_choice("ring5")["K"] == 1251 and cases.case_choice("ring5")["wave_from"] == 41
    assert cases.case_choice("ring2")["K"] == 501 and cases.case_choice("ring2")["wave_from"] is None
    assert cases.case_choice("rate2000")["wave"] == _B + "thr_wave<4, false>"
    assert cases.case_choice("w14000")["K"] >= 15400 and cases.case_choice("w14000")["hilbert"] == "nmx_kern_hilbert_long"
    assert [cases.case_choice(n)["K"] for n in ("k64", "k128", "wide", "tiled")] == [10001, 25001, 33751, 67501]
    assert cases.case_choice("w901")["overlap"] == 53 == cases.CASES["w901"]["hop"]
    for name, c in cases.CASES.items():
        assert [set(b) for b in cases.walk_kernels(name)] == [set(b) for b in c["walk"]], name
        assert len(c["walk"]) == len(c["batches"]), name
        # (while K >= the samples appended the list holds every sample: the cases of the first group)
        if c["kind"] == "constructed":
            assert cases.case_choice(name)["K"] >= c["W"] + (cases.n_hops(c) - 1) * c["hop"], name


def test_the_cases_assert_every_kernel_the_launchers_can_report():
    """Every nmx_kern_hilbert* / nmx_kern_burst* name in the launchers' NMX_LAUNCH / NMX_LAUNCH_AS calls is asserted by a case."""
    text = "".join((CSRC / f).read_text() for f in ("nmx_api.hip", "nmx_wave.hip", "nmx_timeosc.hip", "nmx_hilbert_long.hip"))
    noted = set(re.findall(r"NMX_LAUNCH\(\(?(nmx_kern_(?:hilbert|burst)\w*(?:<[^>]*>)?)", text))
    noted |= set(re.findall(r'NMX_LAUNCH_AS\("(nmx_kern_(?:hilbert|burst)[^"]*)",', text))
    assert 'NMX_LAUNCH_AS("nmx_kern_hilbert_fixed" NMX_STR(NMX_BLOCK_FIXED),' in text and "nmx_hilbert_fixed_launch128(&A" in text
    noted.add("nmx_kern_hilbert_fixed128")
    assert noted == cases.ALL_KERNELS, sorted(noted ^ cases.ALL_KERNELS)
    asserted = set().union(*(cases.expected_kernels(n) for n in cases.CASES))
    assert asserted == cases.ALL_KERNELS, sorted(asserted ^ cases.ALL_KERNELS)
