"""Per-hop probes of the feature normaliser (nmx_k_norm.h, nmx_k_power.h, nmx_engine_norm.inc): every method on every path
-- the five-kernel scan, the column walk, the sorted-list family, the Yeo-Johnson fit -- at the history lengths, batch
lengths, row counters and column counts where their control flow changes, each output against the float64 hop-by-hop
oracle (oracle.nm_oracle.FeatureNormalizer).  Cases and policy only; the tiers are tests/test_norm_probes_cpu.py (the
single-thread emulator) and tests/test_norm_probes_gpu.py (one MI355X); the figures observed: profiles/norm_probes.md.

Long histories and large row counters cost nothing: both sides are PRELOADED -- the device through import_state (row q of
the last min(seq, N - 1) rows in slot q % N, every other slot poisoned), the oracle through its `prev`.

Gates (no miss is accepted, nothing is forgiven):
  * project tolerance 1e-5 relative + 2e-6 absolute on every entry, +-inf / +-max compared through huge();
  * exact: masked and guard columns and the first row ever come back bitwise, a constant column gives 0.0 on every later
    hop of mean / zscore (the correctly rounded quotient), an empty window gives 0.0;
  * tight, mean / zscore on the generic, drifting and cancellation columns:
        |got - want| <= 1 fp32 ulp of want + K eps64 (|x| + |mean|) / d,    d = std (zscore), |mean| (mean)
    (numerator: x - mean carries eps64 (|x| + |mean|); the divisor's relative error times |out| <= (|x| + |mean|) / d is
    of the same form).  K = 16 x the oracle's OWN float64 noise in these units -- its NumPy result against a two-pass
    np.longdouble evaluation of the same windows -- rounded up to a power of two (oracle_noise; pinned by the CPU tier).
"""

import re
import struct
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
TOL_REL, TOL_ABS = 1e-5, 2e-6
EPS64 = 2.0 ** -52
K_TIGHT = 256.0   # 16 x 15.5 (the oracle's worst float64 noise over every window of SCAN_CASES and WALK_CASES) -> 2^8
POISON = np.float32(7.7e7)   # ring slots outside the history: a kernel that reads one misses every gate

# ---- the launcher's choice, restated (nmx_norm_process in nmx_engine_norm.inc; pinned to its text by the CPU tier) --------
SCAN_MIN_ROWS, SCAN_MIN_HIST, SCAN_CAP_LIMIT = 8, 64, 65536
NORM_PF, NORM_SEG = 8, 32
MZ = (("zscore", 3), ("mean", 3), ("zscore", 0), ("mean", 0))


def takes_scan(method, N, n_rows, scan_on=True):
    return bool(scan_on and method in ("mean", "zscore") and n_rows >= SCAN_MIN_ROWS and N - 1 >= SCAN_MIN_HIST
                and N < SCAN_CAP_LIMIT)


def piece_len(N, n_rows):
    return min(n_rows, N - 1)


def source_thresholds():
    """(min rows, min history, cap limit, piece expression present, PF, SEG) as the sources state them."""
    inc = (ROOT / "py_neuromodulation_amd" / "csrc" / "nmx_engine_norm.inc").read_text()
    hdr = (ROOT / "py_neuromodulation_amd" / "csrc" / "nmx_k_norm.h").read_text()
    m = re.search(r"const bool scan = H->scan_on && \(H->method == NMX_NORM_MEAN \|\| H->method == NMX_NORM_ZSCORE\) && "
                  r"N\.n_rows >= (\d+) &&\s*H->cap - 1 >= (\d+) && H->cap < (\d+);", inc)
    assert m, "the scan predicate of nmx_norm_process is no longer the text the probes restate"
    piece = "const int piece = std::min<int>(N.n_rows, H->cap - 1);" in inc
    pf = int(re.search(r"#define NMX_NORM_PF (\d+)", hdr).group(1))
    seg = int(re.search(r"#define NMX_NORM_SEG (\d+)", hdr).group(1))
    return int(m.group(1)), int(m.group(2)), int(m.group(3)), piece, pf, seg


# ---- inputs ---------------------------------------------------------------------------------------------------------------
KINDS = ("generic", "constant", "drift", "cancel", "nan_scatter", "nan_run", "ninf_run", "pinf_ninf", "tiny")
TIGHT = ("generic", "drift", "cancel")
ORDER_KINDS = ("wide", "tie", "nan_scatter", "constant", "tiny")


def masked_columns(n_cols):
    """Four masked columns, the first and the last of a 64-wide block among them; none below 14 columns."""
    if n_cols < 14:
        return []
    out = []
    for c in (0, 63, 64, n_cols - 1, n_cols // 2, 7):
        if 0 <= c < n_cols and c not in out:
            out.append(c)
    return sorted(out[:4])


def layout(n_cols, kinds):
    masked = masked_columns(n_cols)
    names, k = [], 0
    for j in range(n_cols):
        if j in masked:
            names.append("masked")
        else:
            names.append(kinds[k % len(kinds)])
            k += 1
    return names


def _inf_places(N, have, batches):
    """(start of the -inf run, place of the lone +inf) as stream indices: the run enters early in the first batch and leaves
    N - 1 hops later; +inf is the last row of the first piece of a batch longer than N and the -inf that follows it the
    second row of the next piece."""
    b0 = have
    for b in batches:
        if b > N and N > 3:
            return have + 3, b0 + (N - 1) - 1
        b0 += b
    return have + 3, have + 6


def make_stream(seed, N, n_cols, have, batches, kinds):
    """float32 [have + sum(batches)][n_cols]: the history the launch finds, then the probe rows; every column its own
    offset and scale."""
    rng = np.random.default_rng(seed)
    L = have + int(sum(batches))
    names = layout(n_cols, kinds)
    run0, pinf = _inf_places(N, have, batches)
    x = np.empty((L, n_cols), np.float64)
    i = np.arange(L)
    for j, kind in enumerate(names):
        off, sc = rng.uniform(-50, 50), rng.uniform(0.01, 30)
        col = rng.standard_normal(L) * sc + off
        if kind == "generic":      # |mean| >= 4 std: the "mean" method's quotient is well conditioned
            col = rng.standard_normal(L) * rng.uniform(0.5, 5) + rng.choice((-1.0, 1.0)) * rng.uniform(20, 50)
        elif kind == "constant":
            col[:] = np.round(off, 2) if abs(off) > 0.5 else 2.5 + j
        elif kind == "drift":
            col = np.cumsum(np.abs(col - off)) + 1e4 + j
        elif kind == "cancel":
            col = 1e4 + 3 * j + 1e-3 * rng.standard_normal(L)
        elif kind in ("nan_scatter", "masked"):
            col[rng.random(L) < 0.1] = np.nan
            if kind == "masked" and L > 4:
                col[4] = np.inf
        elif kind == "nan_run":    # the whole history and the first hops; then a run longer than N inside the probe rows
            col[:min(L, have + 3)] = np.nan
            if L - have >= N + 12:
                col[have + 8:have + 8 + N + 2] = np.nan
        elif kind == "ninf_run":
            col[run0:run0 + 12] = -np.inf
            if have == N - 1 and have >= 8:
                col[4:8] = -np.inf   # found in the history, leaves during the first hops
        elif kind == "pinf_ninf":
            if pinf < L:
                col[pinf] = np.inf
            if pinf + 2 < L:
                col[pinf + 2] = -np.inf
        elif kind == "tiny":
            col = np.abs(col - off) / sc * 1e-6 * (1 + j % 7)
            col[i % 97 == 3] = 40.0
        elif kind == "tie":
            col = np.round(col) + 0.0   # (no -0.0: the sign of a zero median is nobody's to define)
        elif kind == "wide":
            pass
        else:
            raise KeyError(kind)
        x[:, j] = col
    with np.errstate(over="ignore"):
        return x.astype(np.float32), names


def huge(a):
    """nan_to_num(+-inf) is the dtype's max: float64 in the reference, fp32 on the device."""
    a = np.array(a, dtype=np.float64)
    big = np.abs(a) >= 1e37
    a[big] = np.sign(a[big]) * np.inf
    return a


def settings_for(method, clip, N):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.sampling_rate_features_hz = 1
    s.feature_normalization_settings.normalization_time_s = N
    s.feature_normalization_settings.normalization_method = method
    s.feature_normalization_settings.clip = clip
    return s


# ---- the two sides --------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_rows(key, method, clip, N, stream, have, mask):
    """The oracle hop by hop over the probe rows of the unmasked columns, its history preloaded; computed once per key and
    handed out read-only."""
    if key not in _ORACLE:
        from oracle import nm_oracle as orc
        from tests import parity

        ref = orc.FeatureNormalizer(settings_for(method, clip, N))
        wide = np.stack([parity.widen_huge(r) for r in stream[:, mask == 1]])
        if have:
            ref.prev = wide[:have].copy()
        want = np.stack([ref.process(r) for r in wide[have:]])
        want.setflags(write=False)
        _ORACLE[key] = want
    return _ORACLE[key]


def ring_image(N, n_cols, seq0, hist):
    ring = np.full((N, n_cols), POISON, np.float32)
    for k in range(len(hist)):
        ring[(seq0 - len(hist) + k) % N] = hist[k]
    return ring


def make_norm(lib, method, clip, N, n_cols, mask, seq0=0, hist=None, scan_on=True, env=None):
    """A normaliser on `lib` (None: the GPU library), preloaded.  `env` is pytest's monkeypatch: NMX_NORM_SCAN is read when
    the normaliser is created, and never taken from the caller's environment."""
    from py_neuromodulation_amd.processing import DeviceFeatureNormalizer

    if env is not None:
        if scan_on:
            env.delenv("NMX_NORM_SCAN", raising=False)
        else:
            env.setenv("NMX_NORM_SCAN", "0")
    else:
        assert scan_on, "the walk form of a scan case needs monkeypatch"
    dn = DeviceFeatureNormalizer(settings_for(method, clip, N), n_cols, colmask=None if mask.all() else mask, lib=lib)
    if env is not None:
        env.delenv("NMX_NORM_SCAN", raising=False)
    if seq0:
        dn.import_state(struct.pack("<q", seq0) + ring_image(N, n_cols, seq0, hist).tobytes())
    return dn


def host_call(dn, rows):
    return dn.process_batch(rows)


def engine_rows(dn, rows, batches, call=host_call):
    got, r = [], 0
    for b in batches:
        got.append(call(dn, rows[r:r + b]))
        r += b
    assert r == len(rows)
    return np.concatenate(got)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_state(dn, N, seq0, stream, have, mask):
    """export_state() against the ring computed here: the counter, and bitwise the slots of the last N - 1 rows."""
    state = dn.export_state()
    seq = struct.unpack("<q", state[:8])[0]
    total = len(stream) - have
    assert seq == seq0 + total, (seq, seq0 + total)
    ring = np.frombuffer(state[8:], np.float32).reshape(N, -1)
    keep = min(seq, N - 1)
    qs = np.arange(seq - keep, seq)
    rows = stream[len(stream) - keep:] if keep else stream[:0]
    np.testing.assert_array_equal(bits(ring[qs % N][:, mask == 1]), bits(rows[:, mask == 1]))
    return state


def check_tolerance(got, want, label):
    """1e-5 relative + 2e-6 absolute through huge(); returns the worst error as a fraction of the tolerance."""
    g, w = huge(got), huge(want)
    assert g.shape == w.shape, (label, g.shape, w.shape)
    assert np.array_equal(np.isnan(g), np.isnan(w)), label
    inf = np.isinf(w)
    assert np.array_equal(inf, np.isinf(g)) and np.array_equal(g[inf], w[inf]), label
    fin = ~inf & ~np.isnan(w)
    frac = np.abs(g[fin] - w[fin]) / (TOL_REL * np.abs(w[fin]) + TOL_ABS)
    worst = float(frac.max()) if frac.size else 0.0
    if worst > 1.0:
        rr, cc = np.nonzero(fin & ~(np.abs(np.where(fin, g - w, 0.0)) <= TOL_REL * np.abs(np.where(fin, w, 0.0)) + TOL_ABS))
        first = [(int(r), int(c), float(g[r, c]), float(w[r, c])) for r, c in zip(rr[:5], cc[:5])]
        raise AssertionError(f"{label}: {len(rr)} entries beyond 1e-5 rel + 2e-6 abs, worst {worst:.3g} x; "
                             f"(row, unmasked column, got, want): {first}")
    return worst


def window_bounds(N, have, r):
    """Stream indices [lo, hi] of the window of probe row r."""
    return max(0, have + r - (N - 1)), have + r


def window_stats_ld(method, clip, N, col, have, n_probe):
    """(out, mean, divisor) per probe row of one NaN-free column: two passes in np.longdouble."""
    c = col.astype(np.longdouble)
    out, mean, div = np.zeros(n_probe), np.zeros(n_probe), np.ones(n_probe)
    for r in range(n_probe):
        lo, hi = window_bounds(N, have, r)
        w = c[lo:hi + 1]
        m = w.sum() / len(w)
        d = w - m
        sd = np.sqrt((d * d).sum() / len(w))
        dv = abs(m) if method == "mean" else (sd if sd > 0 else np.longdouble(1))
        o = (c[hi] - m) / (m if method == "mean" else dv) if dv != 0 else np.longdouble(0)
        if clip:
            o = min(max(o, -clip), clip)
        out[r], mean[r], div[r] = float(o), float(m), float(dv)
    return out, mean, div


def tight_units(method, clip, N, stream, have, names, mask, first_ever):
    """Per tight column (index among the unmasked ones): (long-double output, eps64 (|x| + |mean|) / divisor) per probe row;
    the first row ever is left out (mask False)."""
    n_probe = len(stream) - have
    cols = [j for j in range(stream.shape[1]) if mask[j]]
    out = {}
    for u, j in enumerate(cols):
        if names[j] not in TIGHT:
            continue
        o, m, d = window_stats_ld(method, clip, N, stream[:, j], have, n_probe)
        unit = EPS64 * (np.abs(stream[have:, j].astype(np.float64)) + np.abs(m)) / np.where(d > 0, d, 1.0)
        ok = np.ones(n_probe, bool)
        if first_ever:
            ok[0] = False
        out[u] = (o, unit, ok)
    return out


def ulp32(w):
    return np.spacing(np.abs(np.asarray(w)).astype(np.float32)).astype(np.float64)


# ---- mean / zscore cases --------------------------------------------------------------------------------------------------
def _b(N):
    return [8, 31, 32, 33, N - 2, N - 1, N, N + 7, 2 * N + 1]


# name: (N, n_cols, seq0, batches, (method, clip) combinations, column kinds)
SCAN_CASES = {
    "n65_from_zero": (65, 23, 0, _b(65), MZ, KINDS),
    "n66_have1": (66, 23, 1, [64, 8, 133, 65, 73], MZ, KINDS),
    "n66_wrap": (66, 23, 66 * 5 + 60, _b(66), MZ[:2], KINDS),
    "n97_have31": (97, 23, 31, [33, 31, 97, 8], MZ[:2], KINDS),
    "n97_have32": (97, 23, 32, [32, 104, 95], MZ[:2], KINDS),
    "n97_have33": (97, 23, 33, [96, 8, 195], MZ[2:], KINDS),
    "n97_2p40": (97, 23, 2 ** 40 + 123, _b(97), MZ[:2], KINDS),
    "n300_from_zero": (300, 23, 0, _b(300), MZ[:2], KINDS),
    "n300_have31": (300, 23, 31, [32, 299, 8], MZ[:2], KINDS),
    "n300_have32": (300, 23, 32, [33, 300], MZ[:2], KINDS),
    "n300_have33": (300, 23, 33, [31, 307], MZ[:2], KINDS),
    "n300_have_nm2": (300, 23, 298, [8, 298, 33], MZ[:2], KINDS),
    "n300_have_nm1": (300, 23, 299, [299, 8, 601], MZ, KINDS),
    "n300_wrap": (300, 23, 300 * 7 + 290, _b(300), MZ[:2], KINDS),
    "n300_2p31": (300, 23, 2 ** 31 + 5, [33, 307, 8], MZ, KINDS),
    "n300_2p40": (300, 23, 2 ** 40 + 123, [300, 31, 32], MZ[:2], KINDS),
    "n65535_preloaded": (65535, 4, 65535 * 3 + 65520, [8, 32], MZ[:2], ("generic", "constant", "cancel", "ninf_run")),
    "n65535_2p31": (65535, 4, 2 ** 31 + 5, [31, 9], MZ[2:], ("drift", "generic", "nan_run", "cancel")),
    "cols1": (97, 1, 200, [33, 97], MZ[:2], ("cancel",)),
    "cols63": (97, 63, 200, [33, 97], MZ[:1], KINDS),
    "cols64": (97, 64, 200, [33, 97], MZ[1:2], KINDS),
    "cols65": (97, 65, 200, [33, 97], MZ[:1], KINDS),
    "cols255": (97, 255, 200, [33, 97], MZ[2:3], KINDS),
    "cols256": (97, 256, 200, [33, 97], MZ[:1], KINDS),
    "cols257": (97, 257, 200, [33, 97], MZ[:2], KINDS),
}
_W = [1, 7, 8, 9, 15, 16, 17]
WALK_CASES = {
    "w2": (2, 23, 0, _W, MZ, KINDS),
    "w3": (3, 23, 0, _W, MZ, KINDS),
    "w3_have2": (3, 23, 2 ** 31 + 5, _W, MZ[:2], KINDS),
    "w8": (8, 23, 0, _W, MZ, KINDS),
    "w9": (9, 23, 5, _W, MZ, KINDS),
    "w10": (10, 23, 0, _W, MZ, KINDS),
    "w10_2p40": (10, 23, 2 ** 40 + 123, _W, MZ[:2], KINDS),
    "w64": (64, 23, 0, _W + _W, MZ, KINDS),
    "w64_wrap": (64, 65, 64 * 9 + 60, _W, MZ[:2], KINDS),
    "w300_short_batches": (300, 23, 300 * 3 + 290, [1, 2, 3, 4, 5, 6, 7], MZ, KINDS),
    "w65536_a": (65536, 4, 65536 * 2 + 65530, [1, 7, 8, 9, 15], MZ[:2], ("generic", "constant", "cancel", "ninf_run")),
    "w65536_b": (65536, 4, 2 ** 31 + 5, [16, 17], MZ[2:], ("drift", "generic", "nan_run", "cancel")),
}
SCAN_OFF_CASES = [n for n, c in SCAN_CASES.items() if c[0] == 300]   # the same inputs with NMX_NORM_SCAN=0


def case_paths(name):
    """[(method, n_rows of the launch, takes the scan)] of every launch of a mean / zscore case, scan enabled."""
    N, _, _, batches, combos, _ = (SCAN_CASES.get(name) or WALK_CASES[name])
    return [(m, b, takes_scan(m, N, b)) for m, _ in combos for b in batches]


def mz_inputs(name):
    N, n_cols, seq0, batches, combos, kinds = (SCAN_CASES.get(name) or WALK_CASES[name])
    have = min(seq0, N - 1)
    seed = sum(name.encode()) * 7919 + N
    stream, names = make_stream(seed, N, n_cols, have, batches, kinds)
    mask = np.array([0 if k == "masked" else 1 for k in names], np.uint8)
    return N, n_cols, seq0, have, batches, combos, stream, names, mask


def exact_properties(got, stream, have, seq0, N, names, mask, label):
    rows = stream[have:]
    np.testing.assert_array_equal(bits(got[:, mask == 0]), bits(rows[:, mask == 0]), err_msg=f"{label}: masked columns")
    first = 1 if seq0 == 0 else 0
    if first:
        np.testing.assert_array_equal(bits(got[0]), bits(rows[0]), err_msg=f"{label}: the first row ever")
    for j, k in enumerate(names):
        if k == "constant":
            np.testing.assert_array_equal(got[first:, j], 0.0, err_msg=f"{label}: constant column {j}")
        if k == "nan_run":
            nan = np.isnan(stream[:, j])
            empty = np.array([nan[slice(window_bounds(N, have, r)[0], have + r + 1)].all() for r in range(len(rows))])
            empty[:first] = False
            assert empty.any(), label
            np.testing.assert_array_equal(got[empty, j], 0.0, err_msg=f"{label}: empty window, column {j}")


def mz_case(lib, name, scan_on=True, env=None, call=host_call):
    """One mean / zscore case on every (method, clip) of its row; returns {(method, clip): (worst fraction of the project
    tolerance, worst error of the tight columns in fp32 ulps)}."""
    N, n_cols, seq0, have, batches, combos, stream, names, mask = mz_inputs(name)
    out = {}
    for method, clip in combos:
        label = f"{name} {method} clip={clip} scan={'on' if scan_on else 'off'}"
        want = oracle_rows((name, method, clip), method, clip, N, stream, have, mask)
        units = tight_units_cached(name, method, clip)
        dn = make_norm(lib, method, clip, N, n_cols, mask, seq0, stream[:have], scan_on, env)
        got = engine_rows(dn, stream[have:], batches, call)
        exact_properties(got, stream, have, seq0, N, names, mask, label)
        frac = check_tolerance(got[:, mask == 1], want, label)
        worst_ulp = 0.0
        g = got[:, mask == 1].astype(np.float64)
        for u, (_, unit, ok) in units.items():
            err = np.abs(g[:, u] - want[:, u])[ok]
            ulp = ulp32(want[:, u])[ok]
            worst_ulp = max(worst_ulp, float((err / ulp).max()) if err.size else 0.0)
            bad = np.nonzero(~(err <= ulp + K_TIGHT * unit[ok]))[0]
            assert bad.size == 0, (f"{label}: tight gate, unmasked column {u}: {bad.size} hops, first "
                                   f"{[(int(b), float(g[:, u][ok][b]), float(want[:, u][ok][b])) for b in bad[:4]]}")
        check_state(dn, N, seq0, stream, have, mask)
        out[(method, clip)] = (frac, worst_ulp)
    return out


_UNITS = {}


def tight_units_cached(name, method, clip):
    key = (name, method, clip)
    if key not in _UNITS:
        N, _, seq0, have, _, _, stream, names, mask = mz_inputs(name)
        _UNITS[key] = tight_units(method, clip, N, stream, have, names, mask, seq0 == 0)
    return _UNITS[key]


def oracle_noise(names_of_cases):
    """Worst |oracle - long double| / (eps64 (|x| + |mean|) / divisor) over the tight columns of the given cases: the
    oracle's own float64 noise in the units of the tight gate."""
    worst = 0.0
    for name in names_of_cases:
        N, _, seq0, have, _, combos, stream, names, mask = mz_inputs(name)
        for method, clip in combos:
            want = oracle_rows((name, method, clip), method, clip, N, stream, have, mask)
            for u, (o, unit, ok) in tight_units_cached(name, method, clip).items():
                worst = max(worst, float((np.abs(want[:, u] - o)[ok] / unit[ok]).max()))
    return worst


def state_crossing_case(lib, env, first_scan):
    """A state exported after a scan batch continues in a walk normaliser (NMX_NORM_SCAN=0), and the reverse; both go on
    matching the oracle."""
    name = "n300_have_nm1"
    N, n_cols, seq0, have, batches, _, stream, names, mask = mz_inputs(name)
    method, clip = "zscore", 3
    want = oracle_rows((name, method, clip), method, clip, N, stream, have, mask)
    rows = stream[have:]
    a = make_norm(lib, method, clip, N, n_cols, mask, seq0, stream[:have], first_scan, env)
    got = [a.process_batch(rows[:299])]
    state = a.export_state()
    b = make_norm(lib, method, clip, N, n_cols, mask, 0, None, not first_scan, env)
    b.import_state(state)
    got += [b.process_batch(rows[299:307]), b.process_batch(rows[307:])]
    got = np.concatenate(got)
    exact_properties(got, stream, have, seq0, N, names, mask, name)
    check_state(b, N, seq0, stream, have, mask)
    return check_tolerance(got[:, mask == 1], want, f"{name} crossing, scan first = {first_scan}")


# ---- the device call shape ------------------------------------------------------------------------------------------------
GUARD = np.float32(-1234.5)


def device_shape_case(lib, env, kind, device_call):
    """process_device with ld = n_cols + 3: the three guard columns come back bitwise, the rest matches the oracle.
    `device_call(dn, buf[n][ld]) -> buf after the call` is the tier's (host pointers in the emulator; a torch tensor and a
    non-default stream on the GPU)."""
    if kind == "power":
        return power_case(lib, "p65_have16", device_call=device_call)
    name = {"scan": "n97_have31", "walk": "w9"}[kind]
    N, n_cols, seq0, have, batches, combos, stream, names, mask = mz_inputs(name)
    method, clip = combos[0]
    want = oracle_rows((name, method, clip), method, clip, N, stream, have, mask)

    def call(dn, rows):
        return padded_call(dn, rows, device_call)

    dn = make_norm(lib, method, clip, N, n_cols, mask, seq0, stream[:have], True, env)
    got = engine_rows(dn, stream[have:], batches, call)
    exact_properties(got, stream, have, seq0, N, names, mask, name)
    check_state(dn, N, seq0, stream, have, mask)
    return check_tolerance(got[:, mask == 1], want, f"{name} device shape")


def padded_call(dn, rows, device_call):
    n, nc = rows.shape
    buf = np.full((n, nc + 3), GUARD, np.float32)
    buf[:, :nc] = rows
    buf = device_call(dn, buf)
    np.testing.assert_array_equal(bits(buf[:, nc:]), bits(np.full((n, 3), GUARD, np.float32)), err_msg="guard columns")
    return np.ascontiguousarray(buf[:, :nc])


# ---- the order and scikit-learn family ------------------------------------------------------------------------------------
ORDER_METHODS = ("median", "zscore-median", "robust", "minmax", "quantile")


def _o(N):
    return [1, 7, 8, 9, N - 1, N, N + 7]


# name: (N, n_cols, seq0, batches)
ORDER_CASES = {
    "o2": (2, 7, 0, _o(2)),
    "o3": (3, 7, 0, _o(3)),
    "o4": (4, 7, 0, _o(4)),
    "o5": (5, 7, 3, _o(5)),
    "o9": (9, 7, 0, _o(9)),
    "o50": (50, 7, 0, _o(50)),
    "o300": (300, 7, 0, _o(300)),
    "o301": (301, 7, 301 * 2 + 290, [1, 7, 8, 9, 308]),
    "o302": (302, 7, 2 ** 31 + 5, [9, 301, 8]),
    "o450": (450, 7, 2 ** 40 + 123, [7, 1, 457]),
    "o1000": (1000, 7, 1000 * 4 + 990, [1, 7, 8, 9]),
}
ORDER_WIDE = [(m, nc) for m in ORDER_METHODS for nc in (63, 65, 257)]   # on the inputs of "o50", batches 8 and N - 1


def order_inputs(name, method, n_cols=None):
    N, nc, seq0, batches = ORDER_CASES[name]
    if n_cols is not None:
        nc, batches = n_cols, [8, N - 1]
    have = min(seq0, N - 1)
    kinds = ORDER_KINDS + (("ninf_run",) if method in ("median", "zscore-median") else ())
    stream, names = make_stream(sum(name.encode()) * 104729 + nc, N, nc, have, batches, kinds)
    mask = np.array([0 if k == "masked" else 1 for k in names], np.uint8)
    return N, nc, seq0, have, batches, stream, names, mask


def order_case(lib, name, method, clips=(3, 0), n_cols=None):
    N, nc, seq0, have, batches, stream, names, mask = order_inputs(name, method, n_cols)
    worst = 0.0
    for clip in clips:
        label = f"{name} {method} clip={clip} n_cols={nc}"
        want = oracle_rows((name, method, clip, nc), method, clip, N, stream, have, mask)
        dn = make_norm(lib, method, clip, N, nc, mask, seq0, stream[:have])
        got = engine_rows(dn, stream[have:], batches)
        rows = stream[have:]
        np.testing.assert_array_equal(bits(got[:, mask == 0]), bits(rows[:, mask == 0]), err_msg=f"{label}: masked columns")
        if seq0 == 0:
            np.testing.assert_array_equal(bits(got[0]), bits(rows[0]), err_msg=f"{label}: the first row ever")
        worst = max(worst, check_tolerance(got[:, mask == 1], want, label))
        check_state(dn, N, seq0, stream, have, mask)
    return worst


# ---- "power" --------------------------------------------------------------------------------------------------------------
POWER_KINDS = ("n01", "n3_3", "n5_30", "n01_05", "n0_4_round", "skew_pos", "skew_neg", "n01_nan")
# name: (N, n_cols, have, batches -- the last one is the following batch that proves the ring update, clip)
POWER_CASES = {
    "p65_have16": (65, 9, 16, [9, 1, 3], 3),
    "p65_have63": (65, 9, 63, [1, 9, 2], 0),
    "p65_have64_long": (65, 4, 64, [70, 3], 3),
    "p300_have16": (300, 9, 16, [1, 9, 2], 3),
    "p300_have64": (300, 9, 64, [9, 1, 2], 0),
    "p300_have_nm1": (300, 9, 299, [1, 9, 2], 3),
    "p300_long": (300, 2, 63, [305, 2], 3),
    "p65_cols63": (65, 63, 64, [1, 1], 3),
    "p65_cols65": (65, 65, 63, [1, 1], 0),
    "p65_cols257": (65, 257, 64, [1, 1], 3),
}


def power_inputs(name):
    N, n_cols, have, batches, clip = POWER_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 611953 + N)
    L = have + sum(batches)
    names = layout(n_cols, POWER_KINDS)
    x = np.empty((L, n_cols))
    for j, k in enumerate(names):
        g = rng.standard_normal(L)
        s = 1.0 + 0.05 * (j % 11)   # every column its own scale
        if k in ("n01", "n01_nan"):
            col = g * s
            if k == "n01_nan":
                col[rng.random(L) < 0.06] = np.nan
        elif k == "n3_3":
            col = 3 * s + 3 * g
        elif k == "n5_30":
            col = 5 + 30 * s * g
        elif k == "n01_05":
            col = 0.1 + 0.5 * s * g
        elif k == "n0_4_round":
            col = np.round(4 * s * g)
        elif k == "skew_pos":
            col = (np.exp(g) - 1.5) * s      # skewed to the right, both signs
        elif k == "skew_neg":
            col = (1.2 - np.exp(0.5 * g)) * s   # skewed to the left, both signs
        else:   # masked
            col = 100 * g
            col[rng.random(L) < 0.1] = np.nan
        x[:, j] = col
    mask = np.array([0 if k == "masked" else 1 for k in names], np.uint8)
    seq0 = have if have < N - 1 else 2 ** 31 + 5
    return N, n_cols, seq0, have, batches, clip, x.astype(np.float32), names, mask


def power_conditioning(name):
    """orc.yeo_johnson_conditioning(window, x) / (tolerance / 4) of every entry the case compares; computed once."""
    from oracle import nm_oracle as orc

    key = (name, "conditioning")
    if key not in _ORACLE:
        N, n_cols, seq0, have, batches, clip, stream, names, mask = power_inputs(name)
        want = oracle_rows((name, "power", clip), "power", clip, N, stream, have, mask)
        cols = np.nonzero(mask)[0]
        ratio = np.zeros(want.shape)
        for r in range(len(stream) - have):
            lo, hi = window_bounds(N, have, r)
            for u, j in enumerate(cols):
                slack = orc.yeo_johnson_conditioning(np.nan_to_num(stream[lo:hi + 1, j].astype(np.float64)),
                                                     float(stream[hi, j]))
                ratio[r, u] = slack / ((TOL_REL * abs(want[r, u]) + TOL_ABS) / 4)
        _ORACLE[key] = ratio
    return _ORACLE[key]


def power_case(lib, name, device_call=None):
    """The conditioning of EVERY compared entry is asserted on the oracle alone before the engine's output is looked at."""
    N, n_cols, seq0, have, batches, clip, stream, names, mask = power_inputs(name)
    want = oracle_rows((name, "power", clip), "power", clip, N, stream, have, mask)
    ratio = power_conditioning(name)
    r, u = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[r, u] <= 1.0, (f"{name}: probe row {r}, unmasked column {u} is not well conditioned in the oracle itself: "
                                f"slack / (tolerance / 4) = {ratio[r, u]:.3g}")
    dn = make_norm(lib, "power", clip, N, n_cols, mask, seq0, stream[:have])
    call = host_call if device_call is None else (lambda d, rows: padded_call(d, rows, device_call))
    got = engine_rows(dn, stream[have:], batches, call)
    rows = stream[have:]
    np.testing.assert_array_equal(bits(got[:, mask == 0]), bits(rows[:, mask == 0]), err_msg=f"{name}: masked columns")
    worst = check_tolerance(got[:, mask == 1], want, f"{name} power clip={clip}")
    state = dn.export_state()
    assert struct.unpack("<q", state[:8])[0] == seq0 + len(rows)
    ring = np.frombuffer(state[8:], np.float32).reshape(N, -1)
    keep = min(seq0 + len(rows), N - 1)
    qs = np.arange(seq0 + len(rows) - keep, seq0 + len(rows))
    np.testing.assert_array_equal(bits(ring[qs % N]), bits(stream[len(stream) - keep:]))   # (the fit's ring holds every column)
    return worst
