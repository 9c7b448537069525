"""Float64 restatement of the reference's nolds feature (features/nolds.py) restricted to sample entropy -- NumPy only.

``sampen`` is nolds.sampen with its defaults (emb_dim = 2, lag = 1, Chebyshev distance, open comparison) as recalled for
nolds >= 0.6.1, which the reference requires; nolds itself is not installed where these tests run, so parity is pinned
against this restatement, not against nolds:

    N = len(x), tol = std(x, ddof = 1) * 0.1164 * (0.5627 ln 2 + 1.3334)
    templates i = 0 .. N - 3 (the same T = N - 2 rows for both lengths)
    B = #{i < j : max(|x_i - x_j|, |x_{i+1} - x_{j+1}|) < tol},  A = ... and |x_{i+2} - x_{j+2}| < tol
    -ln(A / B); NaN when both counts are zero; +inf when only A is.

``nolds_features`` is the feature wrapper: nan_to_num, the band-index quirk (the band at position i of nolds' own list
reads series i of the bank over ALL frequency_ranges_hz), the sum rule (0 when series.sum() is falsy) and the key order.

``conditioning`` is the report the device tests accept entries on: on the float32 series the kernel itself read, the
pairs whose distance lies within delta = 2^-23 (|d| + tol) (+ an absolute term for series that went through an fp32 FIR)
of tol could fall either way in float32; from them the intervals [A-, A+] x [B-, B+] and the interval of the result.
"""

from __future__ import annotations

import math

import numpy as np

TOL_FACTOR = 0.1164 * (0.5627 * math.log(2.0) + 1.3334)
DDOF = 1
EPS32 = 2.0 ** -23


def tolerance(x) -> float:
    x = np.asarray(x, np.float64)
    if x.size - DDOF <= 0:
        return float("nan")
    return float(np.std(x, ddof=DDOF) * TOL_FACTOR)


def _diagonals(x, tol, delta_abs=0.0, report=False):
    """Walks j - i = k.  -> (A, B) or, with report, (A-, A+, B-, B+, A, B): the counts with every pair within delta of
    tol taken as outside / inside."""
    x = np.asarray(x, np.float64)
    N = x.size
    T = N - 2
    A = B = 0
    a_lo = a_hi = b_lo = b_hi = 0
    if T < 2 or not tol == tol:
        return (0, 0, 0, 0, 0, 0) if report else (0, 0)
    for k in range(1, T):
        d = np.abs(x[: N - k] - x[k:])          # d[m] = |x_m - x_{m+k}|, m = 0 .. N - 1 - k
        n = T - k
        m2 = np.maximum(d[:n], d[1:n + 1])
        m3 = np.maximum(m2, d[2:n + 2])
        B += int(np.count_nonzero(m2 < tol))
        A += int(np.count_nonzero(m3 < tol))
        if report:
            # float32 rounding of a difference and of tol: a distance within delta of tol is undecided
            dl2 = EPS32 * (m2 + tol) + delta_abs
            dl3 = EPS32 * (m3 + tol) + delta_abs
            b_lo += int(np.count_nonzero(m2 < tol - dl2))
            b_hi += int(np.count_nonzero(m2 < tol + dl2))
            a_lo += int(np.count_nonzero(m3 < tol - dl3))
            a_hi += int(np.count_nonzero(m3 < tol + dl3))
    return (a_lo, a_hi, b_lo, b_hi, A, B) if report else (A, B)


def counts(x, tol=None):
    """(A, B) of the series in float64."""
    x = np.asarray(x, np.float64)
    return _diagonals(x, tolerance(x) if tol is None else tol)


def counts_small_integers(x, tol=None):
    """(A, B) of an INTEGER-valued series by counting template types instead of pairs -- O(N + types^2), for series too
    long for the diagonal walk to stay within seconds (40 000 samples).  Equal to ``counts`` (tests check it)."""
    x = np.asarray(x, np.float64)
    xi = np.rint(x).astype(np.int64)
    assert np.array_equal(xi, x), "integer-valued series only"
    tol = tolerance(x) if tol is None else tol
    T = x.size - 2
    if T < 2 or not tol == tol:
        return 0, 0
    trip = np.stack([xi[:T], xi[1:T + 1], xi[2:T + 2]], axis=1)
    types, cnt = np.unique(trip, axis=0, return_counts=True)
    cnt = cnt.astype(np.int64)
    d = np.abs(types[:, None, :] - types[None, :, :]).astype(np.float64)
    in2 = np.maximum(d[..., 0], d[..., 1]) < tol
    in3 = in2 & (d[..., 2] < tol)
    cross = np.triu(np.outer(cnt, cnt), 1)   # pairs of two different types
    same = cnt * (cnt - 1) // 2              # pairs inside one type

    def pairs(inside):
        return int(cross[inside].sum() + same[np.diag(inside)].sum())

    return pairs(in3), pairs(in2)


def value(A: int, B: int) -> float:
    if A > 0 and B > 0:
        return -math.log(A / B)
    if B > 0:
        return math.inf
    return math.nan


def sampen(x) -> float:
    """nolds.sampen(x) with its defaults."""
    return value(*counts(x))


def series_value(x) -> float:
    """Nolds.calc_nolds for one series: 0 when its sum is falsy (nolds.py:76-80)."""
    x = np.asarray(x, np.float64)
    return sampen(x) if x.sum() else 0


def nolds_features(data, ch_names, ranges: dict, nolds_bands, raw: bool, filter_bank=None) -> dict:
    """The reference's dict for one window data[C, W].  ``filter_bank(data) -> [C, n_global_bands, W]`` is the bank over
    ALL of ``ranges`` (BandPower's MNEFilter); band i of ``nolds_bands`` reads its series i -- the reference's quirk."""
    data = np.nan_to_num(np.asarray(data, np.float64))
    out = {}
    if raw:
        for c, ch in enumerate(ch_names):
            out[f"{ch}_nolds_sample_entropy_raw"] = series_value(data[c])
    if len(nolds_bands) > 0:
        for fb in nolds_bands:
            assert fb in ranges, f"{fb} selected in nolds_features, but not defined in s['frequency_ranges_hz']"
        filt = filter_bank(data)
        for i, fb in enumerate(nolds_bands):
            for c, ch in enumerate(ch_names):
                out[f"{ch}_nolds_sample_entropy_{fb}"] = series_value(filt[c, i])
    return out


def conditioning(x32, delta_abs: float = 0.0) -> dict:
    """On the float32 series the kernel read: tol as the kernel forms it (float64 statistics, rounded once to float32),
    the float64 counts at that tol, the number of undecided pairs and the interval of the result."""
    x = np.asarray(x32, np.float32).astype(np.float64)
    tol = float(np.float32(tolerance(x)))
    a_lo, a_hi, b_lo, b_hi, A, B = _diagonals(x, tol, delta_abs, report=True)
    zero = bool(x.sum() == 0.0)
    amb = (a_hi - a_lo) + (b_hi - b_lo)
    if zero:
        lo = hi = 0.0
    elif amb == 0:
        lo = hi = value(A, B)
    else:
        # -ln(A / B) falls with A and rises with B (A <= B); a corner with a zero count is +inf or NaN
        cand = [value(a, b) for a in (a_lo, a_hi) for b in (b_lo, b_hi) if a <= b]
        fin = [v for v in cand if v == v]
        lo, hi = (min(fin), max(fin)) if len(fin) == len(cand) else (-math.inf, math.inf)
    return {"tol": tol, "A": A, "B": B, "A_lo": a_lo, "A_hi": a_hi, "B_lo": b_lo, "B_hi": b_hi, "ambiguous": amb,
            "zero": zero, "lo": lo, "hi": hi, "value": 0.0 if zero else value(A, B)}
