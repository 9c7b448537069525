"""Float64 restatement of ``nolds.hurst_rs(x, fit="poly")`` with every other argument at its default (``nvals=None``,
``corrected=True``, ``unbiased=True``), as recalled for nolds >= 0.6 -- NumPy only.  nolds itself is not installed where
these tests run, so parity is pinned against this restatement, not against nolds (as tests/nolds_oracle.py has it for
``sampen`` and tests/nolds_dfa_oracle.py for ``dfa``).

    N = len(x); nvals = logmid_n(N, ratio=1/4, nsteps=15): l = ln N, mid_k = l (1 - 1/4) 0.5 + (k / 15) (l / 4), k = 0 .. 14,
    nvals = unique(round(exp(mid))) as int32 (round half to even)
    per n: m = N // n chunks of x[: N - N % n]; per chunk d = x - mean, y = cumsum(d), r = max(y) - min(y),
           s = sqrt(sum(d^2) / (n - 1)); chunks with r == 0 are left out; (R/S)_n = mean(r / s), NaN when none is left
    scales with NaN are dropped; y_k = ln (R/S)_n - ln E(n), E = nolds.expected_rs
    H = np.polyfit(ln n, y, 1)[0] + 0.5

With fewer than TWO scales left nolds' fit is under-determined (the minimum-norm solution for one, NaN for none); the device
returns NaN there and ``hurst`` here does the same.  Below five samples the rule leaves fewer than two scales, or the scale
1 among them (whose E is a math.gamma(0) domain error in nolds): ``scales`` raises ValueError.
"""

from __future__ import annotations

import math

import numpy as np


def logmid_n(max_n, ratio, nsteps):
    """nolds.logmid_n"""
    l = np.log(max_n)
    span = l * ratio
    start = l * (1 - ratio) * 0.5
    midrange = start + 1.0 * np.arange(nsteps) / nsteps * span
    return np.unique(np.round(np.exp(midrange)).astype("int32"))


def scales(total_n: int) -> list[int]:
    """nolds.hurst_rs's default ``nvals``; ValueError where the device refuses the window."""
    nvals = [int(n) for n in logmid_n(total_n, 0.25, 15)]
    if len(nvals) < 2 or min(nvals) < 2 or max(nvals) >= total_n:
        raise ValueError(f"hurst_rs of {total_n} samples: nvals {nvals}")
    return nvals


def expected_rs(n: int) -> float:
    """nolds.expected_rs: Anis-Lloyd-Peters, the gamma quotient up to n = 340 and its asymptote above."""
    front = (n - 0.5) / n
    i = np.arange(1, n)
    back = np.sum(np.sqrt((n - i) / i))
    if n <= 340:
        middle = math.gamma((n - 1) * 0.5) / math.sqrt(math.pi) / math.gamma(n * 0.5)
    else:
        middle = 1.0 / math.sqrt(n * math.pi * 0.5)
    return float(front * middle * back)


def rs(x, n: int):
    """nolds.rs(data, n, unbiased=True) -> ((R/S)_n or NaN, chunks kept)"""
    x = np.asarray(x, np.float64)
    total_n = x.size
    m = total_n // n
    seqs = np.reshape(x[:total_n - (total_n % n)], (m, n))
    means = np.mean(seqs, axis=1)
    y = seqs - means.reshape((m, 1))
    walk = np.cumsum(y, axis=1)
    r = np.max(walk, axis=1) - np.min(walk, axis=1)
    s = np.std(seqs, axis=1, ddof=1)
    idx = np.where(r != 0)
    r, s = r[idx], s[idx]
    if len(r) == 0:
        return math.nan, 0
    return float(np.mean(r / s)), int(len(r))


def rs_values(x, nvals=None):
    """-> (R/S)_n float64[S] (NaN where no chunk is kept), kept chunks int[S]"""
    x = np.asarray(x, np.float64)
    nvals = scales(x.size) if nvals is None else list(nvals)
    both = [rs(x, int(n)) for n in nvals]
    return np.array([b[0] for b in both], np.float64), np.array([b[1] for b in both], np.int64)


def slope(nvals, rsvals) -> float:
    """H of the scales that are not NaN; NaN with fewer than two."""
    nvals, rsvals = np.asarray(nvals, np.float64), np.asarray(rsvals, np.float64)
    keep = np.where(~np.isnan(rsvals))[0]
    if len(keep) < 2:
        return math.nan
    xvals = np.log(nvals[keep])
    yvals = np.log(rsvals[keep]) - np.log([expected_rs(int(n)) for n in nvals[keep]])
    return float(np.polyfit(xvals, yvals, 1)[0] + 0.5)


def hurst(x) -> float:
    """nolds.hurst_rs(x, fit="poly") -- NaN instead of the minimum-norm solution when one scale is left."""
    x = np.asarray(x, np.float64)
    nvals = scales(x.size)
    return slope(nvals, rs_values(x, nvals)[0])


def series_value(x) -> float:
    """Nolds.calc_nolds for one series: 0 when its sum is falsy (features/nolds.py:65-76)."""
    x = np.asarray(x, np.float64)
    return hurst(x) if x.sum() else 0


def slope_weights(nvals) -> np.ndarray:
    """w_k = (ln n_k - mean) / sum((ln n_k - mean)^2): d H / d ln (R/S)_{n_k}, the exact sensitivity of the slope."""
    lx = np.log(np.asarray(nvals, np.float64))
    d = lx - lx.mean()
    return d / np.sum(d * d)


def h_limit(nvals) -> float:
    """The tests' absolute limit on H: 1e-5 relative on every (R/S)_n moves its logarithm by 1e-5 and H by at most
    1e-5 sum |w_k| (ln E(n) is a table both sides share); never below 1e-5 itself."""
    return 1e-5 * max(1.0, float(np.sum(np.abs(slope_weights(nvals)))))


def rs_plain_loop(x, n: int):
    """The same (R/S)_n with plain Python loops and no vectorised call: the cross-check of ``rs``."""
    x = [float(v) for v in x]
    total_n = len(x)
    vals = []
    for q in range(total_n // n):
        chunk = x[q * n:(q + 1) * n]
        mean = math.fsum(chunk) / n
        d = [v - mean for v in chunk]
        y, walk = 0.0, []
        for v in d:
            y += v
            walk.append(y)
        r = max(walk) - min(walk)
        if r != 0:
            vals.append(r / math.sqrt(math.fsum(v * v for v in d) / (n - 1)))
    return (math.fsum(vals) / len(vals), len(vals)) if vals else (math.nan, 0)
