"""Float64 restatement of ``nolds.dfa(x, fit_exp="poly")`` with every other argument at its default (order 1, overlapping
chunks, fit_trend "poly"), as recalled for nolds >= 0.6 -- NumPy only.  nolds itself is not installed where these tests
run, so parity is pinned against this restatement, not against nolds (as tests/nolds_oracle.py has it for ``sampen``).

    N = len(x); nvals = logarithmic_n(4, 0.1 N, 1.2) above 70 samples, [4 .. 9] above 10, [N - 2, N - 1] below
    walk = cumsum(x - mean(x))
    per n: chunks walk[i : i + n], i in range(0, N - n, n // 2); a line through each (np.polyfit over t = 0 .. n - 1);
           fluc = sqrt(sum(residual^2) / n) per chunk; F(n) = sum(fluc) / n_chunks
    scales with F(n) == 0 are dropped; none left: NaN; else the slope of np.polyfit(ln n, ln F, 1)

No closed form anywhere: the chunk fits and the final fit are np.polyfit calls.  With exactly ONE scale left nolds' fit is
under-determined and returns the minimum-norm solution; the device returns NaN there and ``dfa`` here does the same.
"""

from __future__ import annotations

import math

import numpy as np


def logarithmic_n(min_n, max_n, factor):
    """nolds.logarithmic_n"""
    assert max_n > min_n and factor > 1
    max_i = int(np.floor(np.log(1.0 * max_n / min_n) / np.log(factor)))
    ns = [min_n]
    for i in range(max_i + 1):
        n = int(np.floor(min_n * (factor ** i)))
        if n > ns[-1]:
            ns.append(n)
    return ns


def scales(total_n: int) -> list[int]:
    """nolds.dfa's default ``nvals`` and the errors it raises on them."""
    if total_n > 70:
        nvals = logarithmic_n(4, 0.1 * total_n, 1.2)
    elif total_n > 10:
        nvals = [4, 5, 6, 7, 8, 9]
    else:
        nvals = [total_n - 2, total_n - 1]
    if len(nvals) < 2:
        raise ValueError("at least two nvals are needed")
    if np.min(nvals) < 2:
        raise ValueError("nvals must be at least two")
    if np.max(nvals) >= total_n:
        raise ValueError("nvals cannot be larger than the input size")
    return [int(n) for n in nvals]


def fluctuations(x, nvals=None) -> np.ndarray:
    """F(n) for every scale of ``nvals`` (default: the rule), float64."""
    x = np.asarray(x, np.float64)
    N = x.size
    nvals = scales(N) if nvals is None else list(nvals)
    walk = np.cumsum(x - np.mean(x))
    out = []
    for n in nvals:
        d = np.array([walk[i:i + n] for i in range(0, N - n, n // 2)])   # [n_chunks, n]
        t = np.arange(n)
        tpoly = np.polyfit(t, d.T, 1)                                     # [2, n_chunks]: one fit per chunk, vectorised
        trend = np.outer(tpoly[0], t) + tpoly[1][:, None]                 # np.polyval of every chunk's line
        flucs = np.sqrt(np.sum((d - trend) ** 2, axis=1) / n)
        out.append(np.sum(flucs) / len(flucs))
    return np.array(out, np.float64)


def slope(nvals, F) -> float:
    """The final fit over the scales with F != 0; NaN with fewer than two."""
    nvals, F = np.asarray(nvals, np.float64), np.asarray(F, np.float64)
    keep = np.where(F != 0)[0]
    if len(keep) < 2:
        return math.nan
    return float(np.polyfit(np.log(nvals[keep]), np.log(F[keep]), 1)[0])


def dfa(x) -> float:
    """nolds.dfa(x, fit_exp="poly") -- NaN instead of the minimum-norm solution when one scale is left."""
    x = np.asarray(x, np.float64)
    nvals = scales(x.size)
    return slope(nvals, fluctuations(x, nvals))


def series_value(x) -> float:
    """Nolds.calc_nolds for one series: 0 when its sum is falsy (features/nolds.py:65-76)."""
    x = np.asarray(x, np.float64)
    return dfa(x) if x.sum() else 0


def slope_weights(nvals) -> np.ndarray:
    """w_k = (ln n_k - mean) / sum((ln n_k - mean)^2): d alpha / d ln F(n_k), the exact sensitivity of the slope."""
    lx = np.log(np.asarray(nvals, np.float64))
    d = lx - lx.mean()
    return d / np.sum(d * d)


def alpha_limit(nvals) -> float:
    """The tests' absolute limit on alpha: 1e-5 relative on every F(n) moves ln F by 1e-5 and alpha by at most
    1e-5 sum |w_k|; never below 1e-5 itself."""
    return 1e-5 * max(1.0, float(np.sum(np.abs(slope_weights(nvals)))))
