"""Float64 restatement of the reference's coherence feature (features/coherence.py) -- NumPy only.

``spectra`` is scipy.signal.welch / csd as CoherenceObject.get_coh calls them (periodic Hann, noverlap = nperseg // 2,
constant detrend, nperseg clamped to the window; every scale factor cancels in coh / icoh, so plain segment means are
kept).  ``pair_features`` builds the reference's keys and values for one pair; ``bound`` the per-entry conditioning the
GPU tests accept on top of 1e-5: an fp32 transform rounds relative to the segment's energy, so a bin whose power is far
below it carries a relative error of about eps * sqrt(energy / power).
"""

from __future__ import annotations

import numpy as np

EPS_EFF = 1e-6   # per-sample rounding of the fp32 pipeline (input cast, pre-processing, transform), a few fp32 ulps


def spectra(x: np.ndarray, y: np.ndarray, sfreq: float, nperseg: int):
    """-> f, Sxx, Syy, Sxy (segment means, unscaled), Ex, Ey (mean windowed segment energies)."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    W = x.shape[-1]
    n = min(int(nperseg), W)
    step = n - n // 2
    nseg = (W - n) // step + 1
    idx = np.arange(nseg)[:, None] * step + np.arange(n)[None, :]
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)
    xs = x[idx]
    ys = y[idx]
    xs = (xs - xs.mean(-1, keepdims=True)) * win
    ys = (ys - ys.mean(-1, keepdims=True)) * win
    X = np.fft.rfft(xs, axis=-1)
    Y = np.fft.rfft(ys, axis=-1)
    Sxx = (np.abs(X) ** 2).mean(0)
    Syy = (np.abs(Y) ** 2).mean(0)
    Sxy = (np.conj(X) * Y).mean(0)
    f = np.fft.rfftfreq(n, 1 / sfreq)
    return f, Sxx, Syy, Sxy, float((xs ** 2).sum(-1).mean()), float((ys ** 2).sum(-1).mean())


def coh_icoh(x, y, sfreq, nperseg):
    """-> f, coh, icoh, per-bin bound (float64)."""
    f, Sxx, Syy, Sxy, Ex, Ey = spectra(x, y, sfreq, nperseg)
    with np.errstate(divide="ignore", invalid="ignore"):
        coh = np.abs(Sxy) ** 2 / (Sxx * Syy)
        icoh = Sxy.imag / np.sqrt(Sxx * Syy)
        rx = EPS_EFF * np.sqrt(Ex / Sxx)
        ry = EPS_EFF * np.sqrt(Ey / Syy)
    bnd = 4.0 * (rx + ry)
    bnd = np.where(np.isfinite(bnd), bnd, np.inf)
    return f, coh, icoh, bnd


def pair_features(x, y, sfreq, nperseg, ranges: dict, band_names, c1: str, c2: str, feats=None, methods=None,
                  with_bound: bool = False):
    """The reference's dict for one pair (CoherenceObject.get_coh); with_bound -> (values, bounds, ties) where
    ties[key] is True for a max_allfbands entry whose float64 maximum is not unique within the bound."""
    feats = list(feats or ["mean_fband", "max_fband", "max_allfbands"])
    methods = list(methods or ["coh", "icoh"])
    f, coh, icoh, bnd = coh_icoh(x, y, sfreq, nperseg)
    vals, bounds, alts = {}, {}, {}
    for m in (["coh"] + (["icoh"] if "icoh" in methods else [])):
        v = coh if m == "coh" else icoh
        for name in band_names:
            lo, hi = ranges[name]
            sel = (f > lo) & (f < hi)
            if "mean_fband" in feats:
                k = f"{m}_{c1}_to_{c2}_mean_fband_{name}"
                vals[k] = float(np.mean(v[sel])) if sel.any() else np.nan
                bounds[k] = float(np.mean(bnd[sel])) if sel.any() else 0.0
            if "max_fband" in feats:
                k = f"{m}_{c1}_to_{c2}_max_fband_{name}"
                vals[k] = float(np.max(v[sel]))
                bounds[k] = float(np.max(bnd[sel]))
        if "max_allfbands" in feats:
            k = f"{m}_{c1}_to_{c2}_max_allfbands_{band_names[-1]}"
            i = int(np.argmax(v))
            vals[k] = float(f[i])
            bounds[k] = 0.0
            # the frequencies a fp32 run may pick: bins within the bound of the float64 maximum
            if np.isnan(v[i]):
                alts[k] = {float(f[i])}
            else:
                alts[k] = {float(f[j]) for j in range(len(v)) if v[i] - v[j] <= bnd[i] + bnd[j] + 1e-5}
    if with_bound:
        return vals, bounds, alts
    return vals


def resolve(ch_names, name: str) -> int:
    return next(i for i, ch in enumerate(ch_names) if ch.startswith(name))


def features(data, ch_names, sfreq, cs, ranges, with_bound: bool = False):
    """Coherence.calc_feature(data) of the reference (coherence_settings ``cs`` as a dict)."""
    out, bounds, alts = {}, {}, {}
    feats = [k for k, v in cs["features"].items() if v]
    methods = [k for k, v in cs["method"].items() if v]
    bands = [b.replace(" ", "_") for b in cs["frequency_bands"]]
    for c1, c2 in cs["channels"]:
        r = pair_features(data[resolve(ch_names, c1)], data[resolve(ch_names, c2)], sfreq, cs["nperseg"], ranges,
                          bands, c1, c2, feats, methods, with_bound=True)
        for k in r[0]:
            if k not in out:
                out[k], bounds[k] = r[0][k], r[1][k]
                if k in r[2]:
                    alts[k] = r[2][k]
    return (out, bounds, alts) if with_bound else out


def compare(got: dict, want: dict, bounds: dict, alts: dict, atol: float = 1e-5):
    """-> (misses, accepted): entries outside 1e-5 + bound; entries outside 1e-5 but inside the bound, or a
    max_allfbands tie resolved to another bin inside the bound."""
    misses, accepted = [], []
    for k, w in want.items():
        g = float(got[k])
        if "max_allfbands" in k:
            if np.float32(w) == np.float32(g):
                continue
            if any(np.float32(a) == np.float32(g) for a in alts.get(k, ())):
                accepted.append(k)
            else:
                misses.append((k, g, w))
            continue
        if np.isnan(w) or np.isnan(g):
            if not (np.isnan(w) and np.isnan(g)):
                misses.append((k, g, w))
            continue
        err = abs(g - w)
        if err <= atol:
            continue
        if err <= atol + bounds.get(k, 0.0):
            accepted.append(k)
        else:
            misses.append((k, g, w))
    return misses, accepted
