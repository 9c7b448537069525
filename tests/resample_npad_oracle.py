"""``mne.filter.resample`` restated in float64 WITH THE FUNCTION'S OWN SIGNATURE: ``npad=100`` by default.

The reference calls ``mne.filter.resample(data.astype(np.float64), up=ratio, down=1.0)`` and nothing else
(processing/resample.py:58-60), so it gets the function's defaults: ``npad=100``, boxcar window, ``reflect_limited``
padding, the FFT method.  ``oracle.mne_restated.resample`` restates the same steps with ``npad="auto"`` (the default of
``Raw.resample``); this module restates both, and tests/test_resample_npad_cpu.py ties it

  * with ``npad="auto"`` to ``oracle.mne_restated.resample``, and
  * with a fixed pad to the independent form ``scipy.signal.resample(padded, n_new) * (ratio / (n_new / n_pad))``, cropped,

at 1e-12 of the row's scale.  MNE itself is absent: PARITY UNPINNED against it, for either mode.

The lengths (``round`` is Python's round-half-even):
    npad_l = npad_r = npad              n_pad = W + 2 npad              n_new = max(round(ratio n_pad), 1)
    final_len = round(ratio W)          crop_l = round(ratio npad)      crop_r = n_new - final_len - crop_l
"""

from __future__ import annotations

import numpy as np


def lengths(W: int, ratio: float, npad=100) -> dict:
    """The lengths of one call: W raw samples, ``npad`` = "auto" or samples per side."""
    W, ratio = int(W), float(ratio)
    if isinstance(npad, str):
        if npad != "auto":
            raise ValueError(f"npad must be 'auto' or an int >= 0, not {npad!r}")
        n_pad = 2 ** int(np.ceil(np.log2(W + min(W // 8, 100) * 2)))
        pad_l = (n_pad - W) // 2
        pad_r = n_pad - W - pad_l
    else:
        if isinstance(npad, bool) or int(npad) != npad or npad < 0:
            raise ValueError(f"npad must be 'auto' or an int >= 0, not {npad!r}")
        pad_l = pad_r = int(npad)
        n_pad = W + 2 * int(npad)
    n_new = max(int(round(ratio * n_pad)), 1)
    final_len = int(round(ratio * W))
    crop_l = int(round(ratio * pad_l))
    return dict(W=W, ratio=ratio, n_pad=n_pad, pad_l=pad_l, pad_r=pad_r, n_new=n_new, W_new=final_len, crop_l=crop_l,
                crop_r=n_new - final_len - crop_l)


def pad_reflect_limited(x: np.ndarray, pad_l: int, pad_r: int) -> np.ndarray:
    """Rows [.., W] -> [.., pad_l + W + pad_r]: the odd reflection about both ends, at most W - 1 samples of it, zeros beyond."""
    x = np.asarray(x)
    W = x.shape[-1]
    lead = x.shape[:-1]
    z_l = np.zeros(lead + (max(pad_l - W + 1, 0),), x.dtype)
    z_r = np.zeros(lead + (max(pad_r - W + 1, 0),), x.dtype)
    two = x.dtype.type(2)
    return np.concatenate([z_l, two * x[..., :1] - x[..., pad_l:0:-1], x,
                           two * x[..., -1:] - x[..., -2:-pad_r - 2:-1], z_r], axis=-1)


def resample(x, up=1.0, down=1.0, *, axis=-1, window="auto", n_jobs=None, pad="auto", npad=100, method="fft", verbose=None):
    """``mne.filter.resample``: the FFT method, boxcar window, ``reflect_limited`` padding, along the last axis."""
    from scipy.fft import irfft, rfft

    if axis != -1 or method != "fft" or window not in ("auto", "boxcar") or pad not in ("auto", "reflect_limited"):
        raise NotImplementedError("restated: axis=-1, method='fft', the boxcar window and reflect_limited padding only")
    x = np.asarray(x, dtype=np.float64)
    ratio = float(up) / float(down)
    if ratio == 1.0:
        return x.copy()
    L = lengths(x.shape[-1], ratio, npad)
    n_pad, n_new = L["n_pad"], L["n_new"]
    X = rfft(pad_reflect_limited(x, L["pad_l"], L["pad_r"]), axis=-1)
    assert X.shape[-1] == n_pad // 2 + 1
    # MNE _fft_resample: the Nyquist bin of the shorter length is doubled (down-sampling) or halved (up-sampling)
    use_len = min(n_new, n_pad)
    if use_len % 2 == 0:
        X[..., use_len // 2] *= 2.0 if n_new < n_pad else 0.5
    y = irfft(X, n=n_new, axis=-1) * ratio   # (irfft truncates / zero-extends the spectrum)
    return y[..., L["crop_l"]:L["crop_l"] + L["W_new"]]
