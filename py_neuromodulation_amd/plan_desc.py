"""Settings + channel names -> the flat plan description (``nmx_plan_desc``) and the key list.  Pure NumPy / ctypes
structs: no library, no device -- which is all ``HotPathEngine(dry_run=True)`` is.

Key order reproduced: features in ``FeatureSelector`` field order
(stream/settings.py:41-55 via utils/types.py:135-140), and inside each feature the nesting of
the reference class (hjorth_raw.py:37-40, bandpower.py:131-145, oscillatory.py:102-117,
sharpwaves.py:169-197,302-326, bursts.py:119-125,262-298, linelength.py:17-19).
"""

from __future__ import annotations

import ctypes as C
import math
import os
import re
from collections.abc import Mapping

import numpy as np

from . import _lib, fir_design
from ._lib import Cols, PlanDesc
from .settings import validation_error

_FEATURE_BITS = {"raw_hjorth": _lib.F_HJORTH, "return_raw": _lib.F_RAW,
                 "bandpass_filter": _lib.F_BANDPOWER, "stft": _lib.F_STFT, "fft": _lib.F_FFT,
                 "welch": _lib.F_WELCH, "sharpwave_analysis": _lib.F_SHARPWAVE,
                 "bursts": _lib.F_BURSTS, "linelength": _lib.F_LINELENGTH, "coherence": _lib.F_COHERENCE,
                 "nolds": _lib.F_NOLDS}
_OUT_OF_SCOPE = {"fooof", "mne_connectivity", "bispectrum"}
# nolds.sampen's default tolerance, as recalled for nolds >= 0.6.1 (it is not installed here: parity unpinned against
# nolds itself): tol = std(x, ddof = 1) * 0.1164 * (0.5627 * ln(emb_dim) + 1.3334) with emb_dim = 2.  Formed here and
# passed in the plan description -- the kernel (nmx_k_nolds.h) bakes in neither.
NOLDS_TOL_FACTOR = 0.1164 * (0.5627 * float(np.log(2.0)) + 1.3334)
NOLDS_DDOF = 1
NOLDS_MAX_SAMPLES = 40000   # nmx_k_nolds.h: a series sits in the CU's LDS
# nolds.dfa's default scale rule, as recalled for nolds >= 0.6 (not installed here either: parity with nolds itself is
# unpinned, as for NOLDS_TOL_FACTOR): logarithmic_n(4, 0.1 N, 1.2) above 70 samples.  `dfa_scales` forms the table here
# and the plan description carries it -- the kernel bakes in neither the table nor the rule.
NOLDS_DFA_MIN_SCALE, NOLDS_DFA_MAX_SHARE, NOLDS_DFA_FACTOR = 4, 0.1, 1.2
NOLDS_DFA_MAX_SCALES = 64   # nmx_k_nolds.h: NMX_NOLDS_DFA_MAX_SCALES
# nolds.hurst_rs's default scale rule, recalled likewise: logmid_n(N, ratio = 1/4, nsteps = 15); its expected R/S switches
# from the gamma quotient to the asymptote above n = 340.  `hurst_scales` / `hurst_expected_rs` form both tables here.
NOLDS_HURST_RATIO, NOLDS_HURST_STEPS, NOLDS_HURST_GAMMA_MAX = 0.25, 15, 340
NOLDS_HURST_MAX_SCALES = 15   # nmx_k_nolds.h: NMX_NOLDS_HURST_MAX_SCALES
COH_MAX_NPERSEG = 4096   # nmx_k_coh.h: segment length bound of the coherence kernel, at every window (above 16 384 samples too: NMX_LONG_COHERENCE)
_BURST_SLOTS = [("duration", ["duration_mean", "duration_max"]),
                ("amplitude", ["amplitude_mean", "amplitude_max"]),
                ("burst_rate_per_s", ["burst_rate_per_s"]), ("in_burst", ["in_burst"])]


def _enabled(sel) -> list[str]:
    return list(sel.get_enabled())


def _cols(base=0, ch=0, a=0, b=0) -> Cols:
    return Cols(int(base), int(ch), int(a), int(b))


def resample_npad_arg(value=None):
    """The resampler's padding mode as the keyword ``resample_npad`` (``npad`` of ``processing.Resampler``) states it:
    ``"auto"`` (the default: the next power of two, what ``Raw.resample`` defaults to) or an ``int >= 0``, that many samples
    per side (100: the default of ``mne.filter.resample`` itself, which the reference's call gets).  ``None``: the
    environment variable NMX_RESAMPLE_NPAD (``auto`` or an integer), ``"auto"`` without it.  Anything else: ValueError."""
    if value is None:
        text = os.environ.get("NMX_RESAMPLE_NPAD", "").strip()
        if text == "" or text == "auto":
            return "auto"
        if not re.fullmatch(r"\+?[0-9]+", text):
            raise ValueError(f"NMX_RESAMPLE_NPAD must be 'auto' or an integer >= 0, not {text!r}")
        value = int(text)
    if isinstance(value, str):
        if value == "auto":
            return "auto"
        raise ValueError(f"resample_npad must be 'auto' or an int >= 0, not {value!r}")
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < 0:
        raise ValueError(f"resample_npad must be 'auto' or an int >= 0, not {value!r}")
    return int(value)


def nolds_fit_arg(value=None):
    """The final line fit of the nolds measures as the keyword ``nolds_fit`` states it.

    * ``None`` (the default: the reference's, ``fit="RANSAC"``, which has no kernel -- every measure that ends in it
      raises) and ``"RANSAC"`` (the same, said aloud);
    * ``"poly"``: shorthand for ``{"detrended_fluctuation_analysis": "poly"}`` AND NOTHING MORE -- least squares for
      ``nolds.dfa(x, fit_exp="poly")``, which then runs on the device; the other measures keep raising;
    * a mapping ``{measure name: "poly" | "RANSAC" | None}`` over the five names of ``NoldsFeatures``, one entry per
      measure: ``{"hurst_exponent": "poly", "detrended_fluctuation_analysis": "poly"}`` lets ``nolds.hurst_rs(x,
      fit="poly")`` and ``nolds.dfa(x, fit_exp="poly")`` run.  ``"poly"`` for correlation_dimension and lyapunov_exponent
      parses, but they have no kernel and keep raising; sample_entropy has no line fit and needs no entry.

    ``None`` reads the environment variable NMX_NOLDS_FIT: ``poly``, ``RANSAC``, or the mapping as
    ``hurst_exponent:poly,detrended_fluctuation_analysis:poly``.  Anything else: ValueError naming the keyword or the
    variable.  -> None, "poly", or the mapping as a dict in measure order (a value given again comes back unchanged)."""
    name = "nolds_fit"
    if value is None:
        value = os.environ.get("NMX_NOLDS_FIT", "").strip()
        name = "NMX_NOLDS_FIT"
        if value == "":
            return None
        if ":" in value:
            pairs = [item.split(":") for item in value.split(",")]
            if any(len(kv) != 2 for kv in pairs) or len({kv[0].strip() for kv in pairs}) != len(pairs):
                raise ValueError(f"{name} must be 'poly', 'RANSAC' or '<measure>:<fit>,...', not {value!r}")
            value = {k.strip(): v.strip() for k, v in pairs}
    if isinstance(value, str) and value == "poly":
        return "poly"
    if isinstance(value, str) and value == "RANSAC":
        return None
    if isinstance(value, Mapping):
        for k, v in value.items():
            if not isinstance(k, str) or k not in _lib.NOLDS_MEASURES:
                raise ValueError(f"{name}: {k!r} is not a nolds measure (one of {_lib.NOLDS_MEASURES})")
            if not (v is None and name == "nolds_fit") and not (isinstance(v, str) and v in ("poly", "RANSAC")):
                raise ValueError(f"{name}: the fit of {k} must be 'poly' or 'RANSAC'"
                                 f"{' (or None)' if name == 'nolds_fit' else ''}, not {v!r}")
        return {k: value[k] for k in _lib.NOLDS_MEASURES if k in value}
    raise ValueError(f"{name} must be 'poly' or 'RANSAC' (or unset), or a mapping of measure names to them, not {value!r}")


def nolds_poly_measures(fit) -> tuple:
    """The measures whose final fit is least squares under ``fit``, a value ``nolds_fit_arg`` returned."""
    if fit == "poly":
        return ("detrended_fluctuation_analysis",)
    if isinstance(fit, Mapping):
        return tuple(k for k in _lib.NOLDS_MEASURES if fit.get(k) == "poly")
    return ()


def dfa_scales(n_samples: int) -> list[int]:
    """The chunk lengths ``nolds.dfa`` chooses for a series of ``n_samples`` (its default ``nvals``), and its errors."""
    N = int(n_samples)
    if N > 70:
        lo, hi, f = NOLDS_DFA_MIN_SCALE, NOLDS_DFA_MAX_SHARE * N, NOLDS_DFA_FACTOR
        nvals = [lo]   # nolds.logarithmic_n
        for i in range(int(np.floor(np.log(1.0 * hi / lo) / np.log(f))) + 1):
            n = int(np.floor(lo * (f ** i)))
            if n > nvals[-1]:
                nvals.append(n)
    elif N > 10:
        nvals = [4, 5, 6, 7, 8, 9]
    else:
        nvals = [N - 2, N - 1]
    if len(nvals) < 2:
        raise ValueError("at least two nvals are needed")
    if min(nvals) < 2:
        raise ValueError(f"nvals must be at least two (detrended_fluctuation_analysis of a {N}-sample series)")
    if max(nvals) >= N:
        raise ValueError("nvals cannot be larger than the input size")
    return nvals


def hurst_scales(n_samples: int) -> list[int]:
    """The chunk lengths ``nolds.hurst_rs`` chooses for a series of ``n_samples`` (its default ``nvals``):
    ``logmid_n(N, ratio=1/4, nsteps=15)`` -- 15 logarithmically spaced values over the middle quarter of [ln 1, ln N],
    rounded half to even and made unique; never more than 15.  Below five samples fewer than two scales are left, or the
    scale 1 among them (whose expected R/S is a gamma(0) domain error in nolds): ValueError."""
    N = int(n_samples)
    if N < 1:
        raise ValueError(f"nolds: hurst_exponent of a {N}-sample series")
    ln = np.log(N)
    mid = ln * (1.0 - NOLDS_HURST_RATIO) * 0.5 + np.arange(NOLDS_HURST_STEPS) * (1.0 / NOLDS_HURST_STEPS) * ln * NOLDS_HURST_RATIO
    nvals = [int(n) for n in np.unique(np.round(np.exp(mid)).astype("int32"))]
    if len(nvals) < 2 or min(nvals) < 2 or max(nvals) >= N:
        raise ValueError(f"nolds: hurst_exponent needs at least two chunk lengths 2 <= n < N; a {N}-sample series gives "
                         f"{nvals} (windows below 5 samples are not supported)")
    return nvals


def hurst_expected_rs(n: int) -> float:
    """nolds.expected_rs(n): the Anis-Lloyd-Peters expectation of (R/S)_n of white noise -- the exact gamma quotient up to
    n = 340 and its asymptote above (nolds' own switch; the two do not meet: E(340) = 21.9607..., E(341) = 21.9462...)."""
    n = int(n)
    if n < 2:
        raise ValueError(f"nolds: the expected R/S of chunk length {n} is undefined")
    i = np.arange(1, n, dtype=np.float64)
    back = float(np.sum(np.sqrt((n - i) / i)))
    if n <= NOLDS_HURST_GAMMA_MAX:
        middle = math.gamma((n - 1) * 0.5) / math.sqrt(math.pi) / math.gamma(n * 0.5)
    else:
        middle = 1.0 / math.sqrt(n * math.pi * 0.5)
    return (n - 0.5) / n * middle * back


class PlanBuilder:
    """The window geometry of one plan (``W`` samples the features see, ``W_in`` incoming, ``resample_ratio``), then
    ``build`` -> (PlanDesc, keys, coh_pairs, filter_taps, the arrays the struct points into).  HotPathEngine's arguments."""

    def __init__(self, settings, ch_names, sfreq, features=None, window=None, resample_from=None, raw_window=None,
                 resample_to=None, pre_taps=None, raw_norm=None, resample_npad=None, nolds_fit=None) -> None:
        self.settings = settings
        self.resample_npad = resample_npad_arg(resample_npad)
        # None, "poly" (detrended_fluctuation_analysis runs) or a mapping measure -> fit (keyword, else NMX_NOLDS_FIT)
        self.nolds_fit = nolds_fit_arg(nolds_fit)
        self.ch_names = list(ch_names)
        self.sfreq = float(sfreq)
        self.C = len(self.ch_names)
        enabled = _enabled(settings.features) if features is None else list(features)
        bad = [f for f in enabled if f in _OUT_OF_SCOPE or f not in _FEATURE_BITS]
        if bad:
            raise NotImplementedError(
                f"features {bad} are outside the accelerated hot path (SURVEY.md section 2)")
        self.enabled = enabled
        # window samples as the generator cuts them (stream/generator.py:34-53)
        self.W = int(window) if window is not None else int(settings.segment_length_features_ms / 1000 * sfreq)
        self.W_in, self.resample_ratio = self.W, 0.0
        target = self.sfreq if resample_to is None else float(resample_to)
        if resample_from is not None and float(resample_from) != target:
            self.resample_ratio = target / float(resample_from)
            self.W_in = (int(raw_window) if raw_window is not None
                         else int(settings.segment_length_features_ms / 1000 * float(resample_from)))
            if window is None:
                self.W = int(round(self.resample_ratio * self.W_in))   # mne.filter.resample: final_len
        self._keep: list = []   # arrays referenced by the C struct
        self._raw_norm = raw_norm   # (method "mean" | "zscore", clip, N samples, add samples)
        self._pre_taps = [np.asarray(t, dtype=np.float64) for t in (pre_taps or [])]
        if len(self._pre_taps) > 4:
            raise ValueError("at most 4 preprocessing_filter stages")
        self.keys: list[str] = []
        self.coh_pairs: list[tuple[int, int]] = []   # coherence: (seed, target) channel indices of the emitted pairs

    def _dptr(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        self._keep.append(arr)
        return arr.ctypes.data_as(C.POINTER(C.c_double))

    def _osc(self, osc_settings, name: str, n: int, freqs: np.ndarray, inclusive: bool,
             bands, base: int) -> tuple[_lib.OscDesc, int]:
        s = osc_settings
        if not s.windowlength_ms <= self.settings.segment_length_features_ms:
            raise AssertionError(
                f"oscillatory feature windowlength_ms = ({s.windowlength_ms}) needs to be smaller "
                f"than settings['segment_length_features_ms'] = "
                f"{self.settings.segment_length_features_ms}")
        o = _lib.OscDesc()
        # a segment longer than the window shrinks to it: x[:, -N:] (oscillatory.py:95) and the nperseg
        # clamp of scipy.signal.welch / stft; the band bins keep the grid of the NOMINAL length
        n_eff = min(int(n), self.W)
        o.n = n_eff
        o.log_transform = int(bool(s.log_transform))
        ests = _enabled(s.features)
        o.estimators = sum(_lib.EST_BITS[e] for e in ests)
        o.return_spectrum = int(bool(s.return_spectrum))
        for b, (_, (lo, hi)) in enumerate(bands):
            idx = np.where((freqs >= lo) & ((freqs <= hi) if inclusive else (freqs < hi)))[0]
            if idx.size and not np.array_equal(idx, np.arange(idx[0], idx[-1] + 1)):
                raise ValueError("non-contiguous band bins")
            if not idx.size and "max" in ests:   # np.max over an empty band (oscillatory.py:170)
                raise ValueError("zero-size array to reduction operation maximum which has no identity "
                                 f"({name}: band {bands[b][0]} holds no bin of the {len(freqs)}-bin grid)")
            o.bin_lo[b] = int(idx[0]) if idx.size else 0
            o.bin_hi[b] = int(idx[-1]) + 1 if idx.size else 0
            if o.bin_hi[b] > n_eff // 2 + 1:
                raise IndexError(f"{name}: band {bands[b][0]} reads bin {o.bin_hi[b] - 1} of a spectrum with "
                                 f"{n_eff // 2 + 1} bins (window shorter than the nominal segment)")
        # keys: band, estimator, channel  (oscillatory.py:102-112)
        o.cols = _cols(base, 1, len(ests) * self.C, self.C)
        for bname, _ in bands:
            for e in ests:
                self.keys += [f"{ch}_{name}_{bname}_{e}" for ch in self.ch_names]
        used = len(bands) * len(ests) * self.C
        if o.return_spectrum:
            if len(freqs) != n_eff // 2 + 1:
                raise IndexError(f"{name}: return_spectrum needs a window as long as the nominal segment")
            ints = [int(f) for f in freqs]
            if len(set(ints)) != len(ints):
                raise NotImplementedError(
                    f"{name}: return_spectrum with a bin spacing below 1 Hz yields colliding "
                    "'psd_<int(f)>' keys in the reference; not supported")
            o.psd_cols = _cols(base + used, len(freqs), 1, 0)
            for ch in self.ch_names:
                self.keys += [f"{ch}_{name}_psd_{i}" for i in ints]
            used += self.C * len(freqs)
        return o, used

    def build(self, ref_matrix=None, notch_taps=None, device=0, bank_taps=None, sharpwave_taps=None):
        st, C_, W, sfreq = self.settings, self.C, self.W, self.sfreq
        d = PlanDesc()
        d.abi_version = _lib.NMX_ABI_VERSION
        d.device = int(device)
        d.n_channels = C_
        d.window = W
        if self.resample_ratio:
            d.raw_window = int(self.W_in)
            d.resample_ratio = float(self.resample_ratio)
            if self.resample_npad != "auto":
                if self.W_in + 2 * self.resample_npad > 65536:
                    raise ValueError(f"raw_resampling: raw window {self.W_in} + 2 x resample_npad {self.resample_npad} = "
                                     f"{self.W_in + 2 * self.resample_npad} samples exceeds the padded limit of 65 536")
                d.resample_npad_mode, d.resample_npad = 1, int(self.resample_npad)
        if self._raw_norm is not None:              # raw_normalization, last pre-processor
            method, clip, n_hist, add = self._raw_norm
            # "quantile": scikit-learn's QuantileTransformer subsamples histories of more than 10 000 samples at random
            # (random_state=None: the reference is not reproducible there); the device draws its own uniformly
            # random subset per hop and channel (nmx_k_rawnorm.h) -- equal in distribution, exact below 10 000 samples
            codes = {"mean": 1, "zscore": 2, "median": 3, "zscore-median": 4, "robust": 5, "minmax": 6,
                     "quantile": 7, "power": 8}
            if method not in codes:
                raise NotImplementedError(f"raw_normalization method {method!r} has no device implementation")
            d.raw_norm_method = codes[method]
            d.raw_norm_clip = float(clip) if clip else 0.0
            d.raw_norm_n, d.raw_norm_add = int(n_hist), int(add)
        d.n_pre_filters = len(self._pre_taps)       # preprocessing_filter stages, before the notch
        for i, t in enumerate(self._pre_taps):
            d.pre_taps[i] = self._dptr(t)
            d.n_pre_taps[i] = len(t)
        d.sfreq = sfreq
        d.segment_length_s = float(st.segment_length_features_ms) / 1000.0
        d.feat_hz = float(st.sampling_rate_features_hz)
        bands = [(name, (float(fr[0]), float(fr[1]))) for name, fr in st.frequency_ranges_hz.items()]
        if len(bands) > _lib.NMX_MAX_BANDS:
            raise ValueError(f"at most {_lib.NMX_MAX_BANDS} frequency bands are supported")
        d.n_bands = len(bands)
        band_index = {name: i for i, (name, _) in enumerate(bands)}
        filters: list[dict] = []
        band_filter: dict[str, int] = {}

        def bank_filter(name: str) -> dict:
            """FIR of band `name` (shared by BandPower and Bursts: same MNEFilter arguments)."""
            if name not in band_filter:
                if bank_taps is not None:
                    taps = np.asarray(bank_taps)[band_index[name]]
                else:
                    taps = fir_design.band_pass_bank([bands[band_index[name]][1]], sfreq)[0]
                band_filter[name] = len(filters)
                filters.append({"taps": taps, "bp_seglen": 0, "bp_band": 0, "burst": -1, "sw": -1})
            return filters[band_filter[name]]

        feats = 0
        col = 0
        for f in self.enabled:
            feats |= _FEATURE_BITS[f]
            if f == "raw_hjorth":
                d.hjorth_cols = _cols(col, 3, 1, 0)
                for ch in self.ch_names:
                    self.keys += [f"{ch}_RawHjorth_Activity", f"{ch}_RawHjorth_Mobility",
                                  f"{ch}_RawHjorth_Complexity"]
                col += 3 * C_
            elif f == "return_raw":
                d.raw_cols = _cols(col, 1)
                self.keys += [f"{ch}_raw" for ch in self.ch_names]
                col += C_
            elif f == "linelength":
                d.linelength_cols = _cols(col, 1)
                self.keys += [f"{ch}_LineLength" for ch in self.ch_names]
                col += C_
            elif f == "fft":
                n = int(np.floor(st.fft_settings.windowlength_ms / 1000 * sfreq))
                freqs = np.fft.rfftfreq(n, 1 / np.floor(int(sfreq)))
                d.fft, used = self._osc(st.fft_settings, "fft", n, freqs, False, bands, col)
                col += used
            elif f == "welch":
                n = int(sfreq)
                freqs = np.fft.rfftfreq(n, 1 / n)
                d.welch, used = self._osc(st.welch_settings, "welch", n, freqs, False, bands, col)
                col += used
            elif f == "stft":
                n = int(st.stft_settings.windowlength_ms)   # ms used as samples (oscillatory.py:199)
                freqs = np.fft.rfftfreq(n, 1 / int(sfreq))
                d.stft, used = self._osc(st.stft_settings, "stft", n, freqs, True, bands, col)
                col += used
            elif f == "bandpass_filter":
                bp = st.bandpass_filter_settings
                bfeats = _enabled(bp.bandpower_features)
                if getattr(bp, "kalman_filter", False) and "activity" in bfeats:
                    # bandpower.py:125-126,147-156: one filter per channel for every band of
                    # kalman_filter_settings.frequency_bands (bands missing from
                    # frequency_ranges_hz never match a feature name and stay unused)
                    ks = st.kalman_filter_settings
                    d.bp_kalman_mask = sum(1 << band_index[b] for b in ks.frequency_bands if b in band_index)
                    d.kalman_Tp, d.kalman_sigma_w, d.kalman_sigma_v = float(ks.Tp), float(ks.sigma_w), float(ks.sigma_v)
                d.bp_features = sum(1 << ["activity", "mobility", "complexity"].index(x) for x in bfeats)
                d.bp_log_transform = int(bool(bp.log_transform))
                nf = len(bfeats)
                d.bp_cols = _cols(col, len(bands) * nf, nf, 1)
                for name, _ in bands:
                    fd = bank_filter(name)
                    fd["bp_seglen"] = min(int(np.floor(sfreq / 1000 * bp.segment_lengths_ms[name])), W)   # y[..., -seglen:]
                    fd["bp_band"] = band_index[name]
                for ch in self.ch_names:
                    for name, _ in bands:
                        self.keys += [f"{ch}_bandpass_{x}_{name}" for x in bfeats]
                col += C_ * len(bands) * nf
            elif f == "bursts":
                bs = st.bursts_settings
                names = list(bs.frequency_bands)
                for nme in names:
                    if nme not in band_index:
                        raise validation_error(f"bursting {nme} needs to be defined in "
                                               "settings['frequency_ranges_hz']",
                                               ["burst_settings", "frequency_bands"])
                groups = _enabled(bs.burst_features)
                slots, mask, bit = [], 0, 0
                for g, outs in _BURST_SLOTS:
                    for o in outs:
                        if g in groups:
                            mask |= 1 << bit
                        bit += 1
                # the reference emits the groups in burst_features order, which is _BURST_SLOTS order
                for g in groups:
                    slots += dict(_BURST_SLOTS)[g]
                d.n_burst_bands = len(names)
                d.burst_threshold = float(bs.threshold)
                d.burst_time_duration_s = float(bs.time_duration_s)
                d.burst_out_mask = mask
                d.burst_cols = _cols(col, len(names) * len(slots), len(slots), 1)
                for i, nme in enumerate(names):
                    bank_filter(nme)["burst"] = i
                for ch in self.ch_names:
                    for nme in names:
                        self.keys += [f"{ch}_bursts_{nme}_{s}" for s in slots]
                col += C_ * len(names) * len(slots)
            elif f == "sharpwave_analysis":
                col = self._sharpwave(d, filters, col, sharpwave_taps)
            elif f == "coherence":
                col = self._coherence(d, col)
            elif f == "nolds":
                col = self._nolds(d, col, bands, bank_taps)
        d.features = feats
        d.n_outputs = col
        if len(filters) > _lib.NMX_MAX_FILTERS:
            raise ValueError(f"at most {_lib.NMX_MAX_FILTERS} FIR filters per plan are supported")
        d.n_filters = len(filters)
        for i, fd in enumerate(filters):
            taps = np.asarray(fd["taps"], np.float64)
            d.filters[i].taps = self._dptr(taps)
            d.filters[i].n_taps = len(taps)
            d.filters[i].bp_seglen = fd["bp_seglen"]
            d.filters[i].bp_band_index = fd["bp_band"]
            d.filters[i].burst_index = fd["burst"]
            d.filters[i].sw_index = fd["sw"]
        filter_taps = [np.asarray(fd["taps"], np.float64) for fd in filters]
        if notch_taps is not None:
            nt = np.asarray(notch_taps, np.float64)
            d.notch_taps = self._dptr(nt)
            d.n_notch_taps = len(nt)
        if ref_matrix is not None:
            R = np.ascontiguousarray(ref_matrix, np.float64)
            if R.ndim != 2 or R.shape[0] != C_:
                raise ValueError("ref_matrix must be [n_channels, n_channels_in]")
            d.ref_matrix = self._dptr(R)
            d.n_channels_in = R.shape[1]
        else:
            d.n_channels_in = C_
        assert len(self.keys) == col
        return d, self.keys, self.coh_pairs, filter_taps, self._keep

    def _sharpwave(self, d: PlanDesc, filters: list, col: int, sharpwave_taps) -> int:
        st, sfreq, C_ = self.settings, self.sfreq, self.C
        sw = st.sharpwave_analysis_settings
        used = [f for f in _lib.SW_FEATURES if getattr(sw.sharpwave_features, f)]
        est_of = {f: [e for e in _lib.SW_ESTIMATORS if f in sw.estimator[e]] for f in used}
        for f in used:
            assert est_of[f], f"Add estimator key for {f}"
        combos = [(f, e) for f in used for e in est_of[f]]
        if len(combos) > _lib.NMX_MAX_SW_COMBOS:
            raise ValueError("too many sharp-wave (feature, estimator) pairs")
        names = []
        for i, fr in enumerate(sw.filter_ranges_hz):
            assert fr[1] < sfreq, ("Filter range has to be smaller than sfreq, "
                                   f"got sfreq {sfreq} and filter range {fr}")
            names.append(f"range_{fr[0]:.0f}_{fr[1]:.0f}")
            taps = (np.asarray(sharpwave_taps[i]) if sharpwave_taps is not None
                    else fir_design.band_pass(sfreq, fr[0], fr[1]))
            filters.append({"taps": taps, "bp_seglen": 0, "bp_band": 0, "burst": -1, "sw": i})
        d.n_sw_filters = len(names)
        d.sw_n_combos = len(combos)
        for i, (f, e) in enumerate(combos):
            d.sw_combo_feature[i] = _lib.SW_FEATURES.index(f)
            d.sw_combo_estimator[i] = _lib.SW_ESTIMATORS.index(e)
        d.sw_distance_peaks = float(sw.detect_troughs.distance_peaks_ms)      # sharpwaves.py:339-344
        d.sw_distance_troughs = float(sw.detect_troughs.distance_troughs_ms)
        d.sw_estimate_peaks = int(bool(sw.detect_peaks.estimate))
        d.sw_estimate_troughs = int(bool(sw.detect_troughs.estimate))
        between = bool(sw.apply_estimator_between_peaks_and_troughs)
        d.sw_between = int(between)
        NF = len(names)
        if between:
            reg = [(f, e) for f, e in combos if f != "num_peaks"]
            d.sw_cols = _cols(col, NF * len(reg), len(reg), 1)
            for ch in self.ch_names:
                for fn in names:
                    self.keys += [f"{ch}_Sharpwave_{e.title()}_{f}_{fn}" for f, e in reg]
            col += C_ * NF * len(reg)
            if "num_peaks" in used:
                d.sw_numpeaks_cols = _cols(col, NF, 1, 0)
                for ch in self.ch_names:
                    self.keys += [f"{ch}_Sharpwave_num_peaks_{fn}" for fn in names]
                col += C_ * NF
        else:
            pols = ([("Peak")] if d.sw_estimate_peaks else []) + (["Trough"] if d.sw_estimate_troughs else [])
            slots, seen_np = [], False
            for f, e in combos:
                if f == "num_peaks":
                    if seen_np:
                        continue
                    seen_np = True
                    slots.append("{ch}_Sharpwave_num_peaks_{fn}")
                else:
                    slots.append("{ch}_Sharpwave_" + e.title() + "_" + f + "_{fn}")
            npol = len(pols)
            d.sw_cols = _cols(col, NF * len(slots) * npol, len(slots) * npol, npol)
            for ch in self.ch_names:
                for fn in names:
                    for s in slots:
                        self.keys += [s.format(ch=ch, fn=fn) + "_analyze_" + p for p in pols]
            col += C_ * NF * len(slots) * npol
        return col

    def _coherence(self, d: PlanDesc, col: int) -> int:
        """features/coherence.py: the reference's construction-time checks (Coherence.test_settings), the pairs resolved
        by name prefix, bins of scipy's float64 grid with strict band edges, keys pair by pair."""
        st, sfreq = self.settings, self.sfreq
        cs = st.coherence_settings
        pairs = [list(p) for p in cs.channels]
        for ch_coh in [ch for p in pairs for ch in p]:
            hits = sum(ch.startswith(ch_coh) for ch in self.ch_names)
            if hits == 0:
                raise RuntimeError(f"Coherence selected channel {ch_coh} does not match any channel name: \n"
                                   f"  - settings.coherence_settings.channels: {cs.channels}\n"
                                   f"  - ch_names: {self.ch_names} \n")
            if hits > 1:
                raise RuntimeError(f"Coherence selected channel {ch_coh} is ambigous and matches more than one channel "
                                   f"name: \n  - settings.coherence_settings.channels: {cs.channels}\n"
                                   f"  - ch_names: {self.ch_names} \n")
        band_names = [str(b).replace(" ", "_") for b in cs.frequency_bands]
        ranges = st.frequency_ranges_hz
        if not all(b in ranges for b in band_names):
            raise AssertionError("coherence selected frequency bands don't match the ones specified in "
                                 f"s['frequency_ranges_hz'] coherence frequency bands: {band_names} specified "
                                 f"frequency_ranges_hz: {ranges}")
        if not all(ranges[b][0] < sfreq / 2 and ranges[b][1] < sfreq / 2 for b in band_names):
            raise AssertionError("the coherence frequency band ranges need to be smaller than the Nyquist frequency "
                                 f"got sfreq = {sfreq} and fband ranges {band_names}")
        if len(band_names) > _lib.NMX_MAX_BANDS:
            raise ValueError(f"at most {_lib.NMX_MAX_BANDS} coherence frequency bands are supported")
        feats = _enabled(cs.features)
        use_coh, use_icoh = bool(cs.method.coh), bool(cs.method.icoh)
        nfb = ("mean_fband" in feats) + ("max_fband" in feats)
        slots = len(band_names) * nfb + ("max_allfbands" in feats)
        if not pairs or slots == 0:
            return col   # (no pair, or nothing to compute: the reference emits no key either)
        if not use_coh:
            # get_coh reads the coh values for every method (coherence.py:104-117): the reference raises
            # UnboundLocalError on its first window
            raise ValueError("coherence_settings.method.coh = False: the reference cannot run this setting "
                             "(CoherenceObject.get_coh fails with UnboundLocalError on its first window)")
        n = min(int(cs.nperseg), self.W)   # scipy.signal.welch: nperseg > len(x) -> len(x)
        if n < 2 or n > COH_MAX_NPERSEG:
            raise ValueError(f"coherence: nperseg {n} (after the clamp to the {self.W}-sample window) must lie in "
                             f"[2, {COH_MAX_NPERSEG}]")
        freqs = np.fft.rfftfreq(n, 1 / sfreq)
        for b, name in enumerate(band_names):
            lo, hi = float(ranges[name][0]), float(ranges[name][1])
            idx = np.where((freqs > lo) & (freqs < hi))[0]
            if not idx.size and "max_fband" in feats:   # np.max over an empty band (coherence.py:136)
                raise ValueError("zero-size array to reduction operation maximum which has no identity "
                                 f"(coherence: band {name} holds no bin of the {len(freqs)}-bin grid)")
            d.coh_bin_lo[b] = int(idx[0]) if idx.size else 0
            d.coh_bin_hi[b] = int(idx[-1]) + 1 if idx.size else 0
        # a pair listed twice writes the same keys with the same values (they keep their first position)
        seen, index = set(), []
        methods = ["coh"] + (["icoh"] if use_icoh else [])   # icoh off: the coh keys are written twice
        for c1, c2 in pairs:
            if (c1, c2) in seen:
                continue
            seen.add((c1, c2))
            i1 = next(i for i, ch in enumerate(self.ch_names) if ch.startswith(c1))
            i2 = next(i for i, ch in enumerate(self.ch_names) if ch.startswith(c2))
            index += [i1, i2]
            for m in methods:
                for name in band_names:
                    if "mean_fband" in feats:
                        self.keys.append(f"{m}_{c1}_to_{c2}_mean_fband_{name}")
                    if "max_fband" in feats:
                        self.keys.append(f"{m}_{c1}_to_{c2}_max_fband_{name}")
                if "max_allfbands" in feats:
                    self.keys.append(f"{m}_{c1}_to_{c2}_max_allfbands_{band_names[-1]}")
        n_pairs = len(index) // 2
        idx_arr = np.ascontiguousarray(index, dtype=np.int32)
        self._keep.append(idx_arr)
        d.coh_n_pairs = n_pairs
        d.coh_pairs = idx_arr.ctypes.data_as(C.POINTER(C.c_int32))
        d.coh_nperseg = n
        d.coh_n_bands = len(band_names)
        d.coh_features = sum(1 << i for i, f in enumerate(["mean_fband", "max_fband", "max_allfbands"]) if f in feats)
        d.coh_methods = 1 | (2 if use_icoh else 0)
        d.coh_df = float(freqs[1] if len(freqs) > 1 else 0.0)
        d.coh_cols = _cols(col, 0, len(methods) * slots, slots)
        self.coh_pairs = [(int(index[2 * i]), int(index[2 * i + 1])) for i in range(n_pairs)]
        return col + n_pairs * len(methods) * slots

    def _nolds(self, d: PlanDesc, col: int, bands, bank_taps) -> int:
        """features/nolds.py: the constructor's checks, the series (the window, then one band series per entry of
        ``nolds_settings.frequency_bands``) and the keys, raw first, then band by band, channel-major inside each.

        The band-index quirk, reproduced on purpose: the reference filters with the bank over ALL of
        ``frequency_ranges_hz`` and reads ``data_filt[:, i, :]`` with ``i`` the position in nolds' OWN list
        (nolds.py:59-65).  Key ``..._<nolds band i>`` therefore holds the entropy of GLOBAL band ``i`` -- with the
        defaults ``..._low_beta`` is the theta series.  Same numbers under the same keys is the goal."""
        st, sfreq = self.settings, self.sfreq
        ns = st.nolds_settings
        feats = _enabled(ns.features)
        other = [f for f in feats if f != "sample_entropy"]
        poly = nolds_poly_measures(self.nolds_fit)
        dfa = "detrended_fluctuation_analysis" in poly and "detrended_fluctuation_analysis" in feats
        hurst = "hurst_exponent" in poly and "hurst_exponent" in feats
        if dfa:   # (nolds.dfa(x, fit_exp="poly") has a kernel; the string "poly" means this measure alone)
            other.remove("detrended_fluctuation_analysis")
        if hurst:   # (nolds.hurst_rs(x, fit="poly") has one too; correlation_dimension and lyapunov_exponent keep raising)
            other.remove("hurst_exponent")
        if other:
            raise NotImplementedError(
                f"nolds measures {other} are not implemented: the reference ends them in a line fit that defaults to "
                "fit='RANSAC' -- scikit-learn's RANSACRegressor without a seed -- so two runs of the reference do not agree "
                "with each other and no parity can be checked; only sample_entropy runs on the device")
        names = [str(b).replace(" ", "_") for b in ns.frequency_bands]
        if names:
            # BandPower(settings, ch_names, sfreq, use_kf=False): its loop reads segment_lengths_ms[band] for every band
            # of frequency_ranges_hz (bandpower.py:128-131)
            seg = st.bandpass_filter_settings.segment_lengths_ms
            for bname, _ in bands:
                if bname not in seg:
                    raise KeyError(bname)
        for fb in names:
            assert fb in st.frequency_ranges_hz, (
                f"{fb} selected in nolds_features, but not defined in s['frequency_ranges_hz']")
        if len(names) > len(bands):
            raise IndexError(f"index {len(bands)} is out of bounds for axis 1 with size {len(bands)} (nolds reads band "
                             "series by the position in nolds_settings.frequency_bands)")
        if self.W > NOLDS_MAX_SAMPLES:
            raise ValueError(f"nolds: a window of {self.W} samples exceeds the {NOLDS_MAX_SAMPLES}-sample limit of the "
                             "sample-entropy kernel (the series has to fit the compute unit's local memory)")
        raw = bool(ns.raw)
        series = (["raw"] if raw else []) + names
        if not feats or not series:
            return col   # (nothing to compute: the reference emits no key either)
        d.nolds_raw = int(raw)
        d.nolds_n_bands = len(names)
        for j in range(len(names)):
            if bank_taps is not None:
                taps = np.asarray(bank_taps)[j]
            else:
                taps = fir_design.band_pass_bank([bands[j][1]], sfreq)[0]
            taps = np.asarray(taps, np.float64)
            d.nolds_taps[j] = self._dptr(taps)
            d.nolds_n_taps[j] = len(taps)
        d.nolds_measures = sum(1 << _lib.NOLDS_MEASURES.index(f) for f in feats)
        d.nolds_tol_factor = NOLDS_TOL_FACTOR
        d.nolds_ddof = NOLDS_DDOF
        C_ = self.C
        # inside a series and a channel the measures stand in get_enabled() order: sample_entropy, hurst_exponent, DFA
        nf = len(feats)
        if "sample_entropy" in feats:
            d.nolds_cols = _cols(col + feats.index("sample_entropy"), nf, C_ * nf, 0)
        if dfa:
            scales = np.ascontiguousarray(dfa_scales(self.W), dtype=np.int32)   # (nolds' ValueError below four samples)
            if len(scales) > NOLDS_DFA_MAX_SCALES:
                raise ValueError(f"nolds: {len(scales)} DFA scales exceed the kernel's table of {NOLDS_DFA_MAX_SCALES}")
            self._keep.append(scales)
            d.nolds_dfa_fit = 1
            d.nolds_dfa_n_scales = len(scales)
            d.nolds_dfa_scales = scales.ctypes.data_as(C.POINTER(C.c_int32))
            d.nolds_dfa_cols = _cols(col + feats.index("detrended_fluctuation_analysis"), nf, C_ * nf, 0)
        if hurst:
            scales = np.ascontiguousarray(hurst_scales(self.W), dtype=np.int32)   # (ValueError below five samples)
            log_e = np.ascontiguousarray([math.log(hurst_expected_rs(n)) for n in scales], dtype=np.float64)
            self._keep += [scales, log_e]
            d.nolds_hurst_fit = 1
            d.nolds_hurst_n_scales = len(scales)
            d.nolds_hurst_scales = scales.ctypes.data_as(C.POINTER(C.c_int32))
            d.nolds_hurst_log_expected = log_e.ctypes.data_as(C.POINTER(C.c_double))
            d.nolds_hurst_cols = _cols(col + feats.index("hurst_exponent"), nf, C_ * nf, 0)
        for sname in series:
            for ch in self.ch_names:
                self.keys += [f"{ch}_nolds_{f}_{sname}" for f in feats]
        return col + len(series) * C_ * len(feats)
