"""What stands between the recording and the features, planned on the host (pure NumPy: no library, no device).

``PrepPlan``: the pre-processors in PREPROCESSOR_DICT order filtered by membership in settings.preprocessing
(processing/data_preprocessor.py:9-15,45-51) as designed taps / tuples, and the channel pick folded with the
re-reference into one [C, C_all] matrix applied on the device.  ``LocalInput``: the rows of that matrix a channel shard
owns, re-expressed over the few input rows the shard is handed.
"""

from __future__ import annotations

import numpy as np

from . import channels as chmod
from . import fir_design

PREPROCESSOR_ORDER = ["preprocessing_filter", "notch_filter", "raw_resampling", "re_referencing", "raw_normalization"]


class PrepPlan:
    """``order`` (the validated pre-processing order), ``notch_taps``, ``pre_taps``, ``raw_norm`` (method, clip, N samples,
    add samples), ``resample_to`` (None: no resampler), ``sfreq_design`` (the rate the features are designed with) and
    ``matrix`` (the folded [C, C_all] channel pick x re-reference, None: the identity)."""

    def __init__(self, settings, channels, sfreq, line_noise=None, resample_features_at_new_rate: bool = False,
                 resample_npad=None) -> None:
        from .plan_desc import resample_npad_arg

        st = settings
        self.resample_npad = resample_npad_arg(resample_npad)   # "auto" or samples per side (keyword, else NMX_RESAMPLE_NPAD)
        self.sfreq_raw = sfreq // 1
        self.ch_names_used, self.feature_idx, self.target_idx = chmod.channel_info(channels)
        self.notch_taps = self.pre_taps = self.raw_norm = self.resample_to = self.ref_matrix = None
        for name in st.preprocessing:
            if name not in PREPROCESSOR_ORDER:
                raise ValueError(f"Invalid preprocessing method '{name}'. Must be one of {PREPROCESSOR_ORDER}")
        self.order = [name for name in PREPROCESSOR_ORDER if name in st.preprocessing]
        for name in self.order:
            if name == "notch_filter":
                if line_noise is None:
                    raise ValueError("Either line_noise or freqs must be defined if notch_filter is activated.")
                self.notch_taps = fir_design.notch_bank(self.sfreq_raw, line_noise)
            elif name == "preprocessing_filter":
                self.pre_taps = fir_design.preprocessing_filter_bank(st.preprocessing_filter, self.sfreq_raw)
            elif name == "raw_resampling":
                new_rate = float(st.raw_resampling_settings.resample_freq_hz)
                if float(new_rate / self.sfreq_raw) != 1.0:
                    # The reference resamples every window but keeps building notch AND features with the
                    # RAW rate (stream/data_processor.py:55,68,80): every frequency axis of the features is
                    # off by the ratio.  Reproduced as is (default); resample_features_at_new_rate=True
                    # selects the consistent pipeline (features designed for the rate they see).
                    self.resample_to = new_rate
                    if not resample_features_at_new_rate:
                        from . import logger

                        logger.info("raw_resampling %g -> %g Hz: features are designed with the raw rate like "
                                    "the reference (pass resample_features_at_new_rate=True for the new rate)",
                                    self.sfreq_raw, new_rate)
            elif name == "re_referencing":
                self.ref_matrix = chmod.reref_matrix(channels)
            elif name == "raw_normalization":
                rs = st.raw_normalization_settings
                rate = self.resample_to if (self.resample_to is not None and resample_features_at_new_rate) else self.sfreq_raw
                # normalization.py:52-58: add_samples = int(sfreq / feat_hz), N = int(time_s * sfreq)
                self.raw_norm = (rs.normalization_method, rs.clip, int(rs.normalization_time_s * rate),
                                 int(rate / st.sampling_rate_features_hz))
        self.sfreq_design = (self.resample_to if self.resample_to is not None and resample_features_at_new_rate
                             else self.sfreq_raw)
        R, C, n_all = self.ref_matrix, len(self.feature_idx), len(channels)
        if R is not None and R.shape[0] != C:
            raise ValueError(f"re-reference matrix is {R.shape} but {C} channels are picked for features")
        # fold data[feature_idx] (and R) into one [C, C_all] matrix applied on the device
        self.matrix = None
        if R is not None or self.feature_idx != list(range(n_all)):
            S = np.zeros((C, n_all))
            S[np.arange(C), self.feature_idx] = 1.0
            self.matrix = (R @ S) if R is not None else S

    def engine_kwargs(self, window) -> dict:
        """HotPathEngine's keywords for windows of ``window`` incoming samples (None: the settings' segment length).  With a
        resampler ``window`` counts RAW samples (the generator cuts raw data) and the features are designed with
        ``sfreq_design``: the raw rate like the reference (windows resampled, everything designed as if they were not), or
        the new rate (resample_features_at_new_rate)."""
        kw = dict(sfreq=self.sfreq_design, ref_matrix=self.matrix, notch_taps=self.notch_taps, pre_taps=self.pre_taps,
                  raw_norm=self.raw_norm)
        if self.resample_to is None:
            return dict(kw, window=window)
        return dict(kw, resample_from=self.sfreq_raw, resample_to=self.resample_to, raw_window=window,
                    resample_npad=self.resample_npad)


class LocalInput:
    """A channel shard WITHOUT replicating the recording: the shard is handed only the input rows its own output rows tap
    (``rows``, global indices in order), plus per type group it needs (``groups``: the member rows of each) TWO float32
    rows holding hi + lo of the float64 sum_{j in group} x_j (channels.split_hi_lo, at local rows ``pairs[q]`` and
    ``pairs[q] + 1``): the device accumulates coefficient x row in float64, so the re-referenced sample is rounded to
    float32 once, as in the single-device kernel that forms the sum itself.  ``matrix``: the shard's rows of the folded
    matrix over these ``n_rows`` local rows -- a handful of non-zeros per row -- or None when it is the identity."""

    def __init__(self, full: np.ndarray) -> None:
        """``full``: the shard's rows of PrepPlan.matrix, [C_shard, C_all]."""
        st_ = chmod.reref_structure(full)
        if st_ is None:
            raise NotImplementedError("local_inputs needs re-reference rows made of a few named channels "
                                      "and / or one group average (processing/rereference.py:52-86)")
        taps, gi, gb, groups = st_
        self.rows = sorted({j for t in taps for j, _ in t})
        self.pos = {j: i for i, j in enumerate(self.rows)}
        used = sorted({int(k) for k in gi if k >= 0})
        self.groups = [groups[k] for k in used]
        self.pairs = [len(self.rows) + 2 * i for i in range(len(used))]
        self.n_rows = len(self.rows) + 2 * len(used)
        gpos = dict(zip(used, self.pairs))
        loc = np.zeros((len(taps), self.n_rows))
        for r, t in enumerate(taps):
            for j, c in t:
                loc[r, self.pos[j]] += c
            if gi[r] >= 0:
                loc[r, gpos[int(gi[r])]] = loc[r, gpos[int(gi[r])] + 1] = gb[r]
        self.matrix = loc if not (loc.shape[0] == loc.shape[1] and np.array_equal(loc, np.eye(len(loc)))) else None

    def columns(self, rows) -> list[int]:
        """Where the global input ``rows`` stand among the local rows."""
        return [self.pos[int(j)] for j in rows]

    def fill_pairs(self, x: np.ndarray, hilo, a: int = 0, b: int | None = None) -> np.ndarray:
        """Samples [a, b) of the hi / lo rows of ``x``: ``hilo[q]`` = split_hi_lo of group q's sum over that range."""
        for p, h in zip(self.pairs, hilo):
            x[p:p + 2, a:b] = h
        return x

    def stage(self, x: np.ndarray, data: np.ndarray, lib, hilo) -> np.ndarray:
        """The shard's input from the recording ``data[C_all, T]`` (float rows libnmx reads in place) into ``x`` float32
        [n_rows, T]: its rows in one pass of libnmx's staging helper, then the hi / lo rows."""
        rows = np.ascontiguousarray(self.rows, dtype=np.int32)
        lib.check(lib.lib.nmx_host_stage_rows(x.ctypes.data, x.strides[0] // 4, data.ctypes.data,
                                              int(data.dtype == np.float64), data.strides[0] // data.itemsize,
                                              rows.ctypes.data, len(rows), 0, data.shape[1], None, 0))
        return self.fill_pairs(x, hilo)

    def row_pointers(self, x: np.ndarray, dst: np.ndarray) -> None:
        """``dst[j]`` (uint64, one per row of the recording) := the address of sample 0 of the row of ``x`` that input row j
        goes to (nmx_host_stage_parts)."""
        dst[self.rows] = x.ctypes.data + np.arange(len(self.rows), dtype=np.uint64) * np.uint64(x.strides[0])

    def mask_to_all(self, mask: np.ndarray, full: np.ndarray) -> np.ndarray:
        """The local NaN mask [n, n_rows] OR-ed into ``full`` [n, C_all] (a group-sum row is never NaN)."""
        r, nl = self.rows, len(self.rows)
        if nl and r == list(range(r[0], r[0] + nl)):
            full[:, r[0]:r[0] + nl] |= mask[:, :nl]
        else:
            full[:, r] |= mask[:, :nl]
        return full
