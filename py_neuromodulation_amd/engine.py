"""Host side of the hot path: settings -> flat C plan -> HIP kernels (via libnmx.so).

``HotPathEngine`` turns a (duck-typed) ``NMSettings`` + channel names into an
``nmx_plan_desc`` (plan_desc.PlanBuilder: band -> FFT-bin tables, FIR taps designed on the host, the output column
of every (feature, channel) in the reference's key order) and drives the C ABI:

    process_window(data[C_in, W] float64) -> float32[F]      one hop, the reference call shape
    process_batch(data[C_in, T], starts)   -> float32[n, F]   many hops resident on the GPU

The host memory around it (result tables, page-locked staging, conversion threads) lives in host_mem.
"""

from __future__ import annotations

import ctypes as C
import os
import threading
import time
from collections.abc import Sequence

import numpy as np

from . import _lib
from .host_mem import (_TABLES, _ld, _offset_scratch, _pool, _rows_ok, _staging, parallel_cast,  # noqa: F401
                       release_staging, release_tables, staging_thread, table_empty, trim_device_pool)
from .plan_desc import COH_MAX_NPERSEG, PlanBuilder  # noqa: F401

MAX_PLAN_WINDOW = 16384   # nmx_plan_create: window in [4, 16384] samples for a plan in general; the stand-alone filter objects cut longer
                          # recordings into segments of this length (a plan of raw_hjorth, return_raw, linelength, fft, welch, nolds and
                          # sharpwave_analysis, without raw normaliser or resampling, may be built up to 40 000 samples; with
                          # NMX_LONG_BURSTS=1 in the environment bursts too, with NMX_LONG_BANDPOWER=1 bandpass_filter, with
                          # NMX_LONG_STFT=1 stft, with NMX_LONG_COHERENCE=1 coherence: raw_normalization and raw_resampling then
                          # are what remains limited)


def long_segments(n_samples: int, halo: int, window: int = MAX_PLAN_WINDOW):
    """A FIR filter over a recording longer than one plan's window, for the stand-alone filter classes (MNEFilter,
    NotchFilter, PreprocessingFilter: the reference's filter any length): windows ``[lo, lo + window)`` of the recording
    and the output samples ``[a, b)`` each of them is exact for -- every sample at least ``halo`` (half the filter, or
    the sum of the halves of a chain) away from a cut that is not an end of the recording, so that it sees the same
    input samples as in one long convolution; at the two ends of the recording the window's own edge handling (zeros,
    or the notch's reflection) IS the recording's.  Yields (lo, a, b)."""
    step = window - 2 * halo
    if step < 1:
        raise ValueError(f"a filter chain of {2 * halo + 1} taps leaves no room for data in one {window}-sample window")
    a = 0
    while a < n_samples:
        lo = min(max(a - halo, 0), n_samples - window)
        b = n_samples if lo + window >= n_samples else lo + window - halo
        yield lo, a, b
        a = b


class HotPathEngine:
    """One plan on one GPU for ``len(ch_names)`` channels."""

    def __init__(self, settings, ch_names: Sequence[str], sfreq: float, *,
                 features: Sequence[str] | None = None, ref_matrix: np.ndarray | None = None,
                 notch_taps: np.ndarray | None = None, device: int = 0,
                 lib: _lib.NmxLibrary | None = None, bank_taps: np.ndarray | None = None,
                 sharpwave_taps: Sequence[np.ndarray] | None = None,
                 window: int | None = None, dry_run: bool = False,
                 resample_from: float | None = None, raw_window: int | None = None,
                 pre_taps: Sequence[np.ndarray] | None = None,
                 raw_norm: tuple | None = None, resample_to: float | None = None, staging_slot: int = 0,
                 extra_cols=0, resample_npad=None, nolds_fit=None) -> None:
        """``sfreq`` is the rate every feature and filter is DESIGNED with (what the reference passes to the
        feature constructors).  ``resample_from`` = sampling rate of the incoming windows when they are
        resampled (raw_resampling, processing/resample.py:19-60): incoming windows then hold ``raw_window``
        samples (default int(segment_length_features_ms / 1000 * resample_from)) and are resampled on the
        device to ``window`` = round(ratio * raw_window) samples, ratio = ``resample_to`` / resample_from.
        ``resample_to`` defaults to ``sfreq`` (features designed for the rate they see).  The reference
        instead keeps designing with the RAW rate (stream/data_processor.py:55,68,80): that is
        ``sfreq = resample_from`` with ``resample_to`` = the new rate -- windows of round(ratio * raw_window)
        samples analysed as if sampled at the raw rate (FFT / Welch segments longer than the window shrink
        to it as NumPy slicing / scipy.signal.welch do, band-pass tails are clamped, bursts keep
        seg_s = segment_length_features_ms / 1000).

        ``resample_npad``: the resampler's padding, ``"auto"`` (the default) or an int >= 0 samples per side -- 100 is what
        the reference's call of ``mne.filter.resample`` gets (plan_desc.resample_npad_arg; None: NMX_RESAMPLE_NPAD).

        ``nolds_fit``: ``"poly"`` lets ``nolds_settings.features.detrended_fluctuation_analysis`` run -- ``nolds.dfa`` with
        its final log-log line fitted by least squares instead of nolds' default, an unseeded RANSAC -- and that measure only.
        A mapping names the fit measure by measure: ``{"hurst_exponent": "poly", "detrended_fluctuation_analysis": "poly"}``
        lets ``nolds.hurst_rs(x, fit="poly")`` run as well.  ``None`` (the default; NMX_NOLDS_FIT where it is not given)
        and ``"RANSAC"`` keep the measures' NotImplementedError (plan_desc.nolds_fit_arg).

        ``dry_run=True`` only derives the plan description and the key list (no library, no
        GPU) -- used to lay out the global column order when channels are sharded over GPUs.

        ``extra_cols``: columns behind the features in every output row (an int, or a function of the key list that
        returns one): room for the grid projection (``attach_projection``).  The rows are then ``row_width`` =
        n_outputs + n_extra floats; 0 keeps the plain layout."""
        self.lib = None if dry_run else (lib if lib is not None else _lib.get_library())
        b = PlanBuilder(settings, ch_names, sfreq, features, window, resample_from, raw_window, resample_to, pre_taps,
                        raw_norm, resample_npad, nolds_fit)
        self.resample_npad = b.resample_npad
        self.nolds_fit = b.nolds_fit
        self.settings, self.ch_names, self.sfreq, self.C, self.enabled = b.settings, b.ch_names, b.sfreq, b.C, b.enabled
        self.W, self.W_in, self.resample_ratio = b.W, b.W_in, b.resample_ratio
        # (`_keep`: the arrays the C struct points into)
        self.desc, self.keys, self.coh_pairs, self.filter_taps, self._keep = b.build(ref_matrix, notch_taps, device,
                                                                                     bank_taps, sharpwave_taps)
        self.n_outputs = len(self.keys)
        self.n_extra = int(extra_cols(self.keys) if callable(extra_cols) else extra_cols)
        self.desc.n_extra_cols = self.n_extra
        self.row_width = self.n_outputs + self.n_extra   # floats per output row (features, then the extra columns)
        self.C_in = int(self.desc.n_channels_in)
        self._plan = C.c_void_p()
        self._dc = None        # host offsets in force (None: not decided yet -- `_host_offsets`)
        self._dc_any = False
        self._pinned = self._norm = self._proj = None   # (staging pool; the attached normaliser and projection)
        if not dry_run:
            self.lib.check(self.lib.lib.nmx_plan_create(C.byref(self.desc), C.byref(self._plan)))
            self._pinned = _staging(self.lib, device, staging_slot)

    # ------------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_plan", None) is not None and self._plan.value:
            self.lib.lib.nmx_plan_destroy(self._plan)
            self._plan = C.c_void_p()
        if getattr(self, "_pinned", None) is not None:
            self._pinned.users -= 1   # (the pool stays cached: host_mem._staging)
        self._pinned = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- offset split (include/nmx.h, nmx_engine_dc.inc) -----------------------------------------------------------------
    @property
    def carries_offsets(self) -> bool:
        """The plan can take a recording as (float32 residual, one float64 constant per row)."""
        yes = C.c_int(0)
        self.lib.check(self.lib.lib.nmx_plan_carries_offsets(self._plan, C.byref(yes)))
        return bool(yes.value)

    def set_offsets(self, d) -> None:
        """``d[C_in]`` float64 (None: none): every recording handed over afterwards is split as x = u + d on the host --
        in float64, before the cast to float32.  ``process_batch`` / ``process_window`` choose the constants themselves
        from the first float64 data they see (`_host_offsets`); this is for callers who know better."""
        if d is None:
            self.lib.check(self.lib.lib.nmx_plan_set_offsets(self._plan, None))
            self._dc = np.zeros(self.C_in)
        else:
            d = np.ascontiguousarray(d, dtype=np.float64)
            if d.shape != (self.C_in,):
                raise ValueError(f"expected {self.C_in} offsets, got shape {d.shape}")
            self.lib.check(self.lib.lib.nmx_plan_set_offsets(self._plan, d.ctypes.data))
            self._dc = d.copy()
        self._dc_any = bool(np.any(self._dc != 0.0))

    def offsets(self):
        """(d_in[C_in], d_pre[C]): constants of the input rows (host + learned on the device) and of the pre-processed
        windows the features read."""
        d_in, d_pre = np.zeros(self.C_in), np.zeros(self.C)
        self.lib.check(self.lib.lib.nmx_plan_get_offsets(self._plan, d_in.ctypes.data, d_pre.ctypes.data, None))
        return d_in, d_pre

    def _host_offsets(self, data: np.ndarray):
        """The host constants in force (None: none).  Decided ONCE per stream, by the first data the engine sees -- a
        result must not depend on how the hops were batched: float64 data that needs it (some row's level beyond 64 times
        its spread: below that a float32 cast costs the features nothing) is split at the mean of each row's first
        samples; float32 data is taken as it is (in front of a re-reference the library splits it on the device)."""
        if self._dc is None:
            d = None
            if data.dtype == np.float64 and self.carries_offsets:
                # (C order: NumPy's sums follow the memory layout, the constants must not.  The copy lives in a scratch array
                # of this thread and the deviations are formed in place: every half-megabyte temporary is an mmap / munmap pair,
                # and on a host with hundreds of cores and a process with dozens of threads those were 2 ms of a fresh stream)
                w = min(data.shape[1], 256)
                seg = _offset_scratch(data.shape[0], w)
                np.copyto(seg, data[:, :w])
                ok = np.isfinite(seg)
                if ok.all():   # (the same sums over the same C-ordered values as below: the same constants)
                    m = seg.sum(1) / w
                    seg -= m[:, None]
                    np.multiply(seg, seg, out=seg)
                    sd = np.sqrt(seg.sum(1) / w)
                    if np.any(np.abs(m) > 64.0 * sd):
                        d = m
                else:
                    cnt = np.maximum(ok.sum(1), 1)
                    m = np.where(ok, seg, 0.0).sum(1) / cnt
                    sd = np.sqrt(np.where(ok, (seg - m[:, None]) ** 2, 0.0).sum(1) / cnt)
                    if np.any(np.abs(m) > 64.0 * sd):
                        d = np.where(ok.any(1), m, 0.0)
            if d is not None:
                self.set_offsets(d)
            else:
                self._dc = np.zeros(self.C_in)
                self._dc_any = False
        return self._dc if self._dc_any else None

    def reset_state(self) -> None:
        self.lib.check(self.lib.lib.nmx_state_reset(self._plan))
        if self._dc is not None and self._dc_any:
            self.lib.check(self.lib.lib.nmx_plan_set_offsets(self._plan, None))
        self._dc = None
        self._dc_any = False

    def export_state(self) -> bytes:
        n = C.c_int64()
        self.lib.check(self.lib.lib.nmx_state_size(self._plan, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        self.lib.check(self.lib.lib.nmx_state_export(self._plan, buf, n.value))
        return buf.raw

    def import_state(self, blob: bytes) -> None:
        self.lib.check(self.lib.lib.nmx_state_import(self._plan, blob, len(blob)))
        # the blob carries the offsets of the stream it came from: adopt them
        st = C.c_int(0)
        d_in = np.zeros(self.C_in)
        self.lib.check(self.lib.lib.nmx_plan_get_offsets(self._plan, d_in.ctypes.data, None, C.byref(st)))
        if st.value & 1:
            host = d_in   # (host offsets set: nothing is learned next to them)
            self._dc, self._dc_any = host, bool(np.any(host != 0.0))
        else:
            self._dc, self._dc_any = np.zeros(self.C_in), False

    def process_window(self, data: np.ndarray, want_nan_mask: bool = False):
        """data[C_in, W] (float64, may be a non-contiguous view) -> float32[row_width]."""
        data = np.asarray(data, dtype=np.float64)
        if data.ndim != 2 or data.shape[0] != self.C_in or data.shape[1] != self.W_in:
            raise ValueError(f"expected data of shape ({self.C_in}, {self.W_in}), got {data.shape}")
        if data.strides[1] != 8:
            data = np.ascontiguousarray(data)
        self._host_offsets(data)   # (the library subtracts them from the float64 window itself)
        out = np.empty(self.row_width, np.float32)
        mask = np.zeros(self.C_in, np.uint8) if want_nan_mask else None
        self.lib.check(self.lib.lib.nmx_process_window(
            self._plan, data.ctypes.data, _ld(data), out.ctypes.data,
            mask.ctypes.data if mask is not None else None))
        return (out, mask.astype(bool)) if want_nan_mask else out

    def attach_normalizer(self, norm) -> None:
        """Run ``norm`` (a DeviceFeatureNormalizer or None) inside this plan's launch sequence: every batch /
        window comes back already normalised, without a second host round trip (nmx_plan_attach_norm)."""
        self.lib.check(self.lib.lib.nmx_plan_attach_norm(self._plan, norm._h if norm is not None else None))
        self._norm = norm   # keep it alive

    def attach_projection(self, proj) -> None:
        """Run ``proj`` (a projection.DeviceProjection or None) inside this plan's launch sequence, behind the attached
        normaliser: the grid columns of every row come back filled (nmx_plan_attach_proj; they need ``extra_cols``)."""
        self.lib.check(self.lib.lib.nmx_plan_attach_proj(self._plan, proj._h if proj is not None else None))
        self._proj = proj   # keep it alive

    def pinned_empty(self, shape, dtype=np.float32) -> np.ndarray:
        """A page-locked array of the caller's own: inputs / ``out=`` buffers allocated here move at the full PCIe
        rate, asynchronously.  The allocation belongs to the returned array (and its views): it is released
        (nmx_host_free) when the last of them is garbage-collected, never handed to anybody else."""
        import weakref

        shape = tuple(int(x) for x in shape)
        count = int(np.prod(shape))
        n = max(count * np.dtype(dtype).itemsize, 1)
        p = C.c_void_p()
        lib = self.lib
        lib.check(lib.lib.nmx_host_alloc(n, C.byref(p)))
        buf = (C.c_char * n).from_address(p.value)
        weakref.finalize(buf, lib.lib.nmx_host_free, p.value)   # numpy keeps `buf` alive as the base of every view
        return np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)

    @property
    def preprocessing_is_identity(self) -> bool:
        """No stage between the incoming rows and the features (no re-reference / channel pick, FIR stage,
        resampler, raw normaliser): the features see nan_to_num(window) itself."""
        d = self.desc
        return not (bool(d.ref_matrix) or d.n_notch_taps or d.n_pre_filters or d.raw_norm_method
                    or self.resample_ratio)

    def process_batch(self, data: np.ndarray, starts: np.ndarray, want_nan_mask: bool = False,
                      staged_output: bool = False, out: np.ndarray | None = None, tap: bool = False):
        """data[C_in, T] host array, starts[n] window start samples -> float32[n, row_width].

        ``tap=True`` appends float32[n, C, W] to the result: the pre-processed windows the features were computed
        from (nmx_process_batch_tap) -- the ``data`` argument of ``NMFeature.calc_feature`` for user-registered
        host features (features/feature_processor.py:52-53,80-82).

        A recording that is not contiguous float32 is cast into a page-locked staging array (first axis
        split over a few threads): the host -> device copies then run at the PCIe rate next to the kernels;
        contiguous float32 input is handed over as it is (allocate it with ``pinned_empty`` for the same
        effect).  ``out``: caller's float32[n, row_width] buffer.  ``staged_output=True`` returns a VIEW of
        the library's page-locked output staging array (valid until the next call) instead of a fresh
        array -- for callers that convert / consume the rows right away."""
        data = np.asarray(data)
        if data.ndim != 2 or data.shape[0] != self.C_in:
            raise ValueError(f"expected data with {self.C_in} rows, got {data.shape}")
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        n = len(starts)
        dc = self._host_offsets(data)
        if dc is None and _rows_ok(data, np.float32) and _ld(data) >= data.shape[1]:
            x = data   # (rows of a C-ordered float32 array or a view with longer rows: handed over as it is)
        elif data.size >= (1 << 18):
            x = self._pinned.array("x", data.shape, np.float32)
            parallel_cast(x, data, dc, self.lib)
        elif dc is not None:
            # any layout comes in (a transposed (samples, channels) array, a DataFrame's ``to_numpy().T``: the reference
            # takes them all, stream/stream.py:108); the library reads C-ordered float32 rows
            x = np.ascontiguousarray(np.asarray(data, dtype=np.float64) - dc[:, None], dtype=np.float32)
        else:
            x = np.ascontiguousarray(data, dtype=np.float32)
        F = self.row_width
        if out is not None:
            if out.dtype != np.float32 or out.shape != (n, F) or not out.flags.c_contiguous:
                raise ValueError(f"out must be a C-contiguous float32 array of shape ({n}, {F})")
        elif staged_output and n * F >= (1 << 18):
            out = self._pinned.array("out", (n, F), np.float32)
        else:
            out = np.empty((n, F), np.float32)
        if want_nan_mask and data.size >= (1 << 18):   # (page-locked next to page-locked samples / rows: see run_pipelined)
            mask = self._pinned.array("mask", (n, self.C_in), np.uint8)
            mask[:] = 0
        else:
            mask = np.zeros((n, self.C_in), np.uint8) if want_nan_mask else None
        if tap:
            pre = np.empty((n, self.C, self.W), np.float32)
            self.lib.check(self.lib.lib.nmx_process_batch_tap(
                self._plan, x.ctypes.data, _ld(x), x.shape[1], starts.ctypes.data, n,
                out.ctypes.data, mask.ctypes.data if mask is not None else None, 0, None, pre.ctypes.data))
            d_pre = self.offsets()[1]
            if np.any(d_pre != 0.0):   # the windows in float64 with their constants back (NMFeature.calc_feature's argument)
                pre = pre.astype(np.float64) + d_pre[None, :, None]
            return (out, mask.astype(bool), pre) if want_nan_mask else (out, pre)
        self.lib.check(self.lib.lib.nmx_process_batch(
            self._plan, x.ctypes.data, _ld(x), x.shape[1], starts.ctypes.data, n,
            out.ctypes.data, mask.ctypes.data if mask is not None else None, 0, None))
        return (out, mask.astype(bool)) if want_nan_mask else out

    def process_batch_f64(self, data: np.ndarray, starts: np.ndarray, want_nan_mask: bool = False, spare_cols: int = 0):
        """``process_batch`` returning the float64 table the reference's consumers expect, with BOTH conversions next to
        the device work instead of around it (nmx_plan_set_pipeline): a thread converts the recording to float32 slice
        by slice into the page-locked staging array and publishes how far it got -- the library enqueues a chunk's copy
        as soon as the samples it reads are there --, another widens the feature rows to float64 as the chunks land
        (their first touch of a fresh 75 MB table costs more than the arithmetic: it, too, hides under the kernels).
        (Measured round 4, 256 ch x 120 s: conversion 1.9 ms + batch 11.7 ms + widening and first touch 4 - 8 ms in a
        row.)  ``spare_cols``: the table gets that many extra columns behind the features for the caller to fill (the
        reference's frame carries "time" and the target channels behind them, stream/stream.py:319-343 -- written into the
        table they need no column insert)."""
        data = np.asarray(data)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        n, F = len(starts), self.row_width
        if data.ndim != 2 or data.shape[0] != self.C_in:
            raise ValueError(f"expected data with {self.C_in} rows, got {data.shape}")
        small = data.size < (1 << 20) or n < 64 or os.environ.get("NMX_PIPELINE", "1") == "0"
        if small or (_rows_ok(data, np.float32) and _ld(data) >= data.shape[1] and self._host_offsets(data) is None):
            res = self.process_batch(data, starts, want_nan_mask=want_nan_mask, staged_output=True)
            out = res[0] if want_nan_mask else res
            o64 = table_empty((n, F + spare_cols))
            parallel_cast(o64[:, :F], out, None, self.lib)
            return (o64, res[1]) if want_nan_mask else o64
        dc = self._host_offsets(data)
        x = self._pinned.array("x", data.shape, np.float32)
        o64 = table_empty((n, F + spare_cols))
        mask = self.run_pipelined(x, starts, o64, stage=lambda a, b: parallel_cast(x[:, a:b], data[:, a:b], dc, self.lib),
                                  want_nan_mask=want_nan_mask)
        return (o64, mask) if want_nan_mask else o64

    def pipeline_counters(self) -> np.ndarray:
        """The int64 counters of ``nmx_plan_set_pipeline`` in page-locked memory, zeroed: [0] samples of the staging array
        in place (written by whoever stages), [8] feature rows landed (written by the library) -- own cache lines."""
        ctr = self._pinned.array("ctr", (16,), np.int64)
        ctr[:] = 0
        return ctr

    def pipeline_edges(self, starts: np.ndarray, T: int) -> list[int]:
        """Sample counts at which to publish progress while staging a recording: what the library's chunks read
        (nmx_engine_run.inc: a short first chunk -- 128 hops, or the fill phase of the burst history, ~320 --, then 512
        hops at a time)."""
        n = len(starts)
        hops = [h for h in (128, 320) if h < n] + list(range(320 + 512, n, 512)) + [n]
        # (finer slices were measured and lose: publishing the first chunk in 8 k-sample pieces, copied as they arrive,
        # costs more in staging calls than the earlier start buys -- Stream.run 17.2 -> 17.9 ms, two plans 12.5 -> 13.6)
        return sorted(set([0] + [int(min(T, starts[h - 1] + self.W_in)) for h in hops] + [T]))

    def run_pipelined(self, x: np.ndarray, starts: np.ndarray, table: np.ndarray, runs: np.ndarray | None = None,
                      stage=None, ctr: np.ndarray | None = None, want_nan_mask: bool = False):
        """One batch with staging and widening NEXT to the device work.  ``x`` float32 [C_in, T]: the (page-locked)
        staging array the library copies from; it is filled either by ``stage(a, b)`` -- called here, on a thread of
        this call, for consecutive sample ranges -- or by the caller, who then owns ``ctr`` (``pipeline_counters()``) and
        publishes in ``ctr[0]`` how many samples of EVERY row are in place (a multi-device stream stages all its parts
        from one thread).  The rows are widened as the chunks land into the float64 ``table``: columns
        ``runs[k] = (first column in table, first column of the engine's row, length)``, None: the whole row from column
        0.  -> the NaN mask (bool [n, C_in]) or None."""
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        n, T = len(starts), x.shape[1]
        if not (_rows_ok(x, np.float32) and x.shape[0] == self.C_in and _rows_ok(table, np.float64) and table.shape[0] == n):
            raise ValueError("run_pipelined: float32 staging rows and a float64 table with one row per window")
        if runs is None:
            runs = np.array([[0, 0, self.row_width]], dtype=np.int64)
        runs = np.ascontiguousarray(runs, dtype=np.int64).reshape(-1, 3)
        out = self._pinned.array("out", (n, self.row_width), np.float32)
        # (page-locked like `out`: a copy into PAGEABLE memory is synchronous for the calling thread -- the library's host
        # loop stood at the mask of chunk k - 1 until that chunk was complete, and the samples of chunk k + 1 waited with it)
        mask = self._pinned.array("mask", (n, self.C_in), np.uint8) if want_nan_mask else None
        if mask is not None:
            mask[:] = 0
        own = ctr is None
        if own:
            ctr = self.pipeline_counters()
        failed: list = []
        lib = self.lib

        def widen():
            done = 0
            try:
                while done < n and not failed:
                    d = int(ctr[8])
                    if d > done:
                        lib.check(lib.lib.nmx_host_widen_rows(table.ctypes.data, table.strides[0] // 8, out.ctypes.data,
                                                              self.row_width, done, d, runs.ctypes.data, len(runs), 0))
                        done = d
                    else:
                        time.sleep(0.0001)
            except BaseException as e:   # noqa: BLE001
                failed.append(e)

        lib.check(lib.lib.nmx_plan_set_pipeline(self._plan, ctr.ctypes.data, ctr.ctypes.data + 64))
        jobs = [threading.Thread(target=widen, daemon=True)]
        if stage is not None:
            jobs.append(staging_thread(lambda: self.pipeline_edges(starts, T), stage, [ctr], T, failed))
        elif own:
            ctr[0] = T   # (nobody stages: the array is complete)
        for j in jobs:
            j.start()
        try:
            lib.check(lib.lib.nmx_process_batch(
                self._plan, x.ctypes.data, _ld(x), T, starts.ctypes.data, n,
                out.ctypes.data, mask.ctypes.data if mask is not None else None, 0, None))
        except BaseException:
            if own:
                ctr[0] = T   # (let the threads run out)
            ctr[8] = n
            failed.append(None)
            raise
        finally:
            lib.lib.nmx_plan_set_pipeline(self._plan, None, None)
            for j in jobs:
                j.join()
        if failed:
            raise failed[0]
        return mask.astype(bool) if want_nan_mask else None

    def process_batch_device(self, x_ptr: int, ldx: int, n_samples: int, starts: np.ndarray,
                             out_ptr: int, mask_ptr: int | None = None, stream: int | None = None) -> None:
        """Device-resident variant: raw pointers on the plan's device (e.g. torch ``data_ptr()``)."""
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        self.lib.check(self.lib.lib.nmx_process_batch(
            self._plan, x_ptr, ldx, n_samples, starts.ctypes.data, len(starts), out_ptr, mask_ptr,
            1, stream))

    def preprocess_window(self, data: np.ndarray) -> np.ndarray:
        data = np.ascontiguousarray(data, dtype=np.float64)
        if data.ndim != 2 or data.shape != (self.C_in, self.W_in):
            raise ValueError(f"expected data of shape ({self.C_in}, {self.W_in}), got {data.shape}")
        y = np.empty((self.C, self.W), np.float64)
        self.lib.check(self.lib.lib.nmx_preprocess_window(self._plan, data.ctypes.data, data.shape[1],
                                                         y.ctypes.data, self.W))
        return y

    def filter_window(self, data: np.ndarray) -> np.ndarray:
        data = np.ascontiguousarray(data, dtype=np.float64)
        y = np.empty((self.C, int(self.desc.n_filters), self.W), np.float64)
        self.lib.check(self.lib.lib.nmx_filter_window(self._plan, data.ctypes.data, data.shape[1],
                                                     y.ctypes.data))
        return y

    def nolds_probe(self, data: np.ndarray, starts: np.ndarray, want_series: bool = True) -> dict:
        """``process_batch`` of a plan with nolds that also hands back what the sample-entropy kernel counted
        (nmx_nolds_probe): ``"out"`` float32[n, row_width]; ``"A"``, ``"B"`` (uint32), ``"tol"`` (float32), ``"sum_zero"``
        (bool), each [n, n_series, C] with the series raw first, then the bands; ``"series"`` float32[n, n_series, C, W]: the
        samples the walk read (without the plan's carried offsets, which no difference sees).  For tests that judge the
        counts, not only their logarithm, on the series the kernel itself read."""
        data = np.asarray(data)
        if data.ndim != 2 or data.shape[0] != self.C_in:
            raise ValueError(f"expected data with {self.C_in} rows, got {data.shape}")
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        dc = self._host_offsets(data)
        x = np.ascontiguousarray(data if dc is None else np.asarray(data, np.float64) - dc[:, None], dtype=np.float32)
        n, S = len(starts), int(self.desc.nolds_raw) + int(self.desc.nolds_n_bands)
        out = np.empty((n, self.row_width), np.float32)
        a, b = np.zeros((n, S, self.C), np.uint32), np.zeros((n, S, self.C), np.uint32)
        tol, zero = np.zeros((n, S, self.C), np.float32), np.zeros((n, S, self.C), np.uint8)
        series = np.zeros((n, S, self.C, self.W), np.float32) if want_series else None
        self.lib.check(self.lib.lib.nmx_nolds_probe(
            self._plan, x.ctypes.data, _ld(x), x.shape[1], starts.ctypes.data, n, out.ctypes.data, a.ctypes.data,
            b.ctypes.data, tol.ctypes.data, zero.ctypes.data, series.ctypes.data if series is not None else None))
        return {"out": out, "A": a, "B": b, "tol": tol, "sum_zero": zero.astype(bool), "series": series}

    def nolds_dfa_probe(self, data: np.ndarray, starts: np.ndarray, want_series: bool = True) -> dict:
        """``process_batch`` of a plan with detrended fluctuation analysis that also hands back what the DFA kernel formed
        (nmx_nolds_dfa_probe): ``"out"`` float32[n, row_width]; ``"scales"`` int[S], the plan's table; ``"F"`` float64[n,
        n_series, C, S], the fluctuation function; ``"alpha"`` float64 (the slope, before the sum rule), ``"sum_zero"`` (bool)
        and ``"n_kept"`` (scales with F != 0), each [n, n_series, C]; ``"series"`` float32[n, n_series, C, W]: the samples the
        kernel read."""
        data = np.asarray(data)
        if data.ndim != 2 or data.shape[0] != self.C_in:
            raise ValueError(f"expected data with {self.C_in} rows, got {data.shape}")
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        dc = self._host_offsets(data)
        x = np.ascontiguousarray(data if dc is None else np.asarray(data, np.float64) - dc[:, None], dtype=np.float32)
        n, S = len(starts), int(self.desc.nolds_raw) + int(self.desc.nolds_n_bands)
        K = int(self.desc.nolds_dfa_n_scales)
        out = np.empty((n, self.row_width), np.float32)
        fluct, alpha = np.zeros((n, S, self.C, K), np.float64), np.zeros((n, S, self.C), np.float64)
        zero, kept = np.zeros((n, S, self.C), np.uint8), np.zeros((n, S, self.C), np.int32)
        series = np.zeros((n, S, self.C, self.W), np.float32) if want_series else None
        self.lib.check(self.lib.lib.nmx_nolds_dfa_probe(
            self._plan, x.ctypes.data, _ld(x), x.shape[1], starts.ctypes.data, n, out.ctypes.data, fluct.ctypes.data,
            alpha.ctypes.data, zero.ctypes.data, kept.ctypes.data, series.ctypes.data if series is not None else None))
        scales = np.array([self.desc.nolds_dfa_scales[k] for k in range(K)], np.int64)
        return {"out": out, "scales": scales, "F": fluct, "alpha": alpha, "sum_zero": zero.astype(bool), "n_kept": kept,
                "series": series}

    def nolds_hurst_probe(self, data: np.ndarray, starts: np.ndarray, want_series: bool = True) -> dict:
        """``process_batch`` of a plan with the rescaled-range Hurst exponent that also hands back what the Hurst kernel
        formed (nmx_nolds_hurst_probe): ``"out"`` float32[n, row_width]; ``"scales"`` int[S] and ``"log_expected"``
        float64[S], the plan's tables; ``"RS"`` float64[n, n_series, C, S], (R/S)_n (NaN where no chunk was kept) and
        ``"kept"`` int32 of the same shape, the chunks kept; ``"hurst"`` float64 (H, before the sum rule), ``"sum_zero"``
        (bool) and ``"n_kept"`` (scales that are not NaN), each [n, n_series, C]; ``"series"`` float32[n, n_series, C, W]:
        the samples the kernel read."""
        data = np.asarray(data)
        if data.ndim != 2 or data.shape[0] != self.C_in:
            raise ValueError(f"expected data with {self.C_in} rows, got {data.shape}")
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        dc = self._host_offsets(data)
        x = np.ascontiguousarray(data if dc is None else np.asarray(data, np.float64) - dc[:, None], dtype=np.float32)
        n, S = len(starts), int(self.desc.nolds_raw) + int(self.desc.nolds_n_bands)
        K = int(self.desc.nolds_hurst_n_scales)
        out = np.empty((n, self.row_width), np.float32)
        rs, hurst = np.zeros((n, S, self.C, K), np.float64), np.zeros((n, S, self.C), np.float64)
        kept_chunks = np.zeros((n, S, self.C, K), np.int32)
        zero, kept = np.zeros((n, S, self.C), np.uint8), np.zeros((n, S, self.C), np.int32)
        series = np.zeros((n, S, self.C, self.W), np.float32) if want_series else None
        self.lib.check(self.lib.lib.nmx_nolds_hurst_probe(
            self._plan, x.ctypes.data, _ld(x), x.shape[1], starts.ctypes.data, n, out.ctypes.data, rs.ctypes.data,
            kept_chunks.ctypes.data, hurst.ctypes.data, zero.ctypes.data, kept.ctypes.data,
            series.ctypes.data if series is not None else None))
        scales = np.array([self.desc.nolds_hurst_scales[k] for k in range(K)], np.int64)
        log_e = np.array([self.desc.nolds_hurst_log_expected[k] for k in range(K)], np.float64)
        return {"out": out, "scales": scales, "log_expected": log_e, "RS": rs, "kept": kept_chunks, "hurst": hurst,
                "sum_zero": zero.astype(bool), "n_kept": kept, "series": series}

    def timing_ms(self, which: int = 0) -> float:
        ms = C.c_float()
        self.lib.check(self.lib.lib.nmx_last_timing_ms(self._plan, which, C.byref(ms)))
        return float(ms.value)

    def kernels(self, which: int) -> str:
        """Kernels the last batch -- or the last ``preprocess_window`` / ``filter_window`` call -- launched in stage ``which`` (1 prep, 2 time/osc, 3 FIR bank, 4 bursts,
        5 sharp waves, 6 the FIR-bank filters left to a second launch: taps too long for the M = 1536 kernel,
        7 coherence, 8 grid projection, 10 nolds: its band filters and the sample-entropy, Hurst and DFA kernels), named as rocprofv3
        prints them.  ``which = 9``: the launch geometry of the
        channel-pair FIR kernels of that launch sequence, ``"<kernel>: <n> pairs, <workgroups> x <waves> waves"``."""
        buf = C.create_string_buffer(512)
        self.lib.check(self.lib.lib.nmx_last_kernels(self._plan, which, buf, 512))
        return buf.value.decode()
