"""Per-window orchestrator: drop-in for ``DataProcessor`` (stream/data_processor.py:19-311)
plus a batch-of-windows entry point.

process(data[C_all, W]) reproduces, in order: NaN mask over all incoming rows (:253),
nan_to_num + channel pick (:255), pre-processors in PREPROCESSOR_DICT order filtered by
membership in settings.preprocessing (processing/data_preprocessor.py:9-15,45-51), all enabled
features in FeatureSelector order (features/feature_processor.py:45-84), feature normalisation
of the non-"psd" keys (:263-290), and the NaN policy: every key that CONTAINS the new_name of
a NaN channel becomes NaN (:297-306, substring match, reproduced as is).

Everything up to the features is ONE launch sequence on the GPU: the channel pick and the
re-reference matrix are folded into one [C, C_all] matrix applied on the device, notch runs per
window on the device, features read the result from HBM/LDS.

User-registered features (``add_custom_feature``, features/feature_processor.py:52-53,90-108) are
instantiated after the built-in ones and called on the host, hop by hop, with the pre-processed window
the device features read (``nmx_process_batch_tap``; the float64 window itself when nothing is enabled in
``settings.preprocessing`` and every channel is picked); their keys follow the built-in columns in
registration order and go through the same normaliser / NaN policy.
"""

from __future__ import annotations

import weakref
from time import time

import numpy as np

from . import channels as chmod
from . import file_writer as fw
from .engine import HotPathEngine, parallel_cast, table_empty
from .prep import LocalInput, PrepPlan
from .processing import DeviceFeatureNormalizer, FeatureNormalizer
from .projection import DeviceProjection, GridProjection
from .settings import NMSettings


class _LazyNanCols:
    """The NaN policy (stream/data_processor.py:297-306): every key that CONTAINS the new_name of a channel whose window
    held a NaN := NaN (substring match, as the reference).  A channel's columns are found on first use (256 channels x
    8 000 keys of substring tests cost 50 ms up front, and a NaN channel is the exception); ``keys`` is the orchestrator's
    own list, so the columns are looked up again once the plugin keys are appended to it (UserColumns)."""

    def __init__(self, keys, ch_names) -> None:
        self._keys, self._ch, self._cache = keys, ch_names, {}

    def __getitem__(self, ci: int) -> np.ndarray:
        cols = self._cache.get((ci, len(self._keys)))
        if cols is None:
            ch = self._ch[ci]
            cols = self._cache[ci, len(self._keys)] = np.array([i for i, k in enumerate(self._keys) if ch in k], dtype=int)
        return cols

    def apply(self, table: np.ndarray, mask: np.ndarray) -> np.ndarray:
        """The policy in place on the float64 ``table[n, len(keys)...]``; ``mask[n, channels]``: NaN per hop and channel."""
        if mask.any():
            if mask.shape[1] != len(self._ch):
                # the reference indexes ch_names_used with the mask over ALL rows (:300)
                raise IndexError("boolean index did not match: NaN handling needs every channel used")
            for ci in np.where(mask.any(axis=0))[0]:
                table[np.ix_(mask[:, ci], self[ci])] = np.nan
        return table


class UserColumns:
    """The user-registered features of one stream (features/feature_processor.py:52-53): instances built after the
    built-in features with the same ``(settings, ch_names, sfreq)``, called hop by hop on the host with the
    pre-processed window (``estimate_features``, :80-82).  ``keys`` is the orchestrator's column list: the first call
    appends the plugin keys to it (a key that repeats an earlier one overwrites that column, ``dict.update``).
    The plugin columns go through their own device normaliser (per-column statistics: splitting the table changes
    nothing) in float32 like the built-in columns."""

    def __init__(self, settings, ch_names, sfreq, keys: list, device: int = 0, lib=None) -> None:
        self.settings, self.ch_names, self.sfreq, self.keys = settings, list(ch_names), sfreq, keys
        self.device, self.lib = int(device), lib
        self.user_keys: list[str] | None = None
        self.cols: np.ndarray | None = None
        self.norm = None
        self._instantiate()

    def _instantiate(self) -> None:
        from . import user_features as registered

        self.features = {name: cls(self.settings, self.ch_names, self.sfreq) for name, cls in registered.items()}

    def reset(self) -> None:
        """Fresh instances and history, like the reference's new FeatureProcessors per DataProcessor."""
        self._instantiate()
        if self.norm is not None:
            self.norm.reset()

    def rows(self, windows) -> np.ndarray:
        """windows: iterable of float64 [C, W] pre-processed windows in hop order -> float64 [n, n_user]."""
        rows = []
        for w in windows:
            d: dict = {}
            for f in self.features.values():
                d.update(f.calc_feature(w))
            if self.user_keys is None:
                self.user_keys = list(d)
                col = {k: i for i, k in enumerate(self.keys)}
                n0 = len(self.keys)
                new = [k for k in self.user_keys if k not in col]
                self.keys.extend(new)
                col.update({k: n0 + i for i, k in enumerate(new)})
                self.cols = np.array([col[k] for k in self.user_keys], dtype=np.int64)
                st = self.settings
                if st.postprocessing.feature_normalization:
                    mask = None
                    if not st.feature_normalization_settings.normalize_psd:
                        mask = np.array(["psd" not in k for k in self.user_keys], dtype=np.uint8)
                    self.norm = DeviceFeatureNormalizer(st, len(self.user_keys), colmask=mask, device=self.device,
                                                        lib=self.lib)
            if list(d) != self.user_keys:
                raise ValueError("a user feature changed its keys between hops: "
                                 f"{sorted(set(d) ^ set(self.user_keys))[:4]}")
            rows.append(np.fromiter(d.values(), dtype=np.float64, count=len(d)))
        out = np.stack(rows) if rows else np.empty((0, len(self.user_keys or [])))
        if self.norm is not None and len(out):
            out = self.norm.process_batch(out).astype(np.float64)
        return out

    def merge(self, table: np.ndarray, user: np.ndarray) -> np.ndarray:
        """``user`` (from `rows`) into its columns of the float64 ``table``: in place, or in a copy widened to every key
        when the table holds only the built-in columns."""
        if table.shape[1] < len(self.keys):
            wide = np.empty((table.shape[0], len(self.keys)), np.float64)
            wide[:, :table.shape[1]] = table
            table = wide
        if user.shape[0]:
            table[:, self.cols] = user     # after the built-in values: dict.update overwrites a repeated key
        return table


class PostChain:
    """Everything behind the engine's rows, ONE object per processor family (the twins of other window lengths share it):
    the feature normaliser, the grid projection (host plan ``proj``, device object ``proj_dev`` for the engine's key
    layout), the ``user`` columns, the key list and the NaN-column scanner.  ``where`` records where each step runs:

        step         where      when
        normalizer   "engine"   feature_normalization on (inside the plan's launch sequence: no second round trip)
                     "host"     after `detach`: a ragged run normalises the merged table, sequentially over ALL hops
        projection   "engine"   behind an in-engine normaliser, or with no normaliser (it reads normalised rows)
                     "host"     after `detach`, on the engine's rows behind the host normaliser
                     "merged"   user features exist: their keys come first, the grid follows on the merged table
        (None: the step does not exist.  A channel shard has no user features: its coordinator's chain holds them.)"""

    def __init__(self, settings, ch_names, proj=None, plugins: bool = False, device: int = 0, lib=None) -> None:
        self.settings, self.ch_names, self.proj, self.plugins = settings, ch_names, proj, plugins
        self.device, self.lib = device, lib
        self.keys = self.user = self.normalizer = self.proj_dev = self._user_grid = self._nan_cols = None
        self.n_feat, self._engines = 0, weakref.WeakSet()   # (`start` fills the first; the engines `attach` was handed)
        self.where = {"normalizer": None, "projection": "merged" if proj is not None and plugins else None}

    def extra_cols(self, keys) -> int:
        """The grid columns behind the built-in ones in the engine's rows (known when the plan is built)."""
        return self.proj.layout(keys).n_grid if self.proj is not None and not self.plugins else 0

    def start(self, feat_keys, names, sfreq, dry_run: bool = False, normalize: bool = True) -> None:
        """The key list and the objects of the chain, from the engine's keys."""
        st = self.settings
        self.n_feat, self.keys = len(feat_keys), list(feat_keys)
        # with user features their keys come first, and the grid follows on the merged table (`finish_table`)
        layout = self.proj.layout(feat_keys) if self.proj is not None and not self.plugins else None
        if layout is not None:
            self.keys += layout.grid_keys
        # user features: instantiated after the built-ins with the same arguments (feature_processor.py:45-53)
        if self.plugins:
            self.user = UserColumns(st, names, sfreq, self.keys, device=self.device, lib=self.lib)
        if normalize and st.postprocessing.feature_normalization and not dry_run:
            FeatureNormalizer(st)   # an unknown method name raises NotImplementedError here, naming it
            # every method of normalization.py:57-70: one HIP scan per batch of hops; the column mask carries the
            # "psd" exclusion (stream/data_processor.py:263-290); the feature columns, not the grid columns behind them
            mask = None
            if not st.feature_normalization_settings.normalize_psd:
                mask = np.array(["psd" not in k for k in feat_keys], dtype=np.uint8)
            self.normalizer = DeviceFeatureNormalizer(st, len(feat_keys), colmask=mask, device=self.device, lib=self.lib)
            self.where["normalizer"] = "engine"
        if layout is not None and layout.n_grid and not dry_run:
            self.proj_dev = DeviceProjection(layout, self.device, self.lib)   # (stateless: one for every twin)
            self.where["projection"] = "engine"
        self._nan_cols = _LazyNanCols(self.keys, self.ch_names)

    def attach(self, engine) -> None:
        """The steps placed in the engine into ``engine``'s launch sequence."""
        self.lib = engine.lib
        self._engines.add(engine)
        if self.where["normalizer"] == "engine":
            engine.attach_normalizer(self.normalizer)
        if self.where["projection"] == "engine":
            engine.attach_projection(self.proj_dev)

    def detach(self) -> None:
        """Out of EVERY engine of the family (they share ``where``): both steps run in `finish` from now on (a ragged run)."""
        for engine in self._engines:
            if engine._norm is not None:
                engine.attach_normalizer(None)
            if engine._proj is not None:
                engine.attach_projection(None)
        self.where.update({k: "host" for k, v in self.where.items() if v == "engine"})

    def reset(self) -> None:
        if self.normalizer is not None:
            self.normalizer.reset()
        if self.user is not None:
            self.user.reset()

    def table(self, out: np.ndarray) -> np.ndarray:
        """Engine rows ``float32[n, row_width]`` in hop order -> the float64 table: the normaliser and the grid projection
        (unless they ran inside the engine), the cast."""
        F = self.n_feat
        if self.where["normalizer"] == "host":
            if out.shape[1] == F:
                out = self.normalizer.process_batch(out)
            else:   # (the grid columns behind the features)
                out = np.array(out, dtype=np.float32, order="C")
                out[:, :F] = self.normalizer.process_batch(out[:, :F])
        if self.where["projection"] == "host" and out.shape[1] > F:
            out = np.require(out, np.float32, "C")
            self.proj_dev.process(out)
        if len(out) == 1:   # (one hop, `process`: the pooled table and the threaded cast cost more than they save)
            return out.astype(np.float64)
        table = table_empty(out.shape)
        parallel_cast(table, out, None, self.lib)
        return table

    def finish_table(self, table: np.ndarray, mask: np.ndarray, user: np.ndarray | None = None) -> np.ndarray:
        """The user columns and their projection into the float64 ``table``, then the NaN policy (last: the plugin and grid
        keys follow it too)."""
        if user is not None:
            table = self.user.merge(table, user)
            if self.proj is not None:
                # the grid behind the user columns (dict.update after the plugin keys): laid out at the first hop, when the
                # plugin keys are known (Projection.init_projection_run), its keys appended to the list the NaN policy scans
                if self._user_grid is None:
                    lay = self.proj.layout(self.keys)
                    self._user_grid = (lay, DeviceProjection(lay, self.device, self.lib) if lay.n_grid else None)
                    self.keys.extend(lay.grid_keys)
                if self._user_grid[1] is not None:
                    table = self._user_grid[1].process_table(table)
        return self._nan_cols.apply(table, mask)

    def finish(self, out: np.ndarray, mask: np.ndarray, user: np.ndarray | None = None) -> np.ndarray:
        return self.finish_table(self.table(out), mask, user)


class LengthTable:
    """One processor per window length (a sampling rate that is not a whole number of samples per segment: the reference's
    generator cuts two lengths, stream/generator.py:41-53, and its DataProcessor takes whatever arrives), who ran last,
    and the hand-over: what carries over from hop to hop (burst history, Kalman filters, raw-normaliser history; the
    layout depends on sfreq and the settings, not on the length: nmx_state_export / _import) goes from whoever ran last
    into the next where the length changes.  Two drivers: ``DataProcessor.process`` hop by hop over twins that share one
    PostChain, and `run_ragged` for ``Stream.run`` / ``ShardedStream``.  ``make(n_samples)`` builds a new length's."""

    def __init__(self, make, first=None) -> None:
        self.make, self.by_len, self.last = make, {}, first
        if first is not None:
            self.by_len[first.engine.W_in] = first

    def of(self, n_samples: int):
        if n_samples not in self.by_len:
            self.by_len[n_samples] = self.make(n_samples)
        return self.by_len[n_samples]

    @staticmethod
    def plans(p) -> list:
        """The processors that hold a plan: ``p`` itself, or the parts of a MultiDeviceProcessor (one state blob each)."""
        return getattr(p, "parts", [p])

    def switch(self, n_samples: int):
        """The processor for windows of ``n_samples``, holding the state of whoever ran last."""
        p, cur = self.of(n_samples), self.last
        if cur is not None and cur is not p:
            for src, dst in zip(self.plans(cur), self.plans(p)):
                state = src.engine.export_state()
                if state:
                    dst.engine.import_state(state)
            p.cnt_samples = cur.cnt_samples
        self.last = p
        return p

    def run_ragged(self, lens: np.ndarray, run) -> list:
        """The hops in order as consecutive runs of one length, ``run(processor, a, b)`` computing hops [a, b); the
        post-processing is detached from every engine first (PostChain).  -> the results of ``run`` in hop order."""
        for w in sorted(set(int(v) for v in lens)):
            for q in self.plans(self.of(w)):
                q.chain.detach()
        cuts = [0] + [i for i in range(1, len(lens)) if lens[i] != lens[i - 1]] + [len(lens)]
        return [run(self.switch(int(lens[a])), a, b) for a, b in zip(cuts[:-1], cuts[1:])]


def no_sharded_projection(settings) -> None:
    """A grid point mixes the features of channels of every shard: the projection needs them all in one plan."""
    pp = settings.postprocessing
    if pp.project_cortex or pp.project_subcortex:
        raise NotImplementedError("grid projection (project_cortex / project_subcortex) needs every channel in one plan: "
                                  "it is not supported with channels sharded over several devices (use one device)")


class UserViews:
    """``user_features`` / ``user_keys`` (features/feature_processor.py:52-53,80-82) of a processor whose ``chain`` holds them."""

    @property
    def user_features(self) -> dict:
        return self.chain.user.features if self.chain.user is not None else {}

    @property
    def user_keys(self):
        return self.chain.user.user_keys if self.chain.user is not None else None


class DataProcessor(UserViews):
    def __init__(self, sfreq: float, settings, channels, coord_names=None, coord_list=None,
                 line_noise: float | None = None, path_grids=None, verbose: bool = True,
                 device: int = 0, window: int | None = None, lib=None,
                 channel_subset=None, dry_run: bool = False,
                 resample_features_at_new_rate: bool = False, local_inputs: bool = False,
                 staging_slot: int = 0, _family: tuple | None = None, resample_npad=None, nolds_fit=None) -> None:
        """``resample_npad``: the padding of raw_resampling, ``"auto"`` (the default) or an int >= 0 samples per side; 100 is
        what the reference's call of ``mne.filter.resample`` gets (plan_desc.resample_npad_arg; None: NMX_RESAMPLE_NPAD).

        ``nolds_fit``: ``"poly"`` lets nolds' detrended_fluctuation_analysis run, its final line fitted by least squares;
        a mapping ``{measure: "poly" | "RANSAC" | None}`` says it per measure and is what lets hurst_exponent run
        (plan_desc.nolds_fit_arg; None: NMX_NOLDS_FIT, and without it the measures raise as the unseeded RANSAC fit has it).

        ``_family``: (PrepPlan, PostChain, LengthTable) of the processor this one is the twin of for another window
        length (`_twin`): the twin takes them instead of building its own.

        ``coord_names`` / ``coord_list`` / ``path_grids``: the contacts' coordinates and the directory of grid_cortex.tsv /
        grid_subcortex.tsv for the grid projection (postprocessing.project_cortex / project_subcortex,
        processing/projection.py); ``path_grids=None`` takes the grids of an installed reference package."""
        from . import user_features as _registered

        self.settings = st = NMSettings.load(settings)
        self.channels = chmod.load_channels(channels)
        # (what a twin for another window length is built from: `process` under the reference's own loop, below)
        self._ctor = dict(sfreq=sfreq, line_noise=line_noise, verbose=verbose, device=device, lib=lib,
                          resample_features_at_new_rate=resample_features_at_new_rate, staging_slot=staging_slot,
                          resample_npad=resample_npad, nolds_fit=nolds_fit)
        self._twin_ok = channel_subset is None and not dry_run and not local_inputs
        self.sfreq_features, self._sfreq_raw_orig = st.sampling_rate_features_hz, sfreq
        self.line_noise, self.verbose = line_noise, verbose
        projecting = st.postprocessing.project_cortex or st.postprocessing.project_subcortex
        if channel_subset is not None:
            no_sharded_projection(st)
        if _family is None:
            proj = GridProjection(st, self.channels, coord_names, coord_list, path_grids) if projecting else None
            prep = PrepPlan(st, self.channels, sfreq, line_noise, resample_features_at_new_rate, resample_npad)
            # (a channel shard leaves the user features to its coordinator, sharding.MultiDeviceProcessor: they see ALL channels)
            plugins = bool(_registered and not dry_run and channel_subset is None)
            _family = (prep, PostChain(st, prep.ch_names_used, proj, plugins, device, lib), None)
        self.prep, self.chain, self._lengths = _family
        prep, chain = _family[:2]
        self.ch_names_used, self.feature_idx, self.target_idx = prep.ch_names_used, prep.feature_idx, prep.target_idx
        self.ref_matrix, self.sfreq_raw = prep.ref_matrix, prep.sfreq_design
        # channel sharding over GPUs: this processor computes the features of a subset of the
        # picked channels but its re-reference rows still read ALL input rows
        names, kw = self.ch_names_used, prep.engine_kwargs(window)
        self.local = None           # local_inputs: the LocalInput layout of this shard; its `rows` and `groups`:
        self.local_rows, self.local_groups = None, []
        if channel_subset is not None:
            subset = list(channel_subset)
            if ("coherence" in st.features.get_enabled() and st.coherence_settings.channels
                    and sorted(subset) != list(range(len(self.ch_names_used)))):
                # a pair may join channels of two shards; the plan of one shard sees its own channels only
                raise NotImplementedError("coherence needs both channels of every pair in one plan: it is not supported "
                                          "with channels sharded over several devices (use one device)")
            full = (prep.matrix if prep.matrix is not None else np.eye(len(self.channels)))[subset]
            names = [self.ch_names_used[i] for i in subset]
            if local_inputs:
                self.local = LocalInput(full)
                full, self.local_rows, self.local_groups = self.local.matrix, self.local.rows, self.local.groups
            kw["ref_matrix"] = full
        self.engine = HotPathEngine(st, names, device=device, lib=lib, dry_run=dry_run, staging_slot=staging_slot,
                                    extra_cols=chain.extra_cols, nolds_fit=nolds_fit, **kw)
        if chain.keys is None:
            chain.start(self.engine.keys, names, self.sfreq_raw, dry_run)
        if not dry_run:
            chain.attach(self.engine)
        # (the chain's own key list: plugin and grid keys are appended at the first hop; `projection`: the host plan or None)
        self.keys, self.device_normalizer, self.projection = chain.keys, chain.normalizer, chain.proj
        self._user_chunk = 64                          # hops per tapped batch (bounds the [n, C, W] hand-back)
        self._row_template = self.settings_token = None
        self.cnt_samples = 0

    # -- stream/data_processor.py:313-351: what the reference's Stream calls after its loop ---------------------------------
    def save_sidecar(self, out_dir, prefix: str = "", additional_args: dict | None = None) -> None:
        sidecar = {"original_fs": self._sfreq_raw_orig, "final_fs": self.sfreq_raw, "sfreq": self.sfreq_features}
        fw.save_sidecar(sidecar | self.projection_sidecar() | (additional_args or {}), out_dir, prefix)

    def projection_sidecar(self) -> dict:
        """What the grid projection adds to the sidecar (stream/data_processor.py:326-333): coords, grid_cortex,
        proj_matrix_cortex, grid_subcortex, proj_matrix_subcortex; {} without a projection."""
        return self.chain.proj.sidecar() if self.chain.proj is not None else {}

    def save_settings(self, out_dir, prefix: str = "") -> None:
        self.settings.save(out_dir, prefix)

    def save_channels(self, out_dir, prefix: str) -> None:
        fw.save_channels(self.channels, out_dir, prefix)

    def save_features(self, feature_arr, out_dir="", prefix: str = "") -> None:
        fw.save_features(feature_arr, out_dir, prefix)

    def reset(self) -> None:
        """Forget everything carried across hops (burst history, Kalman filters, raw and feature normaliser
        histories): the state of a freshly constructed processor."""
        self.engine.reset_state()
        if self._lengths is not None:   # (the twins of other window lengths take their state from whoever ran last)
            for p in self._lengths.by_len.values():
                p.engine.reset_state()
            self._lengths.last = self
        self.chain.reset()
        self.cnt_samples = 0

    # -- user-registered features (features/feature_processor.py:52-53,80-82) ----------------------
    def process_batch_tapped(self, data: np.ndarray, starts: np.ndarray):
        """One batch through the engine AND the windows its features read: (float32 rows -- normalised when the
        normaliser is attached --, NaN mask, float64 [n, C, W])."""
        eng = self.engine
        if eng.preprocessing_is_identity:
            o, m = eng.process_batch(data, starts, want_nan_mask=True)
            return o, m, np.stack([np.nan_to_num(np.asarray(data[:, int(s):int(s) + eng.W_in], dtype=np.float64)) for s in starts])
        o, m, pre = eng.process_batch(data, starts, want_nan_mask=True, tap=True)
        return o, m, pre.astype(np.float64)

    def _process_batch_user(self, data: np.ndarray, starts: np.ndarray):
        """Engine rows, NaN mask and the user-feature rows of the same hops; the hops go through the engine in chunks
        of ``_user_chunk`` so that the tapped windows stay small."""
        user = self.chain.user
        starts = np.asarray(starts, dtype=np.int64)
        if len(starts) == 0:   # (an empty batch is an empty table, as without plugins)
            return (np.empty((0, self.engine.n_outputs), np.float32), np.zeros((0, self.engine.C_in), bool),
                    np.empty((0, len(user.user_keys or [])), np.float64))
        outs, masks, users = [], [], []
        for i in range(0, len(starts), self._user_chunk):
            o, m, wins = self.process_batch_tapped(data, starts[i:i + self._user_chunk])
            outs.append(o)
            masks.append(m)
            users.append(user.rows(wins))
        return np.concatenate(outs), np.concatenate(masks), np.concatenate(users)

    def _row_dict(self, row: np.ndarray) -> dict:
        """{key: float} in the reference's key order (stream/data_processor.py:238-311 returns a dict).  Built from a template
        that already holds the keys: copying a 10 000-entry dict and overwriting its values costs 0.43 ms where
        ``dict(zip(keys, values))`` -- which grows its table eleven times on the way -- costs 0.72 (the engine's part of a
        256-channel call is 0.36 ms)."""
        keys = self.keys
        tmpl = self._row_template
        if tmpl is None or tmpl[0] is not keys or len(tmpl[1]) != len(keys):
            tmpl = self._row_template = (keys, dict.fromkeys(keys, 0.0), tuple(keys))
        if len(tmpl[1]) != len(tmpl[2]):   # (duplicate keys: nothing a template can hold)
            return dict(zip(keys, row.tolist()))
        d = tmpl[1].copy()
        d.update(zip(tmpl[2], row.tolist()))
        return d

    def _twin(self, n_samples: int) -> "DataProcessor":
        """The twin for windows of ``n_samples``: one plan per length, ONE PostChain (feature normaliser, user features)
        and one table of lengths serve them all."""
        if not self._twin_ok:
            raise ValueError(f"expected windows of {self.engine.W_in} samples, got {n_samples}")
        return DataProcessor(settings=self.settings, channels=self.channels, window=n_samples,
                             _family=(self.prep, self.chain, self._lengths), **self._ctor)

    def process(self, data: np.ndarray) -> dict:
        n_samples = np.shape(data)[-1]
        if n_samples != self.engine.W_in or (self._lengths is not None and self._lengths.last is not self):
            if self._lengths is None:
                self._lengths = LengthTable(self._twin, self)
            p = self._lengths.switch(n_samples)
            if p is not self:
                return p.process(data)
        start_time = time()
        if self.chain.user is not None:
            out, mask, user = self._process_batch_user(np.asarray(data), np.zeros(1, np.int64))
        else:
            out, mask = self.engine.process_window(data, want_nan_mask=True)
            out, mask, user = out[None], mask[None], None
        row = self.chain.finish(out, mask, user)[0]   # (a table of one hop)
        if self.verbose:
            from . import logger

            logger.info("Last batch took: %.3f seconds to process", time() - start_time)
        return self._row_dict(row)

    def process_batch(self, data: np.ndarray, starts: np.ndarray, spare_cols: int = 0) -> np.ndarray:
        """data[C_all, T], window start samples -> float64[n, n_features] (same post-processing,
        applied hop by hop because the normaliser is sequential).  ``spare_cols``: the table MAY come back with that
        many extra columns behind the features (HotPathEngine.process_batch_f64) -- the caller checks the shape."""
        if self.chain.user is not None:
            return self.chain.finish(*self._process_batch_user(data, starts))
        if self.chain.where["normalizer"] != "host":
            # nothing left to do on the host but the NaN policy: conversions pipelined against the device
            rows, mask = self.engine.process_batch_f64(data, starts, want_nan_mask=True, spare_cols=spare_cols)
            return self.chain.finish_table(rows, mask)
        return self.chain.finish(*self.engine.process_batch(data, starts, want_nan_mask=True, staged_output=True))

    # -- the ragged runs of `Stream.run`: the hops cut into consecutive runs of one length, one processor per length
    # (LengthTable.run_ragged)
    def ragged_run(self, data: np.ndarray, starts: np.ndarray):
        """One run of equal-length hops -> (float32 engine rows, NaN mask, pre-processed windows or None)."""
        if self.chain.user is not None:
            return self.process_batch_tapped(data, starts)
        return (*self.engine.process_batch(data, starts, want_nan_mask=True), None)

    def ragged_finish(self, runs) -> np.ndarray:
        """The runs of `ragged_run` in hop order -> the float64 table (normaliser, user columns, NaN policy)."""
        # one set of user-feature instances sees every hop in order, like the reference
        user = self.chain.user.rows([w for r in runs for w in r[2]]) if self.chain.user is not None else None
        return self.chain.finish(np.concatenate([r[0] for r in runs]), np.concatenate([r[1] for r in runs]), user)

