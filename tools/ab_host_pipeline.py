"""A/B of the Python host pipeline: two trees of the package, the same scenarios, results compared bit for bit.

    python tools/ab_host_pipeline.py PARENT NEW --lib emu|gpu [--only 1,6] [--same]

PARENT / NEW: two checkouts (e.g. a ``git worktree`` of the parent commit and the working tree; the directory that holds
``py_neuromodulation_amd``, or that package directory itself).  Every scenario runs once per tree in a fresh child process
(the module name is the same in both) and hands back {label: {keys, table, NaN mask, state, ...}} as bytes; the parent
process compares field by field, prints a table and exits non-zero at the first scenario that differs.  ``--lib emu``: the
single-thread emulator of tests/emu (built from THIS tree: the device code is the same in both); ``--lib gpu``: each tree's
own libnmx.so.  ``--same``: PARENT against itself twice (what is non-deterministic to begin with).  A scenario that
raises records the exception text: both trees must raise the same.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import pickle
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]   # the tree of this tool: tests/user_plugins.py, tests/golden, the emulator
SFREQ, RAGGED = 1000.0, 1111.111


# ---- inputs -----------------------------------------------------------------------------------------------------------
def table(names, reref, used, types):
    import pandas as pd

    return pd.DataFrame({"name": names, "rereference": reref, "used": used, "target": [0] * len(names), "type": types,
                         "status": ["good"] * len(names), "new_name": names})


def six_channels():
    """Four ECoG with a common average, one bipolar LFP, one unused."""
    return table(["ECOG_1", "ECOG_2", "ECOG_3", "ECOG_4", "LFP_1", "EMG_1"],
                 ["average"] * 4 + ["ECOG_4", "None"], [1] * 5 + [0], ["ecog"] * 4 + ["lfp", "emg"])


def five_channels():
    """The used rows of `six_channels` alone: a NaN sample then goes through the NaN policy instead of raising."""
    return six_channels().iloc[:5].reset_index(drop=True)


def seven_channels():
    """Two type groups (five ECoG: a group sum; two LFP) and one bipolar row."""
    return table([f"ECOG_{i}" for i in range(1, 6)] + ["LFP_1", "LFP_2"], ["average"] * 5 + ["LFP_2", "average"], [1] * 7,
                 ["ecog"] * 5 + ["lfp"] * 2)


def recording(n_ch, T, sfreq, seed=7, nan=True):
    rng = np.random.default_rng(seed)
    t = np.arange(T) / sfreq
    x = np.stack([(1 + 0.6 * np.sin(2 * np.pi * 0.3 * t + c)) * 30 * np.sin(2 * np.pi * (11 + 6 * c) * t) for c in range(n_ch)])
    x += rng.standard_normal((n_ch, T)) * 5 + rng.uniform(-300, 300, (n_ch, 1))
    if nan:
        x[1, T // 2] = np.nan
    return x


def settings(norm=True, **features):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()   # (bursts and sharp waves are on by default)
    for k, v in features.items():
        setattr(s.features, k, v)
    s.postprocessing.feature_normalization = norm
    return s


def schedule(T, sfreq, s):
    from py_neuromodulation_amd.generator import window_schedule

    return window_schedule(T, sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)


# ---- what a run hands back ------------------------------------------------------------------------------------------
def pack(keys, tab, state=None, **more):
    tab = np.ascontiguousarray(tab, dtype=np.float64)
    out = {"keys": list(keys), "shape": tab.shape, "table": tab.tobytes(), "nan_mask": np.isnan(tab).tobytes()}
    if state is not None:
        out["state"] = b"|".join(state) if isinstance(state, list) else bytes(state)
    out.update(more)
    return out


def guarded(out, label, fn):
    try:
        out[label] = fn()
    except Exception as e:   # noqa: BLE001 -- compared like a result
        out[label] = {"raised": f"{type(e).__name__}: {e}"}


def three_ways(out, tag, sfreq, ch, s, data, lib, tmp, n_hop=None, **kw):
    """`Stream.run`, `DataProcessor.process_batch` and `process` hop by hop."""
    from py_neuromodulation_amd import DataProcessor, Stream

    starts, lens, _ = schedule(data.shape[1], sfreq, s)

    def stream():
        df = Stream(sfreq, ch, settings=s, lib=lib, line_noise=50, **kw).run(data, out_dir=tmp, save_csv=False)
        return pack(df.columns, df.to_numpy(dtype=np.float64))

    def batch():
        dp = DataProcessor(sfreq, s, ch, line_noise=50, lib=lib, verbose=False, **kw)
        rows = dp.process_batch(data, starts)
        return pack(dp.keys, rows[:, :len(dp.keys)], dp.engine.export_state())

    def hops():
        dp = DataProcessor(sfreq, s, ch, line_noise=50, lib=lib, verbose=False, **kw)
        cut = list(zip(starts, lens))[:n_hop]
        rows = [dp.process(data[:, a:a + n]) for a, n in cut]
        # ({W_in: twin}: `_lengths.by_len`; `_by_len` in trees before the length table)
        twins = getattr(getattr(dp, "_lengths", None), "by_len", None) or getattr(dp, "_by_len", None) or {int(cut[-1][1]): dp}
        return pack(rows[0], [list(r.values()) for r in rows], twins[int(cut[-1][1])].engine.export_state(), n_plans=len(twins))

    guarded(out, tag + " stream", stream)
    if len(set(lens.tolist())) == 1:
        guarded(out, tag + " batch", batch)
    guarded(out, tag + " hops", hops)


# ---- scenarios ------------------------------------------------------------------------------------------------------
def scenario_1(lib, tmp):
    out, ch = {}, six_channels()
    for norm in (True, False):
        three_ways(out, f"norm={norm}", SFREQ, ch, settings(norm), recording(6, 2100, SFREQ, nan=False), lib, tmp)
    three_ways(out, "NaN, unused row", SFREQ, ch, settings(True), recording(6, 1300, SFREQ), lib, tmp)
    three_ways(out, "NaN, five used rows", SFREQ, five_channels(), settings(True), recording(5, 2100, SFREQ), lib, tmp)
    return out


def scenario_2(lib, tmp):
    out, ch = {}, six_channels()
    for norm in (True, False):
        s = settings(norm, bandpass_filter=True)
        s.bandpass_filter_settings.kalman_filter = True
        three_ways(out, f"norm={norm}", RAGGED, ch, s.validate(), recording(6, int(2.25 * RAGGED), RAGGED, nan=False), lib, tmp)
    three_ways(out, "NaN, five used rows", RAGGED, five_channels(), s.validate(), recording(5, int(2.25 * RAGGED), RAGGED), lib, tmp)
    return out


def scenario_3(lib, tmp):
    from py_neuromodulation_amd import DataProcessor
    from py_neuromodulation_amd import channels as chmod

    out, data = {}, recording(3, 1700, SFREQ)
    s = settings(True)
    s.preprocessing = ["raw_resampling", "notch_filter", "re_referencing", "raw_normalization"]
    s.raw_resampling_settings.resample_freq_hz = 500
    s, ch = s.validate(), chmod.get_default_channels_from_data(data)
    for new in (False, True):
        three_ways(out, f"new_rate={new}", SFREQ, ch, s, data, lib, tmp, resample_features_at_new_rate=new)
        guarded(out, f"new_rate={new} sidecar", lambda: {"final_fs": repr(DataProcessor(
            SFREQ, s, ch, line_noise=50, lib=lib, verbose=False, resample_features_at_new_rate=new).sfreq_raw)})
    return out


def scenario_4(lib, tmp):
    import py_neuromodulation_amd as nmx
    from py_neuromodulation_amd import channels as chmod
    from tests import user_plugins as up

    nmx.add_custom_feature("hop_stats", up.HopStats)
    out, data = {}, recording(3, 1000 + 69 * 100, SFREQ)   # 70 hops: one more than a tapped batch holds
    three_ways(out, "plugin", SFREQ, chmod.get_default_channels_from_data(data), settings(True, fft=True, welch=False,
               sharpwave_analysis=False), data, lib, tmp)
    return out


def scenario_5(lib, tmp):
    import pandas as pd
    import py_neuromodulation_amd as nmx
    from tests import user_plugins as up
    from tests.helpers import load_golden, settings_from_json

    g = load_golden("projection_c")
    grids = Path(tmp) / "grids"
    grids.mkdir()
    for name in ("cortex", "subcortex"):
        pd.DataFrame(g[f"grid_{name}"], columns=["x", "y", "z"]).to_csv(grids / f"grid_{name}.tsv", sep="\t", index=False)
    ch = pd.DataFrame(json.loads(str(g["channels_json"])))
    kw = dict(coord_names=json.loads(str(g["coord_names_json"])), coord_list=g["coord_list"].tolist(), path_grids=grids)
    sfreq = float(g["sfreq"])
    out, data = {}, recording(len(ch), int(1.5 * sfreq), sfreq, nan=False)
    for tag, norm, plugin in (("in engine", True, False), ("no normaliser", False, False), ("merged table", True, True)):
        s = settings_from_json(g["settings_json"])
        s.postprocessing.feature_normalization = norm
        for name, cls in (("channel_mean", up.ChannelMean), ("hop_stats", up.HopStats)):
            if plugin:
                nmx.add_custom_feature(name, cls)
            elif name in s.features:   # (the fixture's settings were dumped with the plugins registered)
                delattr(s.features, name)
        three_ways(out, tag, sfreq, ch, s, data, lib, tmp, n_hop=4, **kw)
        if not plugin:   # (the montage has a bad row: like the unused one of scenario 1, a NaN raises in the NaN policy)
            three_ways(out, tag + ", NaN", sfreq, ch, s, recording(len(ch), int(1.5 * sfreq), sfreq), lib, tmp, n_hop=4, **kw)
    return out


def scenario_6(lib, tmp):
    from py_neuromodulation_amd import Stream
    from py_neuromodulation_amd.sharding import MultiDeviceProcessor, ShardedStream

    out, ch = {}, seven_channels()
    s = settings(True)
    big, small = recording(7, 151000, SFREQ), recording(7, 2100, SFREQ)   # 7 x 151 000 samples: beyond pipeline_min

    def mdp(data, starts, local):
        p = MultiDeviceProcessor(SFREQ, s, ch, line_noise=50, devices=[0, 0, 0], lib=lib, local_input=local)
        rows = p.process_batch(data, starts)
        res = pack(p.keys, rows[:, :len(p.keys)], [q.engine.export_state() for q in p.parts], local_input=p.local_input,
                   h2d_rows=list(p.h2d_rows))
        p.close()
        return res

    for local in (True, False):
        guarded(out, f"70 hops pipelined local={local}", lambda: mdp(big, np.arange(70, dtype=np.int64) * 2150, local))
        guarded(out, f"12 hops local={local}", lambda: mdp(small, schedule(2100, SFREQ, s)[0], local))

    def ragged():
        df = Stream(RAGGED, ch, settings=s, lib=lib, line_noise=50, devices=[0, 0, 0]).run(
            recording(7, int(2.25 * RAGGED), RAGGED), out_dir=tmp, save_csv=False)
        return pack(df.columns, df.to_numpy(dtype=np.float64))

    guarded(out, "ragged 1111.111 Hz", ragged)
    for rank in range(3):
        def shard():
            st = ShardedStream(SFREQ, ch, settings=s, rank=rank, world_size=3, device=0, lib=lib, local_input=True)
            d = st._dp.engine.desc
            R = np.ctypeslib.as_array(d.ref_matrix, shape=(int(d.n_channels) * int(d.n_channels_in),)) if d.ref_matrix else np.zeros(0)
            return {"local_rows": list(st.local_rows), "owned_rows": list(st.owned_rows), "ref_matrix": R.tobytes(),
                    "keys": list(st._dp.keys)}
        guarded(out, f"ShardedStream dry run rank {rank}", shard)
    return out


def _zero_pointers(obj):
    for name, typ in obj._fields_:
        v = getattr(obj, name)
        if isinstance(v, C.Structure):
            _zero_pointers(v)
        elif isinstance(v, C.Array):
            for i, e in enumerate(v):
                if isinstance(e, C.Structure):
                    _zero_pointers(e)
                elif isinstance(e, C._Pointer):
                    v[i] = type(e)()
        elif isinstance(v, C._Pointer) or typ is C.c_void_p:
            setattr(obj, name, typ())


def scenario_7(lib, tmp):
    from py_neuromodulation_amd.engine import HotPathEngine

    out, names = {}, ["ECOG_1", "ECOG_2", "LFP_1"]
    everything = settings(True, bandpass_filter=True, stft=True, coherence=True)
    everything.coherence_settings.channels = [["ECOG_1", "LFP_1"], ["ECOG_2", "LFP_1"]]
    everything.bandpass_filter_settings.kalman_filter = True
    spectrum = settings(True, stft=True)
    for name in ("fft_settings", "welch_settings", "stft_settings"):
        spectrum[name].return_spectrum = True
    for tag, s, kw in (("every family", everything.validate(), {}), ("return_spectrum", spectrum.validate(), {}),
                       ("resampled, raw norm", settings(True), dict(resample_from=1000.0, resample_to=500.0, raw_window=1000,
                                                                   raw_norm=("zscore", 3, 30000, 100)))):
        def dry():
            eng = HotPathEngine(s, names, 1000.0, dry_run=True, **kw)
            d = type(eng.desc).from_buffer_copy(bytes(eng.desc))
            _zero_pointers(d)
            return {"keys": list(eng.keys), "desc": bytes(d), "taps": b"".join(t.tobytes() for t in eng.filter_taps),
                    "coh_pairs": repr(eng.coh_pairs), "geometry": repr((eng.W, eng.W_in, eng.resample_ratio, eng.C_in))}
        guarded(out, tag, dry)
    return out


SCENARIOS = {1: scenario_1, 2: scenario_2, 3: scenario_3, 4: scenario_4, 5: scenario_5, 6: scenario_6, 7: scenario_7}


# ---- the two processes ----------------------------------------------------------------------------------------------
def root_of(path) -> Path:
    p = Path(path).resolve()
    return p.parent if p.name == "py_neuromodulation_amd" else p


def child(args) -> None:
    sys.path[:0] = [str(root_of(args.child))]
    sys.path.append(str(HERE))
    from py_neuromodulation_amd import _lib

    import py_neuromodulation_amd

    assert Path(py_neuromodulation_amd.__file__).resolve().parent.parent == root_of(args.child)
    if args.lib == "emu":
        import importlib.util

        spec = importlib.util.spec_from_file_location("_ab_graft_entry", HERE / "__graft_entry__.py")
        ge = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ge)
        lib = _lib.NmxLibrary(ge.build_emu())
    else:
        lib = _lib.get_library()
    with tempfile.TemporaryDirectory() as tmp:
        res = SCENARIOS[args.scenario](lib, tmp)
    Path(args.out).write_bytes(pickle.dumps(res))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trees", nargs="*")
    ap.add_argument("--lib", choices=["emu", "gpu"], default="emu")
    ap.add_argument("--only", default="")
    ap.add_argument("--same", action="store_true")
    ap.add_argument("--timeout", type=float, default=600.0)
    ap.add_argument("--child")
    ap.add_argument("--scenario", type=int)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    if len(args.trees) != 2:
        ap.error("two trees: PARENT NEW")
    trees = [str(root_of(t)) for t in (args.trees[0], args.trees[0] if args.same else args.trees[1])]   # (a child runs elsewhere)
    print(f"{'scenario':8s} {'run':44s} {'field':10s} result")
    fields = 0
    for n in [int(v) for v in args.only.split(",") if v] or sorted(SCENARIOS):
        got = []
        with tempfile.TemporaryDirectory() as tmp:
            for i, tree in enumerate(trees):
                out = Path(tmp) / f"{i}.pkl"
                subprocess.run([sys.executable, __file__, "--child", tree, "--scenario", str(n), "--lib", args.lib, "--out",
                                str(out)], check=True, timeout=args.timeout, cwd=tmp)
                got.append(pickle.loads(out.read_bytes()))
        a, b = got
        differ = list(a) != list(b)
        for label in a:
            for field in a[label]:
                same = label in b and field in b[label] and a[label][field] == b[label][field]
                differ |= not same
                fields += 1
                note = "identical" if same else "DIFFERENT"
                if field == "raised":
                    note += f" ({a[label][field][:70]})"
                elif field in ("shape", "n_plans", "local_input", "h2d_rows", "local_rows", "owned_rows", "geometry"):
                    note += f" ({a[label][field]})"
                print(f"{n:<8d} {label:44s} {field:10s} {note}")
        if differ:
            print(f"scenario {n}: the trees differ")
            return 1
    print(f"every scenario the same in both trees: {fields} fields compared")
    return 0


if __name__ == "__main__":
    sys.exit(main())
