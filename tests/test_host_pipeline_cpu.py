"""The host pipeline's three seams -- PrepPlan / LocalInput, PostChain, LengthTable -- on the CPU (emulator where a
library is needed)."""

import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

RAGGED = 1111.111   # Hz: the generator cuts windows of 1111 and 1112 samples


@pytest.fixture(scope="module")
def emu_lib():
    import __graft_entry__ as ge
    from py_neuromodulation_amd import _lib

    return _lib.NmxLibrary(ge.build_emu())


def _table(names, reref, types):
    n = len(names)
    return pd.DataFrame({"name": names, "rereference": reref, "used": [1] * n, "target": [0] * n, "type": types,
                         "status": ["good"] * n, "new_name": names})


def seven_channels():
    """Two type groups (five ECoG with a common average: a group sum; two LFP) and one bipolar row."""
    return _table([f"ECOG_{i}" for i in range(1, 6)] + ["LFP_1", "LFP_2"], ["average"] * 5 + ["LFP_2", "average"],
                  ["ecog"] * 5 + ["lfp"] * 2)


def _fast(norm=True, **features):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_fast_compute()
    for k, v in features.items():
        setattr(s.features, k, v)
    s.postprocessing.feature_normalization = norm
    return s


def _recording(n_ch, T, seed=3):
    rng = np.random.default_rng(seed)
    t = np.arange(T) / 1000.0
    return np.stack([30 * np.sin(2 * np.pi * (9 + 7 * c) * t) for c in range(n_ch)]) + rng.standard_normal((n_ch, T)) * 4


# ---- PrepPlan / LocalInput ------------------------------------------------------------------------------------------
def test_prep_plan_and_local_input_of_three_shards():
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.prep import LocalInput, PrepPlan
    from py_neuromodulation_amd.sharding import channel_shard

    ch = seven_channels()
    prep = PrepPlan(NMSettings.get_default(), ch, 1000.0, line_noise=50)
    assert prep.order == ["notch_filter", "raw_resampling", "re_referencing"]
    assert prep.resample_to is None and prep.sfreq_design == 1000.0 and prep.raw_norm is None and prep.pre_taps is None
    assert prep.notch_taps is not None and prep.feature_idx == list(range(7))
    want = np.zeros((7, 7))
    want[:5, :5] = -0.25                       # the other four ECoG channels of the common average
    want[np.arange(7), np.arange(7)] = 1.0
    want[5, 6] = want[6, 5] = -1.0             # LFP_1 - LFP_2 (bipolar); LFP_2 minus the one other LFP channel (average)
    np.testing.assert_array_equal(prep.matrix, want)
    kw = prep.engine_kwargs(1000)
    assert kw["window"] == 1000 and kw["sfreq"] == 1000.0 and "resample_from" not in kw and kw["ref_matrix"] is prep.matrix

    shards = [channel_shard(7, 3, r) for r in range(3)]
    assert [list(s) for s in shards] == [[0, 1, 2], [3, 4], [5, 6]]
    a, b, c = (LocalInput(prep.matrix[list(s)]) for s in shards)
    # a row of the average: 1.25 on the channel itself, -0.25 times the sum of the whole group, as (hi, lo) row pair
    assert a.rows == [0, 1, 2] and a.pairs == [3] and a.n_rows == 5 and [g.tolist() for g in a.groups] == [[0, 1, 2, 3, 4]]
    np.testing.assert_array_equal(a.matrix, [[1.25, 0, 0, -0.25, -0.25], [0, 1.25, 0, -0.25, -0.25], [0, 0, 1.25, -0.25, -0.25]])
    assert b.rows == [3, 4] and b.pairs == [2] and b.n_rows == 4 and [g.tolist() for g in b.groups] == [[0, 1, 2, 3, 4]]
    np.testing.assert_array_equal(b.matrix, [[1.25, 0, -0.25, -0.25], [0, 1.25, -0.25, -0.25]])
    assert c.rows == [5, 6] and c.pairs == [] and c.n_rows == 2 and c.groups == []
    np.testing.assert_array_equal(c.matrix, [[1, -1], [-1, 1]])
    assert b.columns([4, 3]) == [1, 0]

    # the hi / lo rows of a sample range, and the way back of a NaN mask
    x = np.zeros((4, 6), np.float32)
    b.fill_pairs(x, [np.array([[1, 2], [3, 4]], np.float32)], 2, 4)
    np.testing.assert_array_equal(x, [[0] * 6, [0] * 6, [0, 0, 1, 2, 0, 0], [0, 0, 3, 4, 0, 0]])
    full = np.zeros((2, 7), bool)
    b.mask_to_all(np.array([[1, 0, 0, 0], [0, 1, 1, 1]], bool), full)       # (the pair rows never carry a NaN back)
    np.testing.assert_array_equal(full, [[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0]])


def test_identity_prep_and_contiguous_shard_need_no_matrix():
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.prep import LocalInput, PrepPlan

    s = NMSettings.get_default()
    s.preprocessing = ["notch_filter"]
    names = [f"c{i}" for i in range(7)]
    prep = PrepPlan(s, _table(names, ["None"] * 7, ["ecog"] * 7), 1000.0, line_noise=50)
    assert prep.matrix is None and prep.ref_matrix is None and prep.order == ["notch_filter"]
    loc = LocalInput(np.eye(7)[3:5])
    assert loc.rows == [3, 4] and loc.groups == [] and loc.pairs == [] and loc.matrix is None


def test_planning_needs_no_library(monkeypatch):
    from py_neuromodulation_amd import NMSettings, _lib
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.sharding import ShardedStream, global_keys

    def no_library():
        raise AssertionError("planning asked for the library")

    monkeypatch.setattr(_lib, "get_library", no_library)
    monkeypatch.setattr(_lib, "NmxLibrary", lambda *a, **k: no_library())
    s, ch = NMSettings.get_default(), seven_channels()
    keys = global_keys(1000.0, s, ch)
    dp = DataProcessor(1000.0, s, ch, line_noise=50, verbose=False, dry_run=True)
    assert dp.keys == keys and dp.device_normalizer is None and dp.chain.where == {"normalizer": None, "projection": None}
    st = ShardedStream(1000.0, ch, settings=s, rank=1, world_size=3, local_input=True)
    assert st.local_rows == [3, 4] and st.owned_rows == [3, 4] and st._dp.local_groups[0].tolist() == [0, 1, 2, 3, 4]


# ---- PostChain: where each step runs --------------------------------------------------------------------------------
@pytest.fixture
def plugin(request):
    import py_neuromodulation_amd as nmx
    from tests import user_plugins as up

    if request.param:
        nmx.add_custom_feature("hop_stats", up.HopStats)
    yield request.param
    if "hop_stats" in nmx.user_features:
        nmx.remove_custom_feature("hop_stats")


def _montage(tmp_path):
    """Three left ECoG contacts and a cortex grid of three points a few millimetres from them."""
    names = ["ECOG_L_1", "ECOG_L_2", "ECOG_L_3"]
    coords = [[-0.030, 0.000, 0.050], [-0.036, 0.006, 0.052], [-0.042, 0.012, 0.054]]
    pd.DataFrame([[-31.0, 1.0, 51.0], [-37.0, 5.0, 50.0], [-44.0, 13.0, 55.0]], columns=["x", "y", "z"]).to_csv(
        tmp_path / "grid_cortex.tsv", sep="\t", index=False)
    return _table(names, ["None"] * 3, ["ecog"] * 3), dict(coord_names=names, coord_list=coords, path_grids=tmp_path)


@pytest.mark.parametrize("plugin", [False, True], indirect=True)
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("norm", [False, True])
def test_post_chain_placement(emu_lib, tmp_path, norm, proj, plugin, ragged):
    """The table of PostChain's docstring, row by row, on 3 channels and 4 hops (11 where the run has to be ragged)."""
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.generator import window_schedule
    from py_neuromodulation_amd.stream import Stream

    ch, kw = _montage(tmp_path)
    s = _fast(norm)
    s.postprocessing.project_cortex = proj
    if not proj:
        kw = {}
    sfreq = RAGGED if ragged else 1000.0
    # (at 1111.111 Hz the tenth window is the first of 1112 samples: eleven hops reach it and come back)
    data = _recording(3, int((2.001 if ragged else 1.34) * sfreq))
    starts, lens, _ = window_schedule(data.shape[1], sfreq, s.sampling_rate_features_hz, s.segment_length_features_ms)
    assert (len(starts), sorted(set(lens.tolist()))) == ((11, [1111, 1112]) if ragged else (4, [1000]))

    st = Stream(sfreq, ch, settings=s, lib=emu_lib, line_noise=50, **kw)
    df = st.run(data, out_dir=tmp_path, save_csv=False)
    dp = st.data_processor
    where = dict(dp.chain.where)
    assert where["normalizer"] == (None if not norm else "host" if ragged else "engine")
    assert where["projection"] == (None if not proj else "merged" if plugin else "host" if ragged else "engine")
    assert dp.engine._norm is (dp.device_normalizer if where["normalizer"] == "engine" else None)
    assert dp.engine._proj is (dp.chain.proj_dev if where["projection"] == "engine" else None)
    assert (dp.chain.user is not None) == plugin and (dp.device_normalizer is not None) == norm
    grid = [k for k in df.columns if k.startswith("gridcortex_")]
    assert bool(grid) == proj and list(df.columns[:-1]) == dp.keys
    if proj:   # behind everything else, the plugin keys included
        assert list(df.columns[-1 - len(grid):-1]) == grid and np.isfinite(df[grid].to_numpy()).all()
    if ragged:
        return
    # the same hops with the chain detached from the engine first: `finish` does on the host what the engine did, bit for bit
    one = DataProcessor(sfreq, s, ch, line_noise=50, lib=emu_lib, verbose=False, **kw)
    attached = one.process_batch(data, starts)
    two = DataProcessor(sfreq, s, ch, line_noise=50, lib=emu_lib, verbose=False, **kw)
    two.chain.detach()
    assert two.engine._norm is None and two.engine._proj is None and "engine" not in two.chain.where.values()
    detached = two.ragged_finish([two.ragged_run(data, starts)])
    assert one.keys == two.keys == dp.keys
    F = len(one.keys)
    assert attached[:, :F].tobytes() == detached[:, :F].tobytes() == df.to_numpy(dtype=np.float64)[:, :F].tobytes()


# ---- LengthTable: two drivers, one hand-over ------------------------------------------------------------------------
def test_length_table_drivers_agree(emu_lib):
    from py_neuromodulation_amd.data_processor import DataProcessor, LengthTable

    s = _fast(True, bursts=True)
    data = _recording(2, 1700)
    ch = _table(["c0", "c1"], ["None"] * 2, ["ecog"] * 2)
    A, B = 1111, 1112
    starts, lens = np.array([0, 111, 222, 333, 444]), np.array([A, B, A, A, B])

    def make(w=None, **kw):
        return DataProcessor(RAGGED, s, ch, line_noise=50, lib=emu_lib, verbose=False, window=w, **kw)

    dp = make()
    assert dp.engine.W_in == A and dp._lengths is None
    for a, n in zip(starts, lens):
        dp.process(data[:, a:a + n])
    twins = dp._lengths
    assert sorted(twins.by_len) == [A, B] and twins.last is twins.by_len[B] and twins.by_len[A] is dp
    assert twins.by_len[B].chain is dp.chain and twins.by_len[B].prep is dp.prep
    hop_by_hop = twins.last.engine.export_state()

    table = LengthTable(make)
    runs = table.run_ragged(lens, lambda p, a, b: p.ragged_run(data, starts[a:b]))
    assert [len(r[0]) for r in runs] == [1, 1, 2, 1] and sorted(table.by_len) == [A, B]
    assert all(p.chain.where["normalizer"] == "host" for p in table.by_len.values())
    assert len(hop_by_hop) > 0 and table.last.engine.export_state() == hop_by_hop

    shard = make(channel_subset=range(0, 1))
    with pytest.raises(ValueError, match=f"expected windows of {A} samples, got {A + 7}"):
        shard.process(data[:, :A + 7])
