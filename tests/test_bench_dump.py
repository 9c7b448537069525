"""bench.py --dump-outputs: the rows are written as float32 .npy files, whole when they fit the cap, else a fixed
seeded sample of whole rows with the kept row indices next to them."""

import numpy as np

import bench


def test_dump_outputs_whole_rows_under_the_cap(tmp_path):
    out = np.random.default_rng(1).standard_normal((16, 24)).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "d"), "features", out)
    got = np.load(tmp_path / "d" / "features.npy")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, out)
    assert not (tmp_path / "d" / "features_rows.npy").exists()


def test_dump_outputs_seeded_sample_above_the_cap(tmp_path):
    out = np.arange(1000 * 50, dtype=np.float32).reshape(1000, 50)
    limit = 40_000
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), "features", out, limit=limit)
    got = np.load(tmp_path / "a" / "features.npy")
    rows = np.load(tmp_path / "a" / "features_rows.npy")
    assert got.dtype == np.float32 and rows.dtype == np.float64
    assert got.nbytes + rows.nbytes <= limit and 0 < len(rows) < 1000
    np.testing.assert_array_equal(got, out[rows.astype(np.int64)])
    # the same sample every time
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "features.npy"), got)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "features_rows.npy"), rows)
