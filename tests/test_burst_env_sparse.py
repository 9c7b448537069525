"""Sparse burst envelope (NMX_BURST_ENV_SPARSE, default 1) against the dense launches it replaces (0), in ONE process.

Once a sequence's 30 s ring is full its threshold only rises, and the walk leaves a lower bound of it (the floor) behind;
the one-wave Hilbert kernel stores a row with no sample at or above the floor as its last `overlap` samples only, and the
statistics kernel answers such a row with six +0.f without loading it.  Nothing of the arithmetic changes, so every column
is equal bit for bit (NaN-aware), not within a tolerance.

The recordings are loud first -- the ring fills with large envelopes -- and continue at 0.2 x the amplitude, so that most
later rows stay below the floor, with short loud bursts where a skipped row would show: across a window's first sample,
ending on a window's last sample (in_burst = 1) and inside the tail the walk reads.  Chunks are short (NMX_CHUNK_WINDOWS), so
that a batch has chunks behind the one in which the ring fills: the floor a walk leaves serves the chunks after it."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPARSE = ("nmx_kern_hilbert_w500_sparse", "nmx_kern_burst_stat_reg_sparse<16>")
W, HOP = 1000, 100


@pytest.fixture(scope="module")
def gpu_lib():
    from py_neuromodulation_amd import _lib

    lib = _lib.get_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    assert "libnmx.so" in str(lib.path)
    return lib


def _settings(duration_s=None):
    from py_neuromodulation_amd import NMSettings

    s = NMSettings.get_default()
    s.features.disable_all()
    s.features.bursts = True
    s.features.raw_hjorth = True   # (columns of another stage next to the bursts': the rows are compared whole)
    if duration_s is not None:
        s.bursts_settings.time_duration_s = duration_s
    return s.validate()


def _engine(lib, monkeypatch, sparse, C, chunk, duration_s=None):
    """An engine built with NMX_BURST_ENV_SPARSE=sparse and chunks of `chunk` hops (both are read when the plan is created)."""
    from py_neuromodulation_amd.engine import HotPathEngine

    monkeypatch.setenv("NMX_BURST_ENV_SPARSE", "2" if sparse else "0")   # (2 = 1 + the flags of every chunk read back and counted)
    monkeypatch.setenv("NMX_CHUNK_WINDOWS", str(chunk))
    try:
        return HotPathEngine(_settings(duration_s), [f"ch{i}" for i in range(C)], 1000.0, lib=lib)
    finally:
        monkeypatch.delenv("NMX_BURST_ENV_SPARSE")
        monkeypatch.delenv("NMX_CHUNK_WINDOWS")


def _recording(C, n_hops, loud_samples, bursts, seed):
    """Noise + weak beta / gamma lines, at full level for the first `loud_samples` samples and at 0.2 x behind them; `bursts`:
    sample ranges [a, b) that carry a strong 17 + 27 Hz oscillation (both burst bands) on every channel."""
    T = W + (n_hops - 1) * HOP
    rng = np.random.default_rng(seed)
    t = np.arange(T) / 1000.0
    osc = np.sin(2 * np.pi * 17 * t) + np.sin(2 * np.pi * 27 * t + 0.7)
    x = rng.standard_normal((C, T)) * 30 + 3 * osc + rng.uniform(-20, 20, (C, 1))
    x[:, loud_samples:] *= 0.2
    for a, b in bursts:
        x[:, a:b] += 80 * osc[a:b]
    return x.astype(np.float32), np.arange(n_hops) * HOP


def _same(a, b, what=""):
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), \
        f"{what}: {int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())} entries differ"


def _tail_rows(ran):
    """(rows stored as their tail only, rows) over the engine's life, from the count mode's note in the stage-4 list."""
    note = [p for p in ran.split(",") if p.startswith("env_tail_rows=")]
    assert len(note) == 1, ran
    a, b = note[0].split("=")[1].split("/")
    return int(a), int(b)


def _check_kernels(eng, sparse, counts=None):
    ran = eng.kernels(4)
    for name in SPARSE:
        assert (name in ran) == bool(sparse), (sparse, ran)
    if sparse and counts is not None:
        counts.append(_tail_rows(ran))


def _both(lib, monkeypatch, C, chunk, run, duration_s=None, counts=None, walks=None):
    """run(make_engine) with engines of each kind; returns (sparse rows, dense rows).  `make_engine()` builds a fresh engine of
    the kind under test; the stage-4 kernel list of every engine is checked when it is closed.  `counts`: gets (tail-only
    rows, rows) of every sparse engine; `walks`: gets every engine's stage-4 list."""
    out = []
    for sparse in (1, 0):
        made = []

        def make():
            made.append(_engine(lib, monkeypatch, sparse, C, chunk, duration_s))
            return made[-1]

        out.append(run(make))
        for eng in made:
            _check_kernels(eng, sparse, counts)
            if walks is not None:
                walks.append(eng.kernels(4))
            eng.close()
    return out


# the 30 s stream of the first and third test: the ring (30 000 samples) is full at hop 291; loud for 32 s; then bursts
N_HOPS, LOUD = 420, 32000
BURSTS = ((32950, 33050),    # inside the tail of window 320 (and one of the one-window calls of the hand-over test)
          (34450, 34550),    # across the first sample of window 345
          (36850, 37000),    # ends on the last sample of window 360
          (38420, 38480))    # inside the tail [900, 1000) of window 375


def _in_burst_cols(keys, ch):
    return [i for i, k in enumerate(keys) if k.startswith(ch + "_") and "_bursts_" in k and k.endswith("in_burst")]


def test_fill_then_steady(gpu_lib, monkeypatch):
    """C = 3, 420 hops, chunks of 64: the fill ends inside the fifth chunk (hop 291) and two steady chunks follow."""
    x, starts = _recording(3, N_HOPS, LOUD, BURSTS, 5)
    keys = []

    def run(make):
        eng = make()
        keys[:] = list(eng.keys)
        return eng.process_batch(x, starts)

    counts = []
    sp, de = _both(gpu_lib, monkeypatch, 3, 64, run, counts=counts)
    _same(sp, de, "420 hops in chunks of 64")
    # the floor did its work: of the 6 x 100 rows of the two steady chunks (hops 320 .. 419) at least the 6 x 20 quiet ones
    # asserted below were stored as their tail only, and none of the 6 x 320 rows of the chunks before them
    tail, rows = counts[0]
    assert rows == 6 * N_HOPS and 6 * 20 <= tail <= 6 * 100, counts
    # the recording does what it was built for (read from the DENSE rows): quiet rows without any burst behind the loud part,
    # bursts where they were inserted, and window 360 ends inside one
    bcols = [i for i, k in enumerate(keys) if "_bursts_" in k]
    quiet = [h for h in range(330, N_HOPS) if not np.any(de[h, bcols])]
    assert len(quiet) >= 20, len(quiet)
    for h in (320, 345, 360, 375):
        assert np.any(de[h, bcols] > 0), h
    assert all(np.any(de[360, _in_burst_cols(keys, f"ch{c}")] == 1.0) for c in range(3))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("duration_s", [5, 2])
def test_shorter_histories(gpu_lib, monkeypatch, duration_s, C):
    """time_duration_s = 5: K = 1251 entries, the one-wave walk; 2: K = 501, the workgroup walk merges every hop with the
    ring full and leaves the floor.  120 hops in chunks of 32; loud for 7 s."""
    bursts = ((8950, 9050), (9450, 9550), (10350, 10500), (11420, 11480))   # tail of 80, first sample of 95, end of 95, tail of 105
    x, starts = _recording(C, 120, 7000, bursts, 40 + duration_s)
    keys = []

    def run(make):   # (two batches: the stage-4 list names the kernels of the LAST batch's first chunk -- a steady one)
        eng = make()
        keys[:] = list(eng.keys)
        return np.concatenate([eng.process_batch(x, starts[:96]),
                               eng.process_batch(x[:, starts[96]:].copy(), starts[96:] - starts[96])])

    counts, walks = [], []
    sp, de = _both(gpu_lib, monkeypatch, C, 32, run, duration_s, counts=counts, walks=walks)
    _same(sp, de, f"{duration_s} s history, {C} channels")
    for ran in walks:
        assert ("nmx_kern_burst_thr_wave" in ran) == (duration_s == 5), ran
        assert ("nmx_kern_burst_thr<" in ran) == (duration_s == 2), ran
    tail, rows = counts[0]
    assert rows == 2 * C * 120 and 2 * C * 5 <= tail <= 2 * C * 56, counts   # only the chunks behind hop 64 can hold such rows
    bcols = [i for i, k in enumerate(keys) if "_bursts_" in k]
    assert sum(1 for h in range(64, 120) if not np.any(de[h, bcols])) >= 5
    assert np.any(de[95, bcols] > 0) and np.any(de[95, _in_burst_cols(keys, "ch0")] == 1.0)


def test_hand_over_paths(gpu_lib, monkeypatch):
    """The stream of the first test as one batch, as 300 hops + 30 one-window calls + the rest, and with the state exported at
    hop 330 and imported into a fresh engine (whose floor starts at "no bound" again)."""
    x, starts = _recording(3, N_HOPS, LOUD, BURSTS, 5)
    one = np.zeros(1, dtype=np.int64)

    def as_one_batch(make):
        return make().process_batch(x, starts)

    def with_single_windows(make):
        eng = make()
        rows = [eng.process_batch(x, starts[:300])]
        rows += [eng.process_batch(x[:, a:a + W].copy(), one) for a in starts[300:330]]
        rows.append(eng.process_batch(x[:, starts[330]:].copy(), starts[330:] - starts[330]))
        return np.concatenate(rows)

    def with_state_import(make):
        eng = make()
        head = eng.process_batch(x, starts[:330])
        blob = eng.export_state()
        fresh = make()
        fresh.import_state(blob)
        return np.concatenate([head, fresh.process_batch(x[:, starts[330]:].copy(), starts[330:] - starts[330])])

    for what, run in (("one batch", as_one_batch), ("300 + 30 x 1 + 90", with_single_windows),
                      ("export / import at hop 330", with_state_import)):
        sp, de = _both(gpu_lib, monkeypatch, 3, 64, run)
        assert sp.shape[0] == N_HOPS
        _same(sp, de, what)


def test_non_finite_samples(gpu_lib, monkeypatch):
    """One NaN sample (the value 0 on load) and one -inf sample (its rows' envelopes are NaN / infinite) behind hop 300, in the
    steady regime.  Two DENSE engines are compared first: should they disagree, only the burst columns of the channel they
    disagree in are left out of the sparse / dense comparison, and nothing else may differ between them."""
    x, starts = _recording(3, N_HOPS, LOUD, BURSTS, 5)
    x[0, 34321] = np.nan
    x[1, 35555] = -np.inf
    keys = []

    def run(make):
        eng = make()
        keys[:] = list(eng.keys)
        return eng.process_batch(x, starts)

    sp, de = _both(gpu_lib, monkeypatch, 3, 64, run)
    _, de2 = _both(gpu_lib, monkeypatch, 3, 64, run)
    keep = np.ones(len(keys), dtype=bool)
    for c in range(3):
        cols = np.array([k.startswith(f"ch{c}_") and "_bursts_" in k for k in keys])
        if not np.array_equal(de[:, cols], de2[:, cols], equal_nan=True):
            keep &= ~cols
    _same(de[:, keep], de2[:, keep], "dense against dense outside the burst columns")
    ch1 = np.array([k.startswith("ch1_") and "_bursts_" in k for k in keys])
    assert keep[~ch1].all(), "only the burst columns of ch1, the channel with the infinite sample, may be left out"
    _same(sp[:, keep], de[:, keep], "NaN / -inf samples")
