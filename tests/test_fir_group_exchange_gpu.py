"""The channel-pair FIR kernels after the exchange went group-wise (nmx_k_bank_w64c.h / nmx_k_bank_w64e.h: one 8-row tile
per wave, one row group per round) against feature rows the PREVIOUS build of the library produced on the GPU
(tests/golden/fir_group_exchange_parent.npz): the arithmetic is untouched, so the rows are equal byte for byte, for every
value of NMX_NOTCH_SW_FUSE.  So that this is not only a comparison of the library with itself, the same rows are held against
the float64 oracle under the standard policy (tests/parity.py).

    case   channels x hops   W     what it reaches
    full   8 x 512           1000  2048 channel pairs in ONE launch: the smallest batch at which nmx_w64_pair_geom builds
                                   full-width workgroups (12 waves at M = 1536, 7 at M = 2048) -- every wave of a workgroup
                                   has an item, every tile is used
    odd    3 x 5             1000  the two-wave form of a small batch; the last pair's partner is missing
    w901   5 x 5             901   the notch of a run-time shape, nmx_kern_bank_w64e_rd64<1> (tests/fir_sample_probe_cases.py:
                                   notch_w901), then the M = 1536 bank and the M = 2048 pre-filters as launches of their own

bandpass_filter, sharpwave_analysis and return_raw behind notch + common average, default bands, hop = 100 samples.  A host
batch is cut into chunks of 128 + 384 hops by default, which would leave every launch of `full` below 2048 pairs and in the
two-wave form: the plans are built under NMX_HOST_FIRST_CHUNK = NMX_HOST_CHUNK_WINDOWS = 512 (chunking does not change a
byte), and every test asserts the geometry its launches had (nmx_last_kernels(plan, 9): pairs, workgroups x waves).  The
recordings are regenerated from their seeds; the fixture holds their SHA-256, so a numpy whose generator draws other numbers
is reported as that and not as a kernel fault.  The oracle walks all hops of `odd` and every 16th hop of `full` plus its
last (33 rows of the full-width launch; a row of the oracle costs ~0.05 s, and the other rows are pinned by the bytes).  It
is held against the rows of NMX_NOTCH_SW_FUSE = 1 only: the rows of 0 and 2 are the same bytes.
tests/golden/make_fir_group_exchange_parent.py records the fixture from a checkout of the previous commit."""

import hashlib
import os
from pathlib import Path

import numpy as np
import pytest

from tests import parity

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).parent / "golden" / "fir_group_exchange_parent.npz"
HOP = 100
# name -> channels, hops, window, seed
CASES = {"full": (8, 512, 1000, 41), "odd": (3, 5, 1000, 42), "w901": (5, 5, 901, 43)}
FUSED1 = "nmx_kern_notch_bank_w64e_rd64<1000, 499, 1>"
FUSED2 = "nmx_kern_notch_bank_w64e_rd64<1000, 499, 2>"
NOTCH_WC, NOTCH_RT = "nmx_kern_bank_w64e_rd64<1, 1000, 499>", "nmx_kern_bank_w64e_rd64<1>"
W64C, W64E0 = "nmx_kern_bank_w64c_rd64", "nmx_kern_bank_w64e_rd64<0>"
# fuse -> (prep, bank, second launch) of the W = 1000 plans
WANT = {1: (FUSED1, W64C, ""), 2: (FUSED2, W64C, ""), 0: (NOTCH_WC, W64C, W64E0)}
ONE_LAUNCH = {"NMX_HOST_FIRST_CHUNK": "512", "NMX_HOST_CHUNK_WINDOWS": "512"}   # (read when the plan is built)
FULL_WAVES = {W64C: 12}   # waves per workgroup of a full-width launch; every M = 2048 kernel: 7


def settings(case: str):
    from py_neuromodulation_amd import NMSettings

    W = CASES[case][2]
    s = NMSettings.get_default()
    s.features.disable_all()
    s.features.bandpass_filter = s.features.sharpwave_analysis = s.features.return_raw = True
    if W != 1000:   # (the band-pass segments may not be longer than the window: tests/fir_sample_probe_cases.py, "w901")
        s.segment_length_features_ms = W
        s.bandpass_filter_settings.segment_lengths_ms = {"theta": W, "alpha": 500, "low_beta": 333, "high_beta": 333}
    return s.validate()


def recording(case: str):
    C, hops, W, seed = CASES[case]
    T = W + (hops - 1) * HOP
    rng = np.random.default_rng(seed)
    t = np.arange(T) / 1000.0
    x = rng.standard_normal((C, T)) * 50 + 10 * np.sin(2 * np.pi * 20 * t) + rng.uniform(-300.0, 300.0, (C, 1))
    return x.astype(np.float32), np.arange(hops) * HOP


def digest(x: np.ndarray) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(x).tobytes()).digest(), np.uint8)


def geometry(text: str) -> dict:
    """nmx_last_kernels(plan, 9), "<kernel>: <n> pairs, <workgroups> x <waves> waves + ..." -> {kernel: (pairs, workgroups, waves)}"""
    out = {}
    for entry in filter(None, text.split(" + ")):
        name, rest = entry.rsplit(": ", 1)
        pairs, shape = rest.split(" pairs, ")
        grid, waves = shape.removesuffix(" waves").split(" x ")
        out[name] = (int(pairs), int(grid), int(waves))
    return out


def check_geometry(case: str, geom: dict, kernels) -> None:
    """Every channel-pair kernel of the batch ran ONE launch over all pairs of the case: full-width workgroups with an item
    for every wave at 2048 pairs, the two-wave form below."""
    C, hops, _, _ = CASES[case]
    n_pairs = hops * ((C + 1) // 2)
    assert set(geom) == set(kernels), (geom, kernels)
    for name, (pairs, grid, waves) in geom.items():
        assert pairs == n_pairs, f"{case}: {name} ran a launch of {pairs} pairs, not the batch's {n_pairs}"
        assert waves == (FULL_WAVES.get(name, 7) if n_pairs >= 2048 else 2), (case, name, waves)
        # a wave walks `chunk` consecutive items: the launch covers the pairs, and its first workgroup is full -- every wave
        # index, so every tile slot of a workgroup, has work
        chunk = -(-n_pairs // (grid * waves))
        assert grid * waves * chunk >= n_pairs >= waves * chunk, (case, name, pairs, grid, waves)


def run(lib, case: str, fuse: int):
    """-> (keys, rows, kernels of the stages prep / bank / second launch, launch geometry of the pair kernels) of an engine
    built with NMX_NOTCH_SW_FUSE=fuse; the batch goes out as one launch sequence."""
    from py_neuromodulation_amd import fir_design
    from py_neuromodulation_amd.engine import HotPathEngine

    C, _, W, _ = CASES[case]
    R = np.full((C, C), -1.0 / (C - 1))
    np.fill_diagonal(R, 1.0)
    x, starts = recording(case)
    env = dict(ONE_LAUNCH, NMX_NOTCH_SW_FUSE=str(fuse))   # (read when the plan is built)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = HotPathEngine(settings(case), [f"ch{i}_avgref" for i in range(C)], 1000.0, lib=lib, ref_matrix=R,
                            notch_taps=fir_design.notch_bank(1000.0, 50), window=W)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        rows = eng.process_batch(x, starts)
        try:
            geom = geometry(eng.kernels(9))
        except (RuntimeError, ValueError):   # (a library from before the geometry was reported: the fixture's maker at the parent)
            geom = None
        return list(eng.keys), rows, tuple(eng.kernels(k).split(" + ") for k in (1, 3, 6)), geom
    finally:
        eng.close()


@pytest.fixture(scope="module")
def gpu_lib():
    from py_neuromodulation_amd import _lib

    lib = _lib.get_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    assert "libnmx.so" in str(lib.path)
    return lib


@pytest.fixture(scope="module")
def parent():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _same_bytes(got: np.ndarray, want: np.ndarray, what: str) -> None:
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} entries differ from the parent build's, first at " \
                           f"{tuple(int(i) for i in np.argwhere(diff)[0])}"


def _check_input(parent, case):
    assert np.array_equal(digest(recording(case)[0]), parent[f"{case}_input_sha256"]), \
        f"{case}: the regenerated recording is not the one the fixture was made from (numpy's generator?)"


@pytest.mark.parametrize("fuse", [1, 0, 2])
@pytest.mark.parametrize("case", ["full", "odd"])
def test_rows_are_the_parent_builds_bytes(gpu_lib, parent, case, fuse):
    _check_input(parent, case)
    keys, rows, (prep, bank, second), geom = run(gpu_lib, case, fuse)
    want = WANT[fuse]
    assert want[0] in prep and want[1] in bank and (want[2] in second if want[2] else second == [""]), (prep, bank, second)
    check_geometry(case, geom, [k for k in want if k])
    assert len(keys) == int(parent[f"{case}_n_keys"])
    _same_bytes(rows, parent[f"{case}_rows"], f"{case}, NMX_NOTCH_SW_FUSE={fuse}")


def test_generic_notch_kernel_rows_are_the_parent_builds_bytes(gpu_lib, parent):
    _check_input(parent, "w901")
    keys, rows, (prep, bank, second), geom = run(gpu_lib, "w901", 1)
    assert NOTCH_RT in prep and W64C in bank and W64E0 in second, (prep, bank, second)
    check_geometry("w901", geom, [NOTCH_RT, W64C, W64E0])
    assert len(keys) == int(parent["w901_n_keys"])
    _same_bytes(rows, parent["w901_rows"], "w901")


ORACLE_HOPS = {"odd": range(5), "full": (*range(0, 512, 16), 511)}


@pytest.mark.parametrize("case", ["full", "odd"])
def test_rows_against_the_oracle(gpu_lib, case):
    from oracle import nm_oracle as orc

    C = CASES[case][0]
    x, starts = recording(case)
    keys, rows, _, geom = run(gpu_lib, case, 1)
    check_geometry(case, geom, [FUSED1, W64C])
    s = settings(case)
    names = [f"ch{i}" for i in range(C)]
    channels = {"name": names, "rereference": ["average"] * C, "used": [1] * C, "target": [0] * C,
                "type": ["ecog"] * C, "status": ["good"] * C, "new_name": [f"{n}_avgref" for n in names]}
    so = type(s)(**s.to_dict())
    so.postprocessing.feature_normalization = False
    so.preprocessing = ["notch_filter", "re_referencing"]
    dp = orc.DataProcessor(1000.0, so, channels, line_noise=50)
    pv = parity.PipelineVerifiers(so, channels, 1000.0, x, starts, 1000, line_noise=50)
    for i in ORACLE_HOPS[case]:
        a = int(starts[i])
        d = dp.process(x[:, a:a + 1000].astype(np.float64))
        b, rep, _ = parity.compare(keys, rows[i], [d[k] for k in keys], so, 1000.0, 400.0, 1000, verifier=pv.row(i))
        assert b == 0, f"{case}, hop {i}\n{rep}"
