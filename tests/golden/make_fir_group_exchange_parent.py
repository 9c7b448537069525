"""Record tests/golden/fir_group_exchange_parent.npz: the feature rows of the three cases of
tests/test_fir_group_exchange_gpu.py as the library of ANOTHER checkout computes them -- the commit before the exchange of
the channel-pair FIR kernels went group-wise (0b4da40).  Runs on the GPU.

    git worktree add ../parent 0b4da40 && (cd ../parent && python __graft_entry__.py)        # build the parent's library
    python tests/golden/make_fir_group_exchange_parent.py ../parent [output.npz]

The package (and so libnmx.so) is imported from the checkout given; cases, seeds, settings and the run itself are the test
module's of THIS tree.  Every case runs with NMX_NOTCH_SW_FUSE = 1, 0 and 2 (W = 901: 1 only), which must agree bit for bit
before the rows are written.  Per case: <case>_rows (float32), <case>_n_keys, <case>_input_sha256."""

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
other = Path(sys.argv[1]).resolve()
out = Path(sys.argv[2]) if len(sys.argv) > 2 else HERE / "fir_group_exchange_parent.npz"
sys.path.insert(0, str(HERE.parents[1]))   # tests.* of this tree ...
sys.path.insert(0, str(other))             # ... the package of the other checkout in front of it

from py_neuromodulation_amd import _lib  # noqa: E402
from tests import test_fir_group_exchange_gpu as ge  # noqa: E402

lib = _lib.get_library()
assert lib.device_count() >= 1, "no HIP device visible"
assert Path(str(lib.path)).resolve().is_relative_to(other), f"{lib.path} is not the library of {other}"
res = {}
for case in ge.CASES:
    first = None
    for fuse in ((1, 0, 2) if case != "w901" else (1,)):
        keys, rows, kernels, _ = ge.run(lib, case, fuse)
        print(case, fuse, rows.shape, kernels, flush=True)
        if first is None:
            first = rows
        assert np.array_equal(first.view(np.uint32), rows.view(np.uint32)), (case, fuse)
    res[f"{case}_rows"] = first
    res[f"{case}_n_keys"] = np.int64(len(keys))
    res[f"{case}_input_sha256"] = ge.digest(ge.recording(case)[0])
out.parent.mkdir(parents=True, exist_ok=True)
np.savez_compressed(out, **res)
print("wrote", out, out.stat().st_size, "bytes")
