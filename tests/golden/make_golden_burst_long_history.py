"""Generate tests/golden/burst_long_history.npz: the reference's `bursts` features with a threshold history of 70 001 top-K
entries (the cases h2k and h4k of tests/burst_long_history_cases.py, which holds the generator, the settings and the
parameters).

Runs in the BUILD container only (it imports the reference through ref_shim, like make_golden_timeosc_long.py); the tests read
the .npz it writes.  Every case is the reference's own Stream.run on 2 channels.  The recordings are NOT stored: the file
holds each case's generator parameters, the settings JSON, the channels, the columns and the reference's feature table.

    python tests/golden/make_golden_burst_long_history.py
"""

from __future__ import annotations

import importlib.util
import json
import sys
import tempfile
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import ref_shim  # noqa: E402

nm = ref_shim.load_reference()

_spec = importlib.util.spec_from_file_location("burst_long_history_cases", HERE.parent / "burst_long_history_cases.py")
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

warnings.filterwarnings("ignore")


def main():
    params = {tag: cases.CASES[tag] for tag in cases.FIXTURE_TAGS}
    out = {"cases": np.array(list(params)), "params_json": json.dumps(params)}
    for tag, p in params.items():
        assert cases.list_entries(p) == cases.K
        data = cases.recording(p)
        st = nm.Stream(sfreq=p["sfreq"], data=data, settings=cases.settings_of(nm, p), line_noise=50, verbose=False)
        with tempfile.TemporaryDirectory() as td:
            df = st.run(data=data, out_dir=td, save_csv=False)
        assert len(df) == p["hops"], (tag, df.shape)
        out.update({f"{tag}_settings_json": json.dumps(st.settings.model_dump()),
                    f"{tag}_columns": np.array(list(df.columns)),
                    f"{tag}_values": df.to_numpy(dtype=np.float64),
                    f"{tag}_channels_json": json.dumps(st.channels.to_dict("list"))})
        print(tag, df.shape)
    np.savez_compressed(HERE / "burst_long_history.npz", **out)
    print("bytes", (HERE / "burst_long_history.npz").stat().st_size)


if __name__ == "__main__":
    main()
