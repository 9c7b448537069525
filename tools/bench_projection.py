"""Grid projection cost at the headline shape: 256 channels at 1 kHz (192 ECoG contacts on a synthetic left-cortex patch, 64
LFP contacts near the left subcortical grid), the default feature set, 1000-sample windows, hop 100, batches of 1024 hops;
projection off and on (cortex + subcortex).

Reports, one JSON line per setting:
  - the projection kernel on 1024 device-resident rows (HIP events) and its algorithmic bytes (gathered inputs C_p * F_c +
    grid outputs G_a * F_c floats per hop) against 8 TB/s; the stage-8 timer of the step (its first chunk only);
  - the whole DataProcessor.process_batch step (host data in, float64 table out), median of --reps;
  - Stream.run hops/s on the same recording (a fresh run each time: plan reuse, one batch, the table and side files).
The grid tables come from tests/golden/projection_d.npz (the reference's grid_cortex.tsv / grid_subcortex.tsv as arrays).

    python tools/bench_projection.py [--reps 10]
"""

from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

PEAK_TBS = 8.0


def montage(g, rng):
    cg, sg = g["grid_cortex"], g["grid_subcortex"]
    ecog = cg[rng.integers(0, len(cg), 192)] + rng.uniform(-6, 6, (192, 3))
    ecog[:, 0] = -np.abs(ecog[:, 0])
    lfp = sg[rng.choice(np.flatnonzero(sg[:, 0] < -8), 64, replace=False)] + rng.uniform(-1, 1, (64, 3))
    names = [f"ECOG_L_{i:03d}" for i in range(192)] + [f"LFP_L_{i:02d}" for i in range(64)]
    return names, (np.concatenate([ecog, lfp]) / 1000).tolist()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--hops", type=int, default=1024)
    args = ap.parse_args()
    import pandas as pd

    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.data_processor import DataProcessor
    from py_neuromodulation_amd.stream import Stream

    g = np.load(ROOT / "tests" / "golden" / "projection_d.npz", allow_pickle=False)
    rng = np.random.default_rng(0)
    names, coords = montage(g, rng)
    C, W, hop, sfreq = 256, 1000, 100, 1000.0
    n = args.hops
    T = W + (n - 1) * hop
    x = (rng.standard_normal((C, T)) * 1e-5).astype(np.float64)
    starts = np.arange(n, dtype=np.int64) * hop
    ch = pd.DataFrame({"name": names, "rereference": ["None"] * C, "used": [1] * C, "target": [0] * C,
                       "type": ["ecog"] * 192 + ["dbs"] * 64, "status": ["good"] * C, "new_name": names})
    with tempfile.TemporaryDirectory() as td:
        grids = Path(td)
        for name in ("cortex", "subcortex"):
            pd.DataFrame(g[f"grid_{name}"], columns=["x", "y", "z"]).to_csv(grids / f"grid_{name}.tsv", sep="\t", index=False)
        for on in (False, True):
            s = NMSettings.get_default()
            s.postprocessing.project_cortex = on
            s.postprocessing.project_subcortex = on
            kw = dict(coord_names=names, coord_list=coords, path_grids=grids)
            dp = DataProcessor(sfreq, s, ch, line_noise=50, verbose=False, **kw)
            dp.process_batch(x, starts)   # warm-up
            ms, k8 = [], []
            for _ in range(args.reps):
                dp.reset()
                t0 = time.perf_counter()
                dp.process_batch(x, starts)
                ms.append((time.perf_counter() - t0) * 1e3)
                if on:
                    k8.append(dp.engine.timing_ms(8))
            rec = {"projection": on, "channels": C, "hops": n, "features": dp.engine.n_outputs, "columns": len(dp.keys),
                   "step_ms_median": round(float(np.median(ms)), 3), "step_ms_min": round(float(np.min(ms)), 3)}
            if on:
                import torch

                lay = dp.projection.layout(dp.engine.keys)
                per_hop = 4 * (len(lay.gather) * lay.n_feat + lay.n_grid)
                # the kernel alone on 1024 device-resident rows of the engine's width, timed with HIP events
                rows = torch.randn((n, dp.engine.row_width), device="cuda", dtype=torch.float32)
                proj = dp.chain.proj_dev
                for _ in range(3):
                    proj.process_device(rows.data_ptr(), rows.shape[1], n)
                kt = []
                for _ in range(args.reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    proj.process_device(rows.data_ptr(), rows.shape[1], n, torch.cuda.current_stream().cuda_stream)
                    b.record()
                    b.synchronize()
                    kt.append(a.elapsed_time(b))
                kmed = float(np.median(kt))
                rec.update({"kernel": dp.engine.kernels(8), "projected_channels": len(lay.gather),
                            "features_per_channel": lay.n_feat, "active_points": len(lay.out_col), "grid_columns": lay.n_grid,
                            "stage8_ms_first_chunk_median": round(float(np.median(k8)), 4),
                            "kernel_ms_1024_hops_median": round(kmed, 4), "bytes_per_hop": per_hop,
                            "kernel_TBps": round(per_hop * n / (kmed * 1e-3) / 1e12, 4),
                            "bytes_at_8TBps_ms": round(per_hop * n / (PEAK_TBS * 1e12) * 1e3, 5)})
            # Stream.run: hops per second (fresh run each rep; the plan of the previous run is reused)
            st = Stream(sfreq, ch, settings=s, line_noise=50, verbose=False, **kw)
            st.run(x, out_dir=td, experiment_name="b", save_csv=False)
            rs = []
            for _ in range(max(3, args.reps // 2)):
                t0 = time.perf_counter()
                st.run(x, out_dir=td, experiment_name="b", save_csv=False)
                rs.append(time.perf_counter() - t0)
            rec["stream_run_ms_median"] = round(1e3 * float(np.median(rs)), 3)
            rec["stream_run_hops_per_s"] = round(n / float(np.median(rs)), 1)
            print(json.dumps(rec), flush=True)
            del dp, st


if __name__ == "__main__":
    main()
