"""Time / oscillatory stage time on long windows: 256 channels x 8 hops of 1 s windows at W Hz (W samples per window, hop
W / 10), raw_hjorth + return_raw + linelength + fft + welch (band means, default bands), device-resident input (one chunk,
so the plan's HIP events around stage 2 cover every hop).  Up to ~13 650 samples the plan launches the generic kernel
(window + transform buffers in LDS), beyond it the persistent long-window kernel (nmx_kern_timeosc_long).

Reports the stage-2 time per batch (median / min / max over --reps batches, each the second of two back-to-back
launches), ns per sample per item (items = hops x channels), the fraction of the 8 TB/s HBM roof that time is (4 W bytes
read per item) and the kernels launched.  One JSON line per window length; --out appends them to a file.

    python tools/bench_timeosc_long.py --windows 13000,16000,30000,40000 [--reps 10]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

FEATURES = ["raw_hjorth", "return_raw", "linelength", "fft", "welch"]


def recording(C, T, sfreq, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64) / sfreq
    x = 0.5 * rng.standard_normal((C, T)).astype(np.float32)
    x += (6 * np.sin(2 * np.pi * 11 * t) + 3 * np.sin(2 * np.pi * 47 * t + 1.0)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="13000,16000,30000,40000")
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--hops", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    dev = torch.device("cuda:0")
    C, n = args.channels, args.hops
    names = [f"ch{i:03d}" for i in range(C)]
    for W in [int(w) for w in args.windows.split(",")]:
        sfreq, hop = float(W), W // 10
        T = W + (n - 1) * hop
        s = NMSettings.get_default()
        s.reset()
        eng = HotPathEngine(s, names, sfreq, features=FEATURES, window=W)
        x = torch.from_numpy(recording(C, T, sfreq)).to(dev)
        out = torch.empty((n, eng.n_outputs), dtype=torch.float32, device=dev)
        starts = np.arange(n, dtype=np.int64) * hop
        st = torch.cuda.current_stream(dev).cuda_stream
        ms = []
        for i in range(args.reps + 2):
            for _ in range(2):   # back to back: the timed launch's start event is reached while the GPU is busy
                eng.process_batch_device(x.data_ptr(), T, T, starts, out.data_ptr(), None, st)
            torch.cuda.synchronize(dev)
            if i >= 2:
                ms.append(eng.timing_ms(2))
        items = n * C
        med = float(np.median(ms))
        line = {"label": args.label, "W": W, "channels": C, "hops": n, "items": items, "kernels": eng.kernels(2),
                "stage2_ms_median": round(med, 4), "stage2_ms_min": round(float(np.min(ms)), 4),
                "stage2_ms_max": round(float(np.max(ms)), 4),
                "ns_per_sample_per_item": round(med * 1e6 / (items * W), 5),
                "hbm_roof_fraction": round((items * 4.0 * W / 8e12) / (med * 1e-3), 5),
                "finite": bool(torch.isfinite(out).all().item())}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        eng.close()
        del x, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
