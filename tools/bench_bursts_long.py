"""Bursts chain time on long windows: C channels x n hops of 1 s windows at W Hz (W samples per window, hop W / 10), only
`bursts` on the default bands and history, device-resident input, one chunk -- so the plan's HIP events around stage 3 (the
band-pass bank) and stage 4 (Hilbert envelope, threshold walk, run statistics) cover every hop.  Up to 8 188 samples the
plan launches the kernels it always launched; beyond ~13 650 nmx_kern_hilbert_long, beyond 16 384 nmx_kern_burst_stat_scan,
and a first hop longer than the walk's staging arrays is absorbed in tiles.

Every timed batch continues the stream (hops k n .. k n + n - 1 of one long recording), so the walk is the one of a running
stream, not the sort-once fill of a fresh one.  Reports the stage times per batch (median / min / max over --reps batches,
each the second of two back-to-back launches), ns per sample per (channel, band) item, the kernels launched and the device
memory the plan and its batches took (hand-off buffers, slabs, state: torch.cuda.mem_get_info before / after).  One JSON
line per window length; --out appends them to a file.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats`.

    python tools/bench_bursts_long.py --windows 8000,14000,20000,40000 [--channels 32] [--hops 8] [--reps 6]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
os.environ.setdefault("NMX_LONG_BURSTS", "1")   # bursts above 16 384 samples are opt-in


def recording(C, T, sfreq, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64) / sfreq
    x = 20 * rng.standard_normal((C, T)).astype(np.float32)
    x += (25 * np.sin(2 * np.pi * 17 * t) * (1 + 0.8 * np.sin(2 * np.pi * 2.3 * t))
          + 18 * np.sin(2 * np.pi * 27 * t) * (1 + 0.8 * np.sin(2 * np.pi * 3.1 * t))).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="8000,14000,20000,40000")
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--hops", type=int, default=8)   # (the plan times its stages from 8 hops on)
    ap.add_argument("--reps", type=int, default=6)
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
        n_batches = 2 * (args.reps + 2)
        T = W + (n * n_batches - 1) * hop
        s = NMSettings.get_default()
        s.reset()
        torch.cuda.synchronize(dev)
        free0, _ = torch.cuda.mem_get_info(dev)
        eng = HotPathEngine(s, names, sfreq, features=["bursts"], window=W)
        n_bands = len(s.bursts_settings.frequency_bands)
        x = torch.from_numpy(recording(C, T, sfreq)).to(dev)
        out = torch.empty((n, eng.n_outputs), dtype=torch.float32, device=dev)
        starts = np.arange(n, dtype=np.int64) * hop
        st = torch.cuda.current_stream(dev).cuda_stream
        seg = W + (n - 1) * hop
        bank, chain, k = [], [], 0
        for i in range(args.reps + 2):
            for _ in range(2):   # back to back: the timed launch's start event is reached while the GPU is busy
                xb = x[:, k * n * hop:]
                eng.process_batch_device(xb.data_ptr(), T, seg, starts, out.data_ptr(), None, st)
                k += 1
            torch.cuda.synchronize(dev)
            if i >= 2:
                bank.append(eng.timing_ms(3))
                chain.append(eng.timing_ms(4))
        free1, _ = torch.cuda.mem_get_info(dev)
        items = n * C * n_bands
        line = {"label": args.label, "W": W, "channels": C, "bands": n_bands, "hops": n, "items": items,
                "kernels_bank": eng.kernels(3), "kernels_chain": eng.kernels(4),
                "bank_ms_median": round(float(np.median(bank)), 4), "bank_ms_min": round(float(np.min(bank)), 4),
                "bank_ms_max": round(float(np.max(bank)), 4),
                "chain_ms_median": round(float(np.median(chain)), 4), "chain_ms_min": round(float(np.min(chain)), 4),
                "chain_ms_max": round(float(np.max(chain)), 4),
                "bank_ns_per_sample_per_item": round(float(np.median(bank)) * 1e6 / (items * W), 4),
                "chain_ns_per_sample_per_item": round(float(np.median(chain)) * 1e6 / (items * W), 4),
                "handoff_mib": round(3 * items * W * 4 / 2**20, 1),
                "device_mib_taken": round((free0 - free1) / 2**20 - x.numel() * 4 / 2**20, 1),
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
