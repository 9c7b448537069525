"""Band-pass bank time on long windows: C channels x n hops of 1 s windows at W Hz (W samples per window, hop W / 10), only
`bandpass_filter` on the default bands, device-resident input, one chunk -- so the plan's HIP events around stage 3 (the
band-pass bank, nmx_kern_bank_diff above 16 384 samples) cover every hop.  One plan per feature set: activity alone (one
series per filter), + mobility (two: y and x * g1), + complexity (three: and x * g2); the frame spectra are shared.

Reports the stage time per batch (median / min / max over --reps batches, each the second of two back-to-back launches), the
ratio to the activity-only plan and the kernel launched.  One JSON line per (window length, feature set); --out appends them
to a file.

    python tools/bench_bandpower_long.py --windows 20000,30000,40000 [--channels 64] [--hops 8] [--reps 6]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
os.environ.setdefault("NMX_LONG_BANDPOWER", "1")   # band-pass power above 16 384 samples is opt-in

FEATS = ("activity", "mobility", "complexity")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="20000,30000,40000")
    ap.add_argument("--channels", type=int, default=64)
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
        T = W + (n * 2 * (args.reps + 2) - 1) * hop
        x = torch.from_numpy((50 * np.random.default_rng(0).standard_normal((C, T))).astype(np.float32)).to(dev)
        base = None
        for k_feat in (1, 2, 3):
            s = NMSettings.get_default()
            s.reset()
            for i, f in enumerate(FEATS):
                setattr(s.bandpass_filter_settings.bandpower_features, f, i < k_feat)
            eng = HotPathEngine(s, names, sfreq, features=["bandpass_filter"], window=W)
            out = torch.empty((n, eng.n_outputs), dtype=torch.float32, device=dev)
            starts = np.arange(n, dtype=np.int64) * hop
            st = torch.cuda.current_stream(dev).cuda_stream
            seg = W + (n - 1) * hop
            bank, k = [], 0
            for i in range(args.reps + 2):
                for _ in range(2):   # back to back: the timed launch's start event is reached while the GPU is busy
                    eng.process_batch_device(x[:, k * n * hop:].data_ptr(), T, seg, starts, out.data_ptr(), None, st)
                    k += 1
                torch.cuda.synchronize(dev)
                if i >= 2:   # (warm-ups discarded)
                    bank.append(eng.timing_ms(3))
            med = float(np.median(bank))
            base = med if base is None else base
            n_bands = len(s.frequency_ranges_hz)
            line = {"label": args.label, "W": W, "channels": C, "bands": n_bands, "hops": n, "features": list(FEATS[:k_feat]),
                    "kernels_bank": eng.kernels(3), "bank_ms_median": round(med, 4), "bank_ms_min": round(float(np.min(bank)), 4),
                    "bank_ms_max": round(float(np.max(bank)), 4), "ratio_to_activity_only": round(med / base, 3),
                    "bank_ns_per_sample_per_item": round(med * 1e6 / (n * C * n_bands * W), 4),
                    "finite": bool(torch.isfinite(out).all().item())}
            text = json.dumps(line)
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")
            eng.close()
            del out
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
