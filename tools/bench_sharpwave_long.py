"""Sharp-wave stage time on long windows: 64 channels x 256 hops of 1 s windows at W Hz (W samples per window, hop W / 10),
only sharpwave_analysis enabled, device-resident input (one chunk, so the plan's HIP events around stage 5 cover every
hop).  Two settings: the default filter ranges on band-limited activity (about 60 extrema of a kind per window: the
dense-first launch finishes every item) and filter_ranges_hz = [[5, 5000]] on white noise (thousands of extrema: every
item goes to the list kernel -- in LDS up to ~14 500 samples, in the per-workgroup slabs of device memory beyond).

Reports the stage-5 time per batch (median / min / max over --reps batches, each the second of two back-to-back
launches), ns per sample of pre-filtered series (items x W), the kernels launched and a HOST ESTIMATE of the share of
items the list kernel took: float64 filtered series of a sample of 4 channels x 4 hops, counted as list items when
they have more than 128 maxima or minima (the kernels' rule), or all of them for a plan without the dense path.  It is
not read back from the device's flags; the two settings are far from the threshold (about 50 and about 4000 extrema).
One JSON line per configuration; --out appends them to a file.

    python tools/bench_sharpwave_long.py --windows 14000,16000,30000 --ranges default,wide [--reps 10]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def recording(C, T, sfreq, kind, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((C, T)).astype(np.float32)
    if kind == "default":
        t = np.arange(T, dtype=np.float64) / sfreq
        x = 0.5 * x + (6 * np.sin(2 * np.pi * 11 * t) + 3 * np.sin(2 * np.pi * 47 * t + 1.0)).astype(np.float32)
        x += np.cumsum(rng.standard_normal((C, T)).astype(np.float32), axis=1) * np.float32(0.05 * np.sqrt(7000.0 / sfreq))
    return np.ascontiguousarray(x, dtype=np.float32)


def slab_share(x, W, hop, taps, dense_ok, n_ch=4, n_hops=4):
    """Share of (window, channel, filter) items with more than 128 maxima or minima, on a sample of items."""
    if not dense_ok:
        return 1.0
    from scipy.signal import fftconvolve

    over = total = 0
    for c in range(min(n_ch, x.shape[0])):
        for h in range(n_hops):
            w = x[c, h * hop:h * hop + W].astype(np.float64)
            for tp in taps:
                y = fftconvolve(w, np.asarray(tp, np.float64), mode="same")
                d = np.sign(np.diff(y))
                d = d[d != 0]
                turns = np.diff(d)
                over += int((turns < 0).sum() > 128 or (turns > 0).sum() > 128)
                total += 1
    return over / total


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="14000,16000,30000")
    ap.add_argument("--ranges", default="default,wide")
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--hops", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from py_neuromodulation_amd import NMSettings, fir_design
    from py_neuromodulation_amd.engine import HotPathEngine

    dev = torch.device("cuda:0")
    C, n = args.channels, args.hops
    names = [f"ch{i:03d}" for i in range(C)]
    for W in [int(w) for w in args.windows.split(",")]:
        sfreq, hop = float(W), W // 10
        T = W + (n - 1) * hop
        for kind in args.ranges.split(","):
            s = NMSettings.get_default()
            s.reset()
            s.features.sharpwave_analysis = True
            if kind == "wide":
                s.sharpwave_analysis_settings.filter_ranges_hz = [[5, 5000]]
            xh = recording(C, T, sfreq, kind)
            eng = HotPathEngine(s, names, sfreq, features=["sharpwave_analysis"], window=W)
            x = torch.from_numpy(xh).to(dev)
            out = torch.empty((n, eng.n_outputs), dtype=torch.float32, device=dev)
            starts = np.arange(n, dtype=np.int64) * hop
            st = torch.cuda.current_stream(dev).cuda_stream
            ms = []
            for i in range(args.reps + 2):
                for _ in range(2):   # back to back: the timed launch's start event is reached while the GPU is busy
                    eng.process_batch_device(x.data_ptr(), T, T, starts, out.data_ptr(), None, st)
                torch.cuda.synchronize(dev)
                if i >= 2:
                    ms.append(eng.timing_ms(5))
            ranges = s.sharpwave_analysis_settings.filter_ranges_hz
            taps = [fir_design.band_pass(sfreq, fr[0], fr[1]) for fr in ranges]
            kernels = eng.kernels(5)
            items = n * C * len(ranges)
            med = float(np.median(ms))
            line = {"label": args.label, "W": W, "ranges": kind, "channels": C, "hops": n, "items": items,
                    "kernels": kernels,
                    "stage5_ms_median": round(med, 4), "stage5_ms_min": round(float(np.min(ms)), 4),
                    "stage5_ms_max": round(float(np.max(ms)), 4),
                    "ns_per_sample": round(med * 1e6 / (items * W), 5),
                    "list_share_host_estimate": round(slab_share(xh, W, hop, taps, "dense" in kernels), 4),
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
