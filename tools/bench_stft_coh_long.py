"""STFT and coherence stage times on long windows (opt-in: NMX_LONG_STFT=1, NMX_LONG_COHERENCE=1), from the plan's HIP events
(nmx_last_timing_ms: stage 2 time / oscillatory, stage 7 coherence), device-resident input, one batch of --hops windows per call.
Method of profiles/nolds_sampen.md: --warmup calls discarded, then median / min / max of --reps timed calls.

Cases (one JSON line each; --out appends them to a file):
  stft            stft alone: (sfreq, window ms, nperseg) of --stft, e.g. 30000:1000:500 (the per-wave class), 2000:20000:20000
                  (the split class), 16000:1000:500 (the generic kernel: the largest STFT plan without the opt-in), per sample of window
  coh             coherence alone, --pairs pairs: (sfreq, nperseg) of --coh, e.g. 30000:256, 40000:4096, 16000:256; per segment
  plan            the default features on a 30 kHz / 1 s plan with the four long-window switches set, with and without stft: host
                  clock around the call (ends in a device synchronise) and the stage-2 timer

    python tools/bench_stft_coh_long.py --case stft --stft 30000:1000:500,2000:20000:20000,16000:1000:500
    python tools/bench_stft_coh_long.py --case coh --coh 30000:256,40000:4096,16000:256
    python tools/bench_stft_coh_long.py --case plan --channels 256 --hops 128
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
for _v in ("NMX_LONG_STFT", "NMX_LONG_COHERENCE", "NMX_LONG_BURSTS", "NMX_LONG_BANDPOWER"):
    os.environ.setdefault(_v, "1")   # opt-ins of windows above 16 384 samples


def _emit(args, line):
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


def _timed(args, eng, x, W, hop, n, stage):
    import torch

    dev = x.device
    out = torch.empty((n, eng.n_outputs), dtype=torch.float32, device=dev)
    starts = np.arange(n, dtype=np.int64) * hop
    st = torch.cuda.current_stream(dev).cuda_stream
    seg = W + (n - 1) * hop
    ms, wall = [], []
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        eng.process_batch_device(x.data_ptr(), x.shape[1], seg, starts, out.data_ptr(), None, st)
        torch.cuda.synchronize(dev)
        if i >= args.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(eng.timing_ms(stage))
    stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}
    return stats(ms), stats(wall), bool(torch.isfinite(out).all().item())


def _input(C, W, hop, n, dev):
    import torch

    T = W + (n - 1) * hop
    return torch.from_numpy(np.random.default_rng(0).standard_normal((C, T)).astype(np.float32)).to(dev)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("stft", "coh", "plan"), required=True)
    ap.add_argument("--stft", default="30000:1000:500,2000:20000:20000,16000:1000:500")
    ap.add_argument("--coh", default="30000:256,40000:4096,16000:256")
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--hops", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    dev = torch.device("cuda:0")
    n = args.hops
    if args.case == "stft":
        C = args.channels
        names = [f"ch{i:03d}" for i in range(C)]
        for spec in args.stft.split(","):
            sfreq, wms, nper = (int(v) for v in spec.split(":"))
            W, hop = sfreq * wms // 1000, sfreq // 10
            s = NMSettings.get_default()
            s.reset()
            s.segment_length_features_ms = wms
            s.stft_settings.windowlength_ms = nper
            s.frequency_ranges_hz["wide"] = [0.05 * sfreq, 0.2 * sfreq]   # (beside the default bands: bins at every rate)
            eng = HotPathEngine(s, names, float(sfreq), features=["stft"], window=W)
            x = _input(C, W, hop, n, dev)
            ms, wall, finite = _timed(args, eng, x, W, hop, n, 2)
            _emit(args, {"label": args.label, "case": "stft", "sfreq": sfreq, "W": W, "nperseg": nper, "channels": C, "hops": n,
                         "kernels": eng.kernels(2), "stage_ms": ms, "wall_ms": wall,
                         "ns_per_sample_of_window": round(ms["median"] * 1e6 / (n * C * W), 5), "finite": finite})
            eng.close()
            del x
            torch.cuda.empty_cache()
    elif args.case == "coh":
        C = 2 * args.pairs
        names = [f"ch{i:03d}" for i in range(C)]
        for spec in args.coh.split(","):
            sfreq, nper = (int(v) for v in spec.split(":"))
            W, hop = sfreq, sfreq // 10
            s = NMSettings.get_default()
            s.reset()
            s.frequency_ranges_hz["wide"] = [0.05 * sfreq, 0.2 * sfreq]
            s.coherence_settings.channels = [[names[2 * i], names[2 * i + 1]] for i in range(args.pairs)]
            s.coherence_settings.nperseg = nper
            s.coherence_settings.frequency_bands = ["wide"]
            eng = HotPathEngine(s, names, float(sfreq), features=["coherence"], window=W)
            x = _input(C, W, hop, n, dev)
            ms, wall, finite = _timed(args, eng, x, W, hop, n, 7)
            nseg = (W - nper) // (nper - nper // 2) + 1
            _emit(args, {"label": args.label, "case": "coh", "sfreq": sfreq, "W": W, "nperseg": nper, "pairs": args.pairs, "hops": n,
                         "segments": nseg, "kernels": eng.kernels(7), "stage_ms": ms, "wall_ms": wall,
                         "ns_per_segment": round(ms["median"] * 1e6 / (n * args.pairs * nseg), 2), "finite": finite})
            eng.close()
            del x
            torch.cuda.empty_cache()
    else:
        C, sfreq, W = args.channels, 30000, 30000
        hop = sfreq // 10
        names = [f"ch{i:03d}" for i in range(C)]
        x = _input(C, W, hop, n, dev)
        for with_stft in (False, True):
            s = NMSettings.get_default()
            s.postprocessing.feature_normalization = False
            s.preprocessing = []
            s.features.stft = with_stft
            feats = [f for f in s.features.get_enabled()]
            eng = HotPathEngine(s, names, float(sfreq), features=feats, window=W)
            ms, wall, finite = _timed(args, eng, x, W, hop, n, 2)
            _emit(args, {"label": args.label, "case": "plan", "stft": with_stft, "features": feats, "W": W, "channels": C, "hops": n,
                         "kernels_timeosc": eng.kernels(2), "timeosc_ms": ms, "wall_ms": wall, "finite": finite})
            eng.close()


if __name__ == "__main__":
    main()
