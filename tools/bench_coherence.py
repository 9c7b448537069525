"""Coherence kernel time at the headline shape: 256 channels at 1 kHz, 1000-sample windows, hop 100, batches of 1024 hops.

Two pair layouts (128 disjoint neighbour pairs; one seed paired with the other 255 channels), nperseg 128 and 256.
Reports the coherence stage's kernel time per batch from the plan's HIP events (nmx_last_timing_ms stage 7), the
algorithmic bytes (4 W per DISTINCT channel window read + the coherence outputs written) and their fraction of the
6.29 TB/s HBM peak.  One JSON line per configuration.

    python tools/bench_coherence.py [--reps 20]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

HBM_TBS = 6.29


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hops", type=int, default=1024)
    args = ap.parse_args()
    from py_neuromodulation_amd import NMSettings
    from py_neuromodulation_amd.engine import HotPathEngine

    C, W, hop, sfreq = 256, 1000, 100, 1000.0
    n = args.hops
    T = W + (n - 1) * hop
    x = np.random.default_rng(0).standard_normal((C, T)).astype(np.float32)
    starts = np.arange(n, dtype=np.int64) * hop
    names = [f"ch{i:03d}" for i in range(C)]
    layouts = {"disjoint128": [[names[2 * i], names[2 * i + 1]] for i in range(C // 2)],
               "seed255": [[names[0], names[i]] for i in range(1, C)]}
    for layout, pairs in layouts.items():
        for nperseg in (128, 256):
            s = NMSettings.get_default()
            s.reset()
            s.features.coherence = True
            s.coherence_settings.channels = pairs
            s.coherence_settings.nperseg = nperseg
            e = HotPathEngine(s, names, sfreq, features=["coherence"], window=W)
            e.process_batch(x, starts)   # warm-up (plan buffers, code objects)
            ms = []
            for _ in range(args.reps):
                e.process_batch(x, starts)
                ms.append(e.timing_ms(7))
            distinct = len({c for p in e.coh_pairs for c in p})
            nbytes = n * (4 * W * distinct + 4 * e.n_outputs)
            med = float(np.median(ms))
            print(json.dumps({"layout": layout, "nperseg": nperseg, "pairs": len(e.coh_pairs), "hops": n,
                              "kernel": e.kernels(7), "kernel_ms_median": round(med, 4),
                              "kernel_ms_min": round(float(np.min(ms)), 4), "algorithmic_bytes": nbytes,
                              "TBps": round(nbytes / med / 1e9, 4),
                              "fraction_of_hbm_peak": round(nbytes / med / 1e9 / HBM_TBS, 4)}), flush=True)
            e.close()


if __name__ == "__main__":
    main()
