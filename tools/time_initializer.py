"""Device time of one Initializer launch sequence (orb_initializer_initialize_device: prepare, evaluate, select,
reconstruct, finish) for a batch of monocular initialisation pairs: torch CUDA events, the median of `--launches`
launches after `--warmup`, with Tracking::MonocularInitialization's parameters (sigma 1.0, 200 iterations).  One JSON
line per batch size.  There is no earlier device path and no CPU baseline for this call: the numbers stand alone.

    python tools/time_initializer.py [--pairs 1024] [--matches 150] [--iterations 200] [--launches 20] [--warmup 3]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from orb_slam2_refactored_amd.initializer import initializer_initialize_device  # noqa: E402
from orb_slam2_refactored_amd.synth import make_initializer_batch  # noqa: E402

HOST = ("gt_r21t21",)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1024])
    ap.add_argument("--matches", type=int, default=150)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for F in a.pairs:
        b = make_initializer_batch(0, n_corr=[a.matches] * F, scene=("plane", "general", "rotation"), outlier_frac=0.2,
                                   max_iterations=a.iterations)
        dd = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) and k not in HOST else v)
              for k, v in b.items()}
        out = initializer_initialize_device(dd)
        ms = []
        for i in range(a.warmup + a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            initializer_initialize_device(dd, out=out)
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        print(json.dumps({"pairs": F, "matches": a.matches, "max_iterations": a.iterations, "launch_ms_median": round(med, 3),
                          "launch_ms_min": round(min(ms), 3), "launch_ms_max": round(max(ms), 3),
                          "us_per_pair": round(1e3 * med / F, 2), "found": int((out["found"][:F] == 1).sum()),
                          "model_h": int((out["model"][:F] == 0).sum())}))


if __name__ == "__main__":
    main()
