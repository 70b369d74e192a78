"""Device time of one Optimizer::OptimizeSim3 launch (orbba_optimize_sim3_device) for a batch of loop
candidates: torch CUDA events, the median of `--launches` launches after `--warmup`.  There is no CPU baseline
for this call (the C++ oracle has none): the number stands alone.

    python tools/time_optsim3.py [--pairs 1024] [--corr 150] [--launches 20] [--warmup 3]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from orb_slam2_refactored_amd.optimizer import optimize_sim3_device  # noqa: E402
from orb_slam2_refactored_amd.synth import make_optsim3_batch  # noqa: E402

HOST = ("inv_level_sigma2", "max_chi2", "fix_scale")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--corr", type=int, default=150)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    b = make_optsim3_batch(0, n_corr=[a.corr] * a.pairs, n_outliers=[a.corr // 10] * a.pairs)
    d = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) and k not in HOST else v)
         for k, v in b.items()}
    out = optimize_sim3_device(d)
    ms = []
    for i in range(a.warmup + a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        optimize_sim3_device(d, out=out)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    it = out["iterations"].cpu().numpy()
    print(json.dumps({"pairs": a.pairs, "corr": a.corr, "launch_ms_median": round(med, 3), "launch_ms_min": round(min(ms), 3),
                      "launch_ms_max": round(max(ms), 3), "us_per_pair": round(1e3 * med / a.pairs, 2),
                      "mean_lm_iterations": round(float(it.sum(1).mean()), 2),
                      "mean_inliers": round(float(out["n_inliers"].float().mean()), 1)}))


if __name__ == "__main__":
    main()
