"""Device time of one Sim3Solver launch sequence (orb_sim3solver_iterate_device: prepare, evaluate, select) for a
batch of loop candidates: torch CUDA events, the median of `--launches` launches after `--warmup`, each from a
fresh solver state.  Two cases: every iteration forced (min_inliers above any count, so nothing stops early), and
LoopClosing's parameters with maxk = max_iterations.  There is no CPU baseline for this call (the C++ oracle has
none): the numbers stand alone.

    python tools/time_sim3solver.py [--pairs 1024] [--corr 150] [--launches 20] [--warmup 3]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from orb_slam2_refactored_amd.sim3solver import sim3solver_iterate_device  # noqa: E402
from orb_slam2_refactored_amd.synth import make_sim3solver_batch  # noqa: E402

HOST = ("level_sigma2", "gt_s12", "outlier", "n_corr")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--corr", type=int, default=150)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    # forced: 90 % gross outliers leave fewer inliers than min_inliers = 20, so no hypothesis can succeed, while
    # nmatches stays far above it and the cap is max_iterations
    for case, frac in (("forced_300", 0.9), ("loop_closing", 0.2)):
        b = make_sim3solver_batch(0, n_corr=[a.corr] * a.pairs, outlier_frac=frac, max_iterations=300, maxk=300)
        dd = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) and k not in HOST else v)
              for k, v in b.items()}
        out = sim3solver_iterate_device(dd)
        ms = []
        for i in range(a.warmup + a.launches):
            out["iterations"].zero_()
            out["max_inliers"].zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sim3solver_iterate_device(dd, out=out)
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        print(json.dumps({"case": case, "pairs": a.pairs, "corr": a.corr, "launch_ms_median": round(med, 3),
                          "launch_ms_min": round(min(ms), 3), "launch_ms_max": round(max(ms), 3),
                          "us_per_pair": round(1e3 * med / a.pairs, 2),
                          "mean_iterations": round(float(out["iterations"].float().mean()), 2),
                          "found": int((out["found"] == 1).sum())}))


if __name__ == "__main__":
    main()
