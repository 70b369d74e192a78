"""Device time of one Optimizer::OptimizeEssentialGraph call (orbba_optimize_essential_graph) on a drifting keyframe
chain closed by a loop, at 13, 128 and ORBBA_EG_MAX_KEYFRAMES keyframes: the device entry on resident tensors between
one event pair (all 1 063 launches back to back, nothing copied), the wall time of the host entry (copies included),
both as the median of the repeats after a warm-up call, and the per-kernel split from orbba_essential_graph_profile,
which brackets every launch with an event pair and so runs slower than either.  Prints one JSON line per size.

    python tools/time_essential_graph.py [--sizes 13 128 512] [--repeats 5]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from essential_graph_cases import make_graph  # noqa: E402
from orb_slam2_refactored_amd.optimizer import (EG_MAX_KEYFRAMES, OptimizeEssentialGraph,  # noqa: E402
                                                optimize_essential_graph_device)

_ARRAYS = ("vertex_sim3", "edge_sim3", "edge_i", "edge_j", "edge_table", "points", "point_ref")


def device_ms(g, repeats):
    """Event-timed device entry on resident tensors: milliseconds per call."""
    import numpy as np
    import torch
    d = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if k in _ARRAYS else v) for k, v in g.items()}
    out = optimize_essential_graph_device(d)
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        optimize_essential_graph_device(d, out=out)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[13, 128, EG_MAX_KEYFRAMES])
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.init()   # before the library's first device call: torch brings its own HIP runtime up first
    for n in a.sizes:
        g = make_graph(1, n_kf=n, n_corrected=max(2, n // 10), covis=3, n_points=20 * n, step_deg=360.0 / n)
        OptimizeEssentialGraph(g)   # warm-up: allocations, code load
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            r = OptimizeEssentialGraph(g)
            ts.append((time.perf_counter() - t0) * 1e3)
        dev = device_ms(g, a.repeats)
        p = OptimizeEssentialGraph(g, profile=True)
        print(json.dumps(dict(keyframes=n, edges=len(g["edge_i"]), points=len(g["points"]), iterations=r["iterations"],
                              trials=r["trials"], chi2=r["chi2"], device_ms_median=statistics.median(dev), device_ms_min=min(dev),
                              call_ms_median=statistics.median(ts), call_ms_min=min(ts),
                              kernel_ms={k: round(v, 4) for k, v in p["kernel_ms"].items()})), flush=True)


if __name__ == "__main__":
    main()
