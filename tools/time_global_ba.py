"""Time of one LM trial of Optimizer::BundleAdjustment (orbba_bundle_adjustment) on each path of the reduced system's
solve, the single workgroup (ORBBA_GBA_SOLVE=single: ba_solve_global_kernel, the kernel orbba_local_ba uses) and the
grid-wide LDL^T (=grid: csrc/ldlt_grid.h), on make_ba_problem maps with np free keyframes.  The two paths share every
other launch of a trial, so the difference of the columns is the difference of the solves.  Per path: the wall time
of the host entry (10 iterations, no robust kernels, as GlobalBundleAdjustemnt calls it) divided by the trials it ran,
for each of --repeats calls after a warm-up; median, minimum and maximum (the run-to-run spread).  --oracle adds the
CPU figure that exists for the same problem: the oracle's LocalBundleAdjustment per LM iteration, one run.  Prints
one JSON line per size.

make_ba_problem always fixes keyframe 0 (the gauge, id == 0), so n_kf keyframes with n_fixed = 0 are n_kf - 1 free.

    python tools/time_global_ba.py [--sizes 23,1000 65,2600 129,5200 257,10300 512,20500 200,20000] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from orb_slam2_refactored_amd.optimizer import BundleAdjustment  # noqa: E402
from orb_slam2_refactored_amd.synth import make_ba_problem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["23,1000", "65,2600", "129,5200", "257,10300", "512,20500", "200,20000"],
                    help="keyframes,points")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--oracle", action="store_true")
    a = ap.parse_args()
    for size in a.sizes:
        n_kf, n_pts = (int(v) for v in size.split(","))
        # (keyframe 0 is fixed by make_ba_problem itself; a small yaw keeps a long path's points in view)
        pr = make_ba_problem(1, n_kf=n_kf, n_pts=n_pts, n_fixed=0, yaw_per_kf=min(0.5, 40.0 / n_kf))
        out = dict(keyframes=n_kf, free_keyframes=n_kf - 1, points=n_pts, edges=len(pr["edge_point"]))
        for path in ("single", "grid"):
            os.environ["ORBBA_GBA_SOLVE"] = path   # read per call
            BundleAdjustment(pr, a.iterations, robust=False)   # warm-up: allocations, code load
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                r = BundleAdjustment(pr, a.iterations, robust=False)
                ts.append((time.perf_counter() - t0) * 1e3 / max(r["trials"], 1))
            out[path] = dict(iterations=r["iterations"], trials=r["trials"], call_ms=statistics.median(ts) * max(r["trials"], 1),
                             trial_ms_median=statistics.median(ts), trial_ms_min=min(ts), trial_ms_max=max(ts))
        del os.environ["ORBBA_GBA_SOLVE"]
        if a.oracle:
            import oracle_api as O
            t0 = time.perf_counter()
            o = O.local_ba(pr)
            dt = (time.perf_counter() - t0) * 1e3
            out.update(oracle_local_ba_ms=dt, oracle_iterations=list(o["iterations"]),
                       oracle_ms_per_iteration=dt / max(sum(o["iterations"]), 1))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
