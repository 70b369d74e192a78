"""Times orbm_search_by_sim3_device at the LoopClosing::FindLoopInCandidateKFs shape (8 candidate pairs x
2000 keypoints a side, about half of the slots holding map points, th 7.5) and
orbm_distinctive_descriptors_device at the LocalMapping::SearchInNeighbors shape (1500 map points x U{2..15}
observations) and at a loop-closing shape (200 points x 100 observations).  Event timing on the current
stream, a warm-up, the median of --runs enqueues.

    python tools/time_sim3.py [--pairs 8 --kp 2000 --runs 30 --warmup 5]
Prints one JSON line: the three medians (ms) with min / max."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from time_fuse import event_ms, to_device   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20 (a median of fewer says little)")
    import torch
    from orb_slam2_refactored_amd.matcher import compute_distinctive_descriptors_device, search_by_sim3_device
    from orb_slam2_refactored_amd.synth import make_observation_sets, make_sim3_batch
    assert torch.cuda.is_available(), "needs a GPU"
    sb = to_device(make_sim3_batch(7, n_pairs=a.pairs, n_kp1=a.kp, n_kp2=a.kp, th=7.5), host=("scale_factors",))
    outs = search_by_sim3_device(sb)
    rng = np.random.default_rng(7)
    res = {"sim3_shape": [a.pairs, a.kp, a.kp], "runs": a.runs}
    t = event_ms(lambda: search_by_sim3_device(sb, *outs), a.runs, a.warmup)
    res["sim3_ms"] = {"median": float(np.median(t)), "min": min(t), "max": max(t)}
    res["n_found_mean"] = float(outs[3].float().mean())
    res["mp_valid_share"] = float(sb["mp1_valid"].float().mean())
    for name, sets in (("distinct_local_mapping", make_observation_sets(7, 1500, rng.integers(2, 16, 1500))),
                       ("distinct_loop_closing", make_observation_sets(8, 200, 100))):
        d, bg = torch.from_numpy(sets["desc"]).cuda(), torch.from_numpy(sets["begin"]).cuda()
        o = compute_distinctive_descriptors_device(d, bg)
        t = event_ms(lambda: compute_distinctive_descriptors_device(d, bg, *o), a.runs, a.warmup)
        res[name + "_ms"] = {"median": float(np.median(t)), "min": min(t), "max": max(t), "rows": int(sets["begin"][-1])}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
