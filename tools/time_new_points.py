"""Device time of LocalMapping::CreateNewMapPoints' neighbour loop (orblm_create_new_map_points_device) on the generator's
keyframes: torch CUDA events, the median of `--launches` launches after `--warmup`, each from the same MapPoint flags.
Four figures per shape: prepare alone (all rounds' pairs), one round's triangulation alone (on the loop's own match12),
the whole loop, and the same rounds' searches alone (frozen flags) for comparison.  One JSON line.  There is no earlier
device path for this call: the numbers stand alone.

    python tools/time_new_points.py [--rounds 20] [--kf1 64] [--keypoints 2000] [--mode mono] [--launches 20] [--warmup 3]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from orb_slam2_refactored_amd.mapping import (create_new_map_points_device, prepare_pairs_device,  # noqa: E402
                                              triangulate_matches_device)
from orb_slam2_refactored_amd.matcher import search_for_triangulation_batch_device  # noqa: E402
from orb_slam2_refactored_amd.synth import make_new_points_batch  # noqa: E402

DEVICE = ("kps1", "kps2", "counts1", "counts2", "uright1", "depth1", "uright2", "depth2", "has_mappoint2", "mp_xw2", "pose1",
          "pose2", "camera1", "camera2", "frame1", "frame2")


def timed(fn, launches, warmup):
    ms = []
    for i in range(warmup + launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn(True)    # untimed: put the flags back
        e0.record()
        fn(False)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--kf1", type=int, default=64)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--mode", default="mono")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    R, P, cap = a.rounds, a.kf1, a.keypoints
    b = make_new_points_batch(0, n_kf1=P, n_rounds=R, cap=cap, mode=a.mode, short_frac=0.1)
    d = {k: v for k, v in b.items() if k not in DEVICE and k not in ("desc", "has_mappoint")}
    for k in DEVICE:
        v = b.get(k)
        d[k] = None if v is None else torch.from_numpy(np.ascontiguousarray(v).view(np.int32).reshape(v.shape + (7,))
                                                       if k.startswith("kps") else np.ascontiguousarray(v)).cuda()
    desc = torch.from_numpy(b["desc"]).cuda()
    flags0 = torch.from_numpy(b["has_mappoint"]).cuda()
    flags = flags0.clone()
    search = dict(desc1=desc, desc2=desc)
    out = create_new_map_points_device(d, search, flags, flags, plan=(b["frame1"], b["frame2"]))
    torch.cuda.synchronize()
    created, matches = int(out["n_created"].sum()), int((out["match12"] >= 0).sum())
    flat = dict(d, frame1=d["frame1"].reshape(-1), frame2=d["frame2"].reshape(-1))
    pairs = prepare_pairs_device(flat)
    one = dict(d, frame1=d["frame1"][0].contiguous(), frame2=d["frame2"][0].contiguous())
    pr0 = {k: v[:P].contiguous() for k, v in pairs.items()}
    m0 = out["match12"][:P].contiguous()
    kps, cnt = d["kps1"], d["counts1"]
    tri_out = search_for_triangulation_batch_device(kps, desc, cnt, kps, desc, cnt, pairs["F12"][:P], pairs["ep2"][:P],
                                                    b["scale_factors2"], b["sigma2_2"], frame1=pairs["frame1"][:P].contiguous(),
                                                    frame2=pairs["frame2"][:P].contiguous(), uright1=d["uright1"], uright2=d["uright2"],
                                                    has_mappoint1=flags0, has_mappoint2=flags0)

    def loop(reset):
        if reset:
            flags.copy_(flags0)
        else:
            create_new_map_points_device(d, search, flags, flags, out=out)

    def prep(reset):
        if not reset:
            prepare_pairs_device(flat, out=pairs)

    tout = triangulate_matches_device(one, pr0, m0)

    def tri(reset):
        if not reset:
            triangulate_matches_device(one, pr0, m0, out=tout)

    def searches(reset):
        if not reset:
            for r in range(R):
                sl = slice(r * P, (r + 1) * P)
                search_for_triangulation_batch_device(kps, desc, cnt, kps, desc, cnt, pairs["F12"][sl], pairs["ep2"][sl],
                                                      b["scale_factors2"], b["sigma2_2"], frame1=pairs["frame1"][sl],
                                                      frame2=pairs["frame2"][sl], uright1=d["uright1"], uright2=d["uright2"],
                                                      has_mappoint1=flags0, has_mappoint2=flags0, out=tri_out)

    res = {"rounds": R, "kf1": P, "keypoints": cap, "mode": a.mode, "matches": matches, "created": created,
           "prepare_ms": timed(prep, a.launches, a.warmup), "triangulate_round_ms": timed(tri, a.launches, a.warmup),
           "loop_ms": timed(loop, a.launches, a.warmup), "searches_ms": timed(searches, a.launches, a.warmup)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
