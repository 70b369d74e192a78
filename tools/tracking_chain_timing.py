"""Times TrackLocalMap's chain ("Tracking's per-frame state") for a batch of frames in two forms, alternating:
  resident   orbtl, SearchByProjection, apply_matches(MERGE), pose_edges, PoseOptimization, finish_pose(LOCAL_MAP), end_frame,
             drop_outliers on one stream, nothing copied in between;
  round trip the same kernels where they existed before the orbtf entries, with kp_match and the PoseOptimization result
             copied back, the gather and the statistics in vectorised numpy, and uploads.
Also each orbtf entry alone (device events), stereo_points on the same batch and on frames of 8192 keypoints.  Prints one
JSON line.
    python tools/tracking_chain_timing.py [--frames 256] [--kp 2000] [--mp 1500] [--steps 20]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--mp", type=int, default=1500)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import torch

    from orb_slam2_refactored_amd import tracking as T
    from orb_slam2_refactored_amd.local_map import LocalMap
    from orb_slam2_refactored_amd.matcher import search_by_projection_device
    from orb_slam2_refactored_amd.optimizer import pose_optimization_device
    from orb_slam2_refactored_amd.synth import make_local_map
    assert torch.cuda.is_available(), "needs a GPU"
    base = 8
    m, fr, kp = make_local_map(seed=3, n_keyframes=70, kf_cap=400, n_mappoints=a.mp, n_frames=base, kp_cap=a.kp,
                               matched=(a.kp // 4, a.kp // 8, a.kp // 3))
    reps = (a.frames + base - 1) // base
    tile = lambda v: np.ascontiguousarray(np.concatenate([v] * reps)[:a.frames])   # noqa: E731
    fr = {k: (tile(v) if isinstance(v, np.ndarray) else v) for k, v in fr.items()}
    kp = {k: (tile(v) if k != "scale_factors" else v) for k, v in kp.items()}
    F, cap, M = a.frames, a.kp, len(m["mp_bad"])
    rng = np.random.default_rng(0)
    kp["kp_uright"] = np.full((F, cap), -1.0, np.float32)
    extra = dict(frame_outlier=np.zeros((F, cap), np.uint8), kp_depth=rng.uniform(1, 20, (F, cap)).astype(np.float32),
                 kp_angle=np.zeros((F, cap), np.float32))
    inv_sigma2 = (1.0 / kp["scale_factors"].astype(np.float32) ** 2).astype(np.float32)
    cu = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()   # noqa: E731
    dm = {k: cu(v) for k, v in m.items()}
    dfr = {k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in fr.items()}
    dkp = {k: (cu(v) if k != "scale_factors" else v) for k, v in kp.items()}
    tfr = dict({k: dfr[k] for k in ("frame_n", "frame_mappoint", "pose", "camera", "bounds")},
               **{k: dkp[k] for k in ("kp_xy", "kp_octave", "kp_uright", "kp_desc")}, **{k: cu(v) for k, v in extra.items()})
    tm = dict({k: dm[k] for k in ("mp_xw", "mp_bad", "mp_nobs", "mp_desc", "kf_n", "kf_mappoint")},
              mp_found=torch.zeros(M, dtype=torch.int32, device="cuda"), mp_replaced=torch.full((M,), -1, dtype=torch.int32, device="cuda"))
    d_table, d_min_obs = cu(inv_sigma2), torch.full((F,), 3, dtype=torch.int32, device="cuda")
    start = {k: tfr[k].clone() for k in ("frame_mappoint", "frame_outlier", "pose")}
    start.update(local_kf=dfr["local_kf"].clone(), n_local_kf=dfr["n_local_kf"].clone(), mp_visible=dm["mp_visible"].clone())
    lm, s = LocalMap(dm), torch.cuda.current_stream()

    def reset():
        for k in ("frame_mappoint", "frame_outlier", "pose"):
            tfr[k].copy_(start[k])
        dfr["local_kf"].copy_(start["local_kf"])
        dfr["n_local_kf"].copy_(start["n_local_kf"])
        dm["mp_visible"].copy_(start["mp_visible"])

    def search():
        res = lm.track_local_map_device(dfr, a.mp)
        b = LocalMap.projection_batch(res, dkp, kp["scale_factors"], th=3.0)
        return res, search_by_projection_device(b)[0]

    def resident():
        res, kp_match = search()
        T.apply_matches(tfr, T.MERGE, kp_match, res["local_mp"], M)
        edges = T.pose_edges(tfr, tm, d_table)
        po = pose_optimization_device(edges)
        fin = T.finish_pose(tfr, tm, T.LOCAL_MAP, edges, po, False, True)
        end = T.end_frame(tfr, tm, 8.0, res["reference_kf"], d_min_obs)
        T.drop_outliers(tfr)
        return fin["n_inliers"].cpu().numpy(), end["counts"].cpu().numpy()   # what the host decides on

    xw64, nobs_h, bad_h = m["mp_xw"].astype(np.float64), m["mp_nobs"], m["mp_bad"]
    live = np.arange(cap)[None, :] < fr["frame_n"][:, None]

    def round_trip():
        res, kp_match = search()
        km = kp_match.cpu().numpy().reshape(F, cap)                      # copy 1: the search result
        local_mp, mp = res["local_mp"].cpu().numpy(), tfr["frame_mappoint"].cpu().numpy()
        ref_kf = res["reference_kf"].cpu().numpy()
        hit = live & (km >= 0)
        mp[hit] = np.take_along_axis(local_mp, np.maximum(km, 0), 1)[hit]
        has = live & (mp >= 0)                                            # the gather of Optimizer.cc:355-411
        f_idx, i_idx = np.nonzero(has)
        p = mp[has]
        pose = fr["pose"].astype(np.float64)
        batch = dict(edge_begin=np.concatenate([[0], np.cumsum(has.sum(1))]).astype(np.int32), pose_R=pose[:, :9].copy(),
                     pose_t=pose[:, 9:].copy(), cam=fr["camera"].astype(np.float64), xw=xw64[p],
                     obs=np.concatenate([kp["kp_xy"][has].astype(np.float64), kp["kp_uright"][has].astype(np.float64)[:, None]], 1),
                     inv_sigma2=inv_sigma2[kp["kp_octave"][has]].astype(np.float64))
        po = pose_optimization_device({k: cu(v) for k, v in batch.items()})   # upload 1
        out_e = po["outlier"].cpu().numpy()[:len(p)].astype(bool)             # copy 2: the result
        new_pose = np.concatenate([po["pose_R"].cpu().numpy(), po["pose_t"].cpu().numpy()], 1).astype(np.float32)
        outlier = np.zeros((F, cap), np.uint8)
        outlier[f_idx, i_idx] = out_e
        found = np.bincount(p[~out_e], minlength=M)
        n_inliers = np.bincount(f_idx[~out_e & (nobs_h[p] > 0)], minlength=F)
        mp[f_idx[out_e], i_idx[out_e]] = -1                                   # stereo; also the final removal
        nobs = np.where(mp >= 0, nobs_h[np.maximum(mp, 0)], -1)
        mp[(mp >= 0) & (nobs < 1)] = -1
        close = live & (extra["kp_depth"] > 0) & (extra["kp_depth"] < 8.0)
        counts = np.stack([(close & (mp >= 0)).sum(1), (close & (mp < 0)).sum(1)], 1)
        rows = m["kf_mappoint"][np.maximum(ref_kf, 0)]
        ok = (rows >= 0) & (np.arange(rows.shape[1])[None, :] < m["kf_n"][np.maximum(ref_kf, 0)][:, None])
        tracked = (ok & (bad_h[np.maximum(rows, 0)] == 0) & (nobs_h[np.maximum(rows, 0)] >= 3)).sum(1) * (ref_kf >= 0)
        tfr["frame_mappoint"].copy_(cu(mp))                                   # upload 2: the state the next frame reads
        tfr["frame_outlier"].copy_(cu(outlier))
        tfr["pose"].copy_(cu(new_pose))
        tm["mp_found"].add_(cu(found.astype(np.int32)))
        return n_inliers, np.concatenate([counts, tracked[:, None]], 1)

    def timed(fn):
        reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    for _ in range(3):
        ra, rb = timed(resident)[1], timed(round_trip)[1]
    agree = bool(np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]))
    t_res, t_trip = [], []
    for _ in range(a.steps):   # alternating
        t_res.append(timed(resident)[0])
        t_trip.append(timed(round_trip)[0])

    def events(fn, n=20):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3   # microseconds per call

    reset()
    res, kp_match = search()
    edges = T.pose_edges(tfr, tm, d_table)
    po = pose_optimization_device(edges)
    last = dict(tfr, frame_mappoint=tfr["frame_mappoint"].clone())
    vel = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.01], dtype=torch.float32, device="cuda").repeat(F, 1).contiguous()
    base_l = torch.full((F,), 0.08, dtype=torch.float32, device="cuda")
    cur = dict(tfr, frame_mappoint=tfr["frame_mappoint"].clone(), pose=tfr["pose"].clone())
    e_out = edges
    per = {
        "apply_matches": lambda: T.apply_matches(tfr, T.MERGE, kp_match, res["local_mp"], M),
        "pose_edges": lambda: T.pose_edges(tfr, tm, d_table, out=e_out),
        "finish_pose": lambda: T.finish_pose(tfr, tm, T.LOCAL_MAP, edges, po, False, False),
        "end_frame": lambda: T.end_frame(tfr, tm, 8.0, res["reference_kf"], d_min_obs),
        "drop_outliers": lambda: T.drop_outliers(tfr),
        "motion_project": lambda: T.motion_project(cur, last, tm, vel, base_l, False),
        "stereo_points": lambda: T.stereo_points(tfr, tm, T.VO, 8.0),
        "pose_optimization": lambda: pose_optimization_device(edges),
        "local_map_and_search": search,
    }
    us = {k: round(events(fn), 1) for k, fn in per.items()}
    # stereo_points at the largest frame: F frames of 8192 keypoints, no map point held, depths around th_depth
    big = dict(frame_n=torch.full((F,), 8192, dtype=torch.int32, device="cuda"),
               frame_mappoint=torch.full((F, 8192), -1, dtype=torch.int32, device="cuda"), pose=tfr["pose"], camera=tfr["camera"],
               kp_xy=cu(rng.uniform(0, 600, (F, 8192, 2)).astype(np.float32)), kp_depth=cu(rng.uniform(1, 20, (F, 8192)).astype(np.float32)))
    us["stereo_points_8192"] = round(events(lambda: T.stereo_points(big, tm, T.VO, 8.0), 5), 1)
    med = lambda v: round(float(np.median(v)), 3)   # noqa: E731
    print(json.dumps(dict(frames=F, kp=cap, mp_cap=a.mp, edges=int(edges["edge_begin"][-1].item()), results_agree=agree,
                          resident_ms=med(t_res), resident_min_ms=round(min(t_res), 3), round_trip_ms=med(t_trip),
                          round_trip_min_ms=round(min(t_trip), 3), per_call_us=us)))


if __name__ == "__main__":
    main()
