"""Named cases for Tracking's local map (tests/test_local_map_*.py): a map (orbtl_map's slot tables), a batch of five frames
and their keypoint arrays, from orb_slam2_refactored_amd.synth.make_local_map.  batch(case, F) is the case's first F frames.

  mixed  K = 70 keyframes (past one wavefront), kf_cap = 96, about 700 map points
  long   K = 130 close together: most frames vote for more than 80 keyframes (the walk stops at its first element), two vote
         for fewer (both parts of the list)
  edges  mixed's kind of map plus hand-placed points in frame 0's reference keyframe: one on each side of each comparison
         of IsInFrustum and of both level clamps (EDGE_POINTS names them and the test each must leave at)

No local point of any frame has log(maxDistance / dist) / logScaleFactor within 1e-6 of an integer, so no point has to be
left out of a comparison (tests/test_local_map_ref.py asserts it on every case)."""
import functools

import numpy as np

import local_map_ref as R
from orb_slam2_refactored_amd.synth import local_map_tables, make_local_map

CASES = ("mixed", "long", "edges")
BATCHES = (1, 3, 5)
MP_CAP = {"mixed": 700, "long": 900, "edges": 720}

# name: (camera-frame position, what to do with the point, the IsInFrustum test it leaves at)
EDGE_POINTS = {
    "depth_neg": ((0.0, 0.0, -0.01), {}, R.DEPTH), "depth_pos": ((0.0, 0.0, 0.01), {}, R.PASS),
    "bounds_in": ((3.19, 0.0, 5.0), {}, R.PASS), "bounds_out": ((3.21, 0.0, 5.0), {}, R.BOUNDS),
    "bounds_top_in": ((0.0, -2.39, 5.0), {}, R.PASS), "bounds_top_out": ((0.0, -2.41, 5.0), {}, R.BOUNDS),
    "near_in": ((0.0, 0.0, 6.0), {"min": 6.0 / 0.8 * 0.999}, R.PASS), "near_out": ((0.0, 0.0, 6.0), {"min": 6.0 / 0.8 * 1.001}, R.DISTANCE),
    "far_in": ((0.0, 0.0, 6.0), {"max": 6.0 / 1.2 * 1.001}, R.PASS), "far_out": ((0.0, 0.0, 6.0), {"max": 6.0 / 1.2 * 0.999}, R.DISTANCE),
    "cos_in": ((0.0, 0.0, 6.0), {"cos": 0.51}, R.PASS), "cos_out": ((0.0, 0.0, 6.0), {"cos": 0.49}, R.VIEW_COS),
    "level_low": ((0.0, 0.0, 6.0), {"max": 5.5}, R.PASS),      # ratio < 1: ceil gives <= 0, clamped to 0
    "level_high": ((0.0, 0.0, 6.0), {"max": 6.0 * 1.2 ** 9.5}, R.PASS),   # level 10 clamped to n_levels - 1
}


def _edges(m, fr):
    """Appends EDGE_POINTS to the map, observed by the keyframe frame 0 votes for most; returns name -> slot."""
    o = R.track_local_map(m, fr, 4096, frames=[0])
    k = int(o["reference_kf"][0])
    assert k >= 0
    P = fr["pose"][0].astype(np.float64)
    Rcw, t = P[:9].reshape(3, 3), P[9:]
    M0, n = len(m["mp_bad"]), len(EDGE_POINTS)
    extra = {key: [] for key in ("mp_xw", "mp_normal", "mp_max_min")}
    for xc, how, _ in EDGE_POINTS.values():
        xc = np.array(xc)
        xw = Rcw.T @ (xc - t)
        d = np.linalg.norm(xc)
        po = (xw - (-Rcw.T @ t)) / d
        c = how.get("cos", 0.9)
        side = np.cross(po, [0.0, 1.0, 0.0])
        side /= np.linalg.norm(side)
        extra["mp_xw"].append(xw)
        extra["mp_normal"].append(c * po + np.sqrt(1 - c * c) * side)
        extra["mp_max_min"].append((how.get("max", d * 1.2 ** 2.5), how.get("min", d * 0.3)))
    for key, rows in extra.items():
        m[key] = np.concatenate([m[key], np.array(rows, np.float32)])
    rng = np.random.default_rng(99)
    m["mp_desc"] = np.concatenate([m["mp_desc"], rng.integers(0, 256, (n, 32), dtype=np.uint8)])
    m["mp_visible"] = np.concatenate([m["mp_visible"], np.arange(n, dtype=np.int32)])
    kfm, kfn = m["kf_mappoint"].copy(), m["kf_n"].copy()
    keep = min(int(kfn[k]), kfm.shape[1] - n)      # the hand points take the row's last places
    kfm[k, keep:keep + n] = M0 + np.arange(n)
    kfn[k] = keep + n
    m.update(local_map_tables(kfm, kfn, M0 + n, kf_bad=m["kf_bad"], mp_bad=np.concatenate([m["mp_bad"], np.zeros(n, np.uint8)]),
                              parent=m["kf_parent"]))
    return {name: M0 + i for i, name in enumerate(EDGE_POINTS)}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(map, frames, keypoints, mp_cap[, edge_slots]); treat it as read-only (batch() copies what a call updates)."""
    if name == "long":
        m, fr, kp = make_local_map(seed=1, n_keyframes=130, step=0.06, n_mappoints=900, n_frames=5)
    else:
        m, fr, kp = make_local_map(seed={"mixed": 0, "edges": 2}[name], n_frames=5)
    c = dict(map=m, frames=fr, keypoints=kp, mp_cap=MP_CAP[name])
    if name == "edges":
        c["edge_slots"] = _edges(m, fr)
    return c


def batch(c, F, frames=None):
    """(map, frames, keypoints) of the case's first F frames (or the frames `frames`), as fresh copies."""
    idx = list(range(F)) if frames is None else list(frames)
    m = {k: v.copy() for k, v in c["map"].items()}
    fr = {k: (v[idx].copy() if isinstance(v, np.ndarray) else v) for k, v in c["frames"].items()}
    kp = {k: (v[idx].copy() if k != "scale_factors" else v) for k, v in c["keypoints"].items()}
    return m, fr, kp


@functools.lru_cache(maxsize=None)
def expected(name, F):
    """The restatement's outputs for batch(case(name), F): computed once, shared, left unchanged."""
    c = case(name)
    m, fr, _ = batch(c, F)
    return R.track_local_map(m, fr, c["mp_cap"])
