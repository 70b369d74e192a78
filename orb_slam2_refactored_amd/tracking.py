"""Tracking's per-frame state (src/Tracking.cc: DiscardOutliers :187-211, TrackWithMotionModel's setup :220-240, the counts of
NeedNewKeyFrame :490-511, TrackLocalMap's statistics :664-680, CreateMapPoints / CreateMapPointsVO :685-786, GetReplaced
:808-814, StereoInitialization :980-997, the end of Update :1259-1313; the gather of src/Optimizer.cc:355-411) over the
gfx950 C-ABI (orbtf_*, include/orbslam2_amd.h), batched over frames.

A batch of frames is a dict with FRAME_KEYS (stride kp_cap; an entry needs only the arrays it reads), the map a dict with
MAP_KEYS.  Every function takes numpy arrays (synchronous, `device=` the GPU index) or CUDA tensors (enqueue only, on
`stream=` or torch's current stream) and works in place: the tables it updates are the arrays it was given, which must be
contiguous and of the listed dtype.  Outputs are returned as a dict (`out=` to reuse one)."""
import ctypes as C

import numpy as np

from ._lib import (OrbtfCreated, OrbtfEdges, OrbtfFrames, OrbtfMap, OrbtfMotion, PoseResult, check, lib, ptr, stream_ptr)

MERGE, REPLACE = 0, 1
DISCARD, LOCAL_MAP = 0, 1
KEYFRAME, VO, INIT = 0, 1, 2
MAX_KP = 8192

# name: (dtype, shape); F frames, M map points, K keyframes, E = F * kp_cap edge rows
FRAME_KEYS = {
    "frame_n": (np.int32, ("F",)), "frame_mappoint": (np.int32, ("F", "kp_cap")), "frame_outlier": (np.uint8, ("F", "kp_cap")),
    "pose": (np.float32, ("F", 12)), "camera": (np.float32, ("F", 5)), "bounds": (np.float32, ("F", 4)),
    "kp_xy": (np.float32, ("F", "kp_cap", 2)), "kp_octave": (np.int32, ("F", "kp_cap")), "kp_uright": (np.float32, ("F", "kp_cap")),
    "kp_depth": (np.float32, ("F", "kp_cap")), "kp_angle": (np.float32, ("F", "kp_cap")), "kp_desc": (np.uint8, ("F", "kp_cap", 32)),
}
MAP_KEYS = {
    "mp_xw": (np.float32, ("M", 3)), "mp_bad": (np.uint8, ("M",)), "mp_nobs": (np.int32, ("M",)), "mp_found": (np.int32, ("M",)),
    "mp_replaced": (np.int32, ("M",)), "mp_desc": (np.uint8, ("M", 32)), "kf_n": (np.int32, ("K",)),
    "kf_mappoint": (np.int32, ("K", "kf_cap")),
}
EDGE_KEYS = {
    "edge_begin": (np.int32, ("F1",)), "pose_R": (np.float64, ("F", 9)), "pose_t": (np.float64, ("F", 3)),
    "cam": (np.float64, ("F", 5)), "xw": (np.float64, ("E", 3)), "obs": (np.float64, ("E", 3)), "inv_sigma2": (np.float64, ("E",)),
    "edge_kp": (np.int32, ("E",)),
}
MOTION_KEYS = {
    "motion": (np.int32, ("F",)), "kp_begin": (np.int32, ("F1",)), "mp_begin": (np.int32, ("F1",)),
    "kp_claimed": (np.uint8, ("F", "kp_cap")), "mp_valid": (np.uint8, ("F", "last_cap")), "mp_proj": (np.float32, ("F", "last_cap", 3)),
    "mp_octave": (np.int32, ("F", "last_cap")), "mp_desc": (np.uint8, ("F", "last_cap", 32)),
    "mp_has_obs": (np.uint8, ("F", "last_cap")), "mp_angle": (np.float32, ("F", "last_cap")),
}
CREATED_KEYS = {
    "created_kp": (np.int32, ("F", "kp_cap")), "created_xw": (np.float32, ("F", "kp_cap", 3)), "n_created": (np.int32, ("F",)),
    "n_processed": (np.int32, ("F",)),
}
FINISH_KEYS = {"n_inliers": (np.int32, ("F",)), "discarded": (np.int32, ("F", "kp_cap")), "n_discarded": (np.int32, ("F",))}
END_KEYS = {"n_observations": (np.int32, ("F", "kp_cap")), "counts": (np.int32, ("F", 3))}
RESULT_KEYS = {"pose_R": (np.float64, ("F", 9)), "pose_t": (np.float64, ("F", 3)), "n_inliers": (np.int32, ("F",)),
               "outlier": (np.uint8, (None,))}


def _is_device(a):
    return not isinstance(a, np.ndarray)


def _shape(spec, d):
    return tuple(d[s] if isinstance(s, str) else s for s in spec)


def _addr(a, dtype, name, want, on_device):
    """The address of array `a` after checking its place, dtype, layout and shape (None in `want`: free)."""
    if on_device:
        import torch
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            raise ValueError(f"{name} must be a GPU tensor")
        if a.dtype != getattr(torch, np.dtype(dtype).name) or not a.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {np.dtype(dtype).name} tensor")
        shape, address = tuple(a.shape), a.data_ptr()
    else:
        if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous:
            raise ValueError(f"{name} must be a C-contiguous numpy array of {np.dtype(dtype).name}")
        shape, address = a.shape, a.ctypes.data
    if len(shape) != len(want) or any(w is not None and w != s for s, w in zip(shape, want)):
        raise ValueError(f"{name} must have shape {want}, not {tuple(shape)}")
    return address


def _dims(fr, m=None):
    for k in ("frame_n", "frame_mappoint"):
        if fr.get(k) is None:
            raise ValueError(f"{k} is required")
    if len(fr["frame_mappoint"].shape) != 2:
        raise ValueError("frame_mappoint must have two dimensions")
    F, cap = (int(s) for s in fr["frame_mappoint"].shape)
    d = {"F": F, "F1": F + 1, "kp_cap": cap, "E": F * cap, "M": 0, "K": 0, "kf_cap": 1}
    if m is not None:
        sized = [m[k] for k in ("mp_nobs", "mp_xw", "mp_bad", "mp_replaced") if m.get(k) is not None]
        d["M"] = int(sized[0].shape[0]) if sized else 0
        if m.get("kf_mappoint") is not None:
            d["K"], d["kf_cap"] = (int(s) for s in m["kf_mappoint"].shape)
    return d


def _fill(struct, head, keys, arrays, d, on_device, need=()):
    """A C struct from a dict: the arrays present are checked and bound, the others stay NULL (the library says which
    ones an entry requires); `need` names those this module itself relies on."""
    for k in need:
        if arrays.get(k) is None:
            raise ValueError(f"{k} is required")
    return struct(*head, *[None if arrays.get(k) is None else _addr(arrays[k], dt, k, _shape(sp, d), on_device)
                           for k, (dt, sp) in keys.items()])


def _frames(fr, d, on_device):
    return _fill(OrbtfFrames, (d["F"], d["kp_cap"]), FRAME_KEYS, fr, d, on_device)


def _map(m, d, on_device):
    return _fill(OrbtfMap, (d["K"], d["M"], d["kf_cap"]), MAP_KEYS, m or {}, d, on_device)


def _new(keys, d, like, out, zero=False):
    """The output arrays of `keys`: those of `out`, or new ones beside `like` (numpy: zeros)."""
    if out is not None:
        return out
    if _is_device(like):
        import torch
        make = torch.zeros if zero else torch.empty
        return {k: make(_shape(sp, d), dtype=getattr(torch, np.dtype(dt).name), device=like.device) for k, (dt, sp) in keys.items()}
    return {k: np.zeros(_shape(sp, d), dt) for k, (dt, sp) in keys.items()}


def _call(name, on_device, args, stream, device):
    fn = getattr(lib(), name + ("_device" if on_device else ""))
    check(fn(*args, stream_ptr(stream) if on_device else int(device)), fn.__name__)


def apply_matches(frames: dict, mode: int, kp_match, src, n_mappoints: int, src_row=None, stream=None, device: int = 0) -> None:
    """frame_mappoint[f][i] = src[row][kp_match[f][i]] (row = src_row[f], or f): MERGE writes where kp_match >= 0 (the
    local-map search, src/ORBmatcher.cc:376), REPLACE also -1 where there is none (src/Tracking.cc:232-239, :273).
    kp_match (F, kp_cap) int32 (a flat search result of F * kp_cap is taken as that); src (n_rows, src_cap) int32: local_mp,
    the last frames' frame_mappoint or kf_mappoint; it must not be the frame_mappoint written."""
    d = _dims(frames)
    dev = _is_device(frames["frame_mappoint"])
    kp_match = kp_match.reshape(d["F"], d["kp_cap"]) if kp_match.shape[0] == d["E"] and len(kp_match.shape) == 1 else kp_match
    if len(src.shape) != 2:
        raise ValueError("src must have two dimensions")
    fs = _frames(frames, d, dev)
    args = [C.byref(fs), int(mode), _addr(kp_match, np.int32, "kp_match", (d["F"], d["kp_cap"]), dev),
            _addr(src, np.int32, "src", (None, None), dev), int(src.shape[0]), int(src.shape[1]),
            None if src_row is None else _addr(src_row, np.int32, "src_row", (d["F"],), dev), int(n_mappoints)]
    _call("orbtf_apply_matches", dev, args, stream, device)


def pose_edges(frames: dict, map: dict, inv_sigma2_table, out: dict = None, stream=None, device: int = 0) -> dict:
    """The gather of src/Optimizer.cc:355-411: returns the arrays of a PoseOptimization batch (EDGE_KEYS: edge_begin,
    pose_R, pose_t, cam, xw, obs, inv_sigma2 with F * kp_cap edge rows) plus edge_kp, and zeroes frame_outlier at the
    keypoints that became edges.  inv_sigma2_table: float32 (n_levels,), beside the other arrays."""
    d = _dims(frames, map)
    dev = _is_device(frames["frame_mappoint"])
    out = _new(EDGE_KEYS, d, frames["frame_mappoint"], out)
    e = _fill(OrbtfEdges, (), EDGE_KEYS, out, d, dev, need=EDGE_KEYS)
    fs, ms = _frames(frames, d, dev), _map(map, d, dev)
    args = [C.byref(fs), C.byref(ms), _addr(inv_sigma2_table, np.float32, "inv_sigma2_table", (None,), dev),
            int(inv_sigma2_table.shape[0]), C.byref(e)]
    _call("orbtf_pose_edges", dev, args, stream, device)
    return out


def finish_pose(frames: dict, map: dict, mode: int, edges: dict, result: dict, localization: bool = False, stereo: bool = False,
                out: dict = None, stream=None, device: int = 0) -> dict:
    """Takes PoseOptimization's result (pose_R, pose_t, outlier per edge) back into the frames: frame_outlier, the pose
    narrowed to float, then DISCARD (DiscardOutliers, src/Tracking.cc:187-211) or LOCAL_MAP (:664-680, mp_found updated).
    Returns n_inliers, and for DISCARD discarded / n_discarded."""
    d = _dims(frames, map)
    dev = _is_device(frames["frame_mappoint"])
    out = _new(FINISH_KEYS, d, frames["frame_mappoint"], out)
    e = _fill(OrbtfEdges, (), EDGE_KEYS, {k: edges.get(k) for k in ("edge_begin", "edge_kp")}, d, dev, need=("edge_begin", "edge_kp"))
    r = _fill(PoseResult, (), RESULT_KEYS, {k: result.get(k) for k in ("pose_R", "pose_t", "outlier")}, d, dev,
              need=("pose_R", "pose_t", "outlier"))
    if int(result["outlier"].shape[0]) < (d["E"] if dev else int(edges["edge_begin"][-1])):
        raise ValueError("result['outlier'] is shorter than the edges")
    fs, ms = _frames(frames, d, dev), _map(map, d, dev)
    o = {k: _addr(out[k], dt, k, _shape(sp, d), dev) for k, (dt, sp) in FINISH_KEYS.items()}
    args = [C.byref(fs), C.byref(ms), int(mode), C.byref(e), C.byref(r), int(bool(localization)), int(bool(stereo)),
            o["n_inliers"], o["discarded"], o["n_discarded"]]
    _call("orbtf_finish_pose", dev, args, stream, device)
    return out


def motion_project(cur: dict, last: dict, map: dict, velocity, baseline, monocular: bool, out: dict = None, stream=None,
                   device: int = 0) -> dict:
    """TrackWithMotionModel's setup: GetReplaced on the last frames' map points, cur["pose"] = velocity * last["pose"], the
    current frames' map points cleared, and the last frames' points projected: returns MOTION_KEYS, the arrays
    motion_batch joins with the current frames' keypoint arrays.  velocity (F, 12) and baseline (F,) float32."""
    d = _dims(cur, map)
    dl = _dims(last, map)
    dev = _is_device(cur["frame_mappoint"])
    d["last_cap"] = dl["kp_cap"]
    out = _new(MOTION_KEYS, d, cur["frame_mappoint"], out)
    o = _fill(OrbtfMotion, (), MOTION_KEYS, out, d, dev, need=MOTION_KEYS)
    fc, fl, ms = _frames(cur, d, dev), _frames(last, dl, dev), _map(map, d, dev)
    args = [C.byref(fc), C.byref(fl), C.byref(ms), _addr(velocity, np.float32, "velocity", (d["F"], 12), dev),
            _addr(baseline, np.float32, "baseline", (d["F"],), dev), int(bool(monocular)), C.byref(o)]
    _call("orbtf_motion_project", dev, args, stream, device)
    return out


def motion_batch(projected: dict, cur: dict, scale_factors, th: float, check_orientation: bool = True) -> dict:
    """The dict search_by_projection_motion_device takes, from motion_project's result and the current frames' keypoint
    arrays.  Only views are taken: nothing is copied or read back."""
    F, cap = projected["kp_claimed"].shape
    b = {"scale_factors": np.ascontiguousarray(scale_factors, np.float32), "th": float(th),
         "check_orientation": bool(check_orientation), "bounds": cur["bounds"]}
    for k, w in (("kp_xy", 2), ("kp_octave", 1), ("kp_uright", 1), ("kp_desc", 32), ("kp_angle", 1)):
        b[k] = cur[k].reshape(F * cap, w) if w > 1 else cur[k].reshape(F * cap)
    for k in ("kp_begin", "mp_begin", "motion"):
        b[k] = projected[k]
    b["kp_claimed"] = projected["kp_claimed"].reshape(-1)
    for k, w in (("mp_valid", 1), ("mp_proj", 3), ("mp_octave", 1), ("mp_desc", 32), ("mp_has_obs", 1), ("mp_angle", 1)):
        b[k] = projected[k].reshape(-1, w) if w > 1 else projected[k].reshape(-1)
    return b


def end_frame(frames: dict, map: dict, th_depth: float, reference_kf, min_obs, out: dict = None, stream=None,
              device: int = 0) -> dict:
    """The end of Update (src/Tracking.cc:1259-1281) and NeedNewKeyFrame's counts (:490-511): returns n_observations
    (F, kp_cap) and counts (F, 3) = (close and tracked, close and not tracked, TrackedMapPoints(min_obs[f]) of
    reference_kf[f]); map points without observations are removed from the frames.  Without kp_depth (monocular) the
    first two counts are 0."""
    d = _dims(frames, map)
    dev = _is_device(frames["frame_mappoint"])
    out = _new(END_KEYS, d, frames["frame_mappoint"], out)
    fs, ms = _frames(frames, d, dev), _map(map, d, dev)
    o = {k: _addr(out[k], dt, k, _shape(sp, d), dev) for k, (dt, sp) in END_KEYS.items()}
    args = [C.byref(fs), C.byref(ms), float(th_depth), _addr(reference_kf, np.int32, "reference_kf", (d["F"],), dev),
            _addr(min_obs, np.int32, "min_obs", (d["F"],), dev), o["n_observations"], o["counts"]]
    _call("orbtf_end_frame", dev, args, stream, device)
    return out


def drop_outliers(frames: dict, stream=None, device: int = 0) -> None:
    """src/Tracking.cc:1309-1313: a keypoint flagged as an outlier loses its map point."""
    d = _dims(frames)
    dev = _is_device(frames["frame_mappoint"])
    fs = _frames(frames, d, dev)
    _call("orbtf_drop_outliers", dev, [C.byref(fs)], stream, device)


def stereo_points(frames: dict, map: dict, mode: int, th_depth: float, out: dict = None, stream=None, device: int = 0) -> dict:
    """The stereo / RGB-D point creation of CreateMapPoints (KEYFRAME), CreateMapPointsVO (VO) and StereoInitialization
    (INIT): returns created_kp (F, kp_cap) in creation order, created_xw (F, kp_cap, 3), n_created and n_processed; the
    caller allocates the slots.  KEYFRAME clears the map points without observations it replaces."""
    d = _dims(frames, map)
    dev = _is_device(frames["frame_mappoint"])
    out = _new(CREATED_KEYS, d, frames["frame_mappoint"], out)
    o = _fill(OrbtfCreated, (), CREATED_KEYS, out, d, dev, need=CREATED_KEYS)
    fs, ms = _frames(frames, d, dev), _map(map, d, dev)
    _call("orbtf_stereo_points", dev, [C.byref(fs), C.byref(ms), int(mode), float(th_depth), C.byref(o)], stream, device)
    return out
