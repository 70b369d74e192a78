"""Tracking's local map (src/Tracking.cc: LocalMap::Update :59-179, SearchLocalPoints up to the matcher call :607-642 with
IsInFrustum :554-605) over the gfx950 C-ABI (orbtl_*, include/orbslam2_amd.h), batched over frames.

The map is slot tables (MAP_KEYS), a batch of frames is FRAME_KEYS plus the scalars n_levels, log_scale_factor and
min_view_cos.  TrackLocalMap takes numpy arrays and is synchronous; track_local_map_device takes CUDA tensors and only
enqueues.  Both update mp_visible, frame_mappoint, local_kf and n_local_kf (the host form in copies it returns, the device
form in place) and return the arrays of an orbm_proj_batch, which projection_batch joins with the frames' keypoint arrays
into the dict search_by_projection_device takes."""
import ctypes as C

import numpy as np

from ._lib import OrbtlFrames, OrbtlMap, OrbtlResult, check, lib, ptr, stream_ptr

COVIS = 10
OK, KF_OVERFLOW, MP_OVERFLOW = 0, 1, 2

# name: (dtype, shape); K keyframes, M map points, F frames, None = free
MAP_KEYS = {
    "kf_bad": (np.uint8, ("K",)), "kf_covis": (np.int32, ("K", COVIS)), "kf_parent": (np.int32, ("K",)),
    "kf_child_off": (np.int32, ("K1",)), "kf_child_idx": (np.int32, (None,)), "kf_n": (np.int32, ("K",)),
    "kf_mappoint": (np.int32, ("K", "kf_cap")), "mp_bad": (np.uint8, ("M",)), "mp_xw": (np.float32, ("M", 3)),
    "mp_normal": (np.float32, ("M", 3)), "mp_max_min": (np.float32, ("M", 2)), "mp_desc": (np.uint8, ("M", 32)),
    "mp_nobs": (np.int32, ("M",)), "mp_obs_off": (np.int32, ("M1",)), "mp_obs_kf": (np.int32, (None,)),
    "mp_visible": (np.int32, ("M",)),
}
FRAME_KEYS = {
    "frame_n": (np.int32, ("F",)), "frame_mappoint": (np.int32, ("F", "kp_cap")), "pose": (np.float32, ("F", 12)),
    "camera": (np.float32, ("F", 5)), "bounds": (np.float32, ("F", 4)), "local_kf": (np.int32, ("F", "kf_list_cap")),
    "n_local_kf": (np.int32, ("F",)),
}
OUT_KEYS = {
    "reference_kf": (np.int32, ("F",)), "local_mp": (np.int32, ("F", "mp_cap")), "n_local_mp": (np.int32, ("F",)),
    "n_to_match": (np.int32, ("F",)), "status": (np.int32, ("F",)), "kp_begin": (np.int32, ("F1",)),
    "mp_begin": (np.int32, ("F1",)), "kp_claimed": (np.uint8, ("F", "kp_cap")), "mp_valid": (np.uint8, ("F", "mp_cap")),
    "mp_proj": (np.float32, ("F", "mp_cap", 3)), "mp_view_cos": (np.float32, ("F", "mp_cap")),
    "mp_level": (np.int32, ("F", "mp_cap")), "mp_desc": (np.uint8, ("F", "mp_cap", 32)),
    "mp_has_obs": (np.uint8, ("F", "mp_cap")), "votes": (np.int32, ("F", "K")),
}
UPDATED = ("mp_visible", "frame_mappoint", "local_kf", "n_local_kf")


def _dims(m, fr, mp_cap):
    for k in ("kf_bad", "kf_mappoint", "mp_bad"):
        if m.get(k) is None:
            raise ValueError(f"{k} is required")
    for k in ("frame_n", "frame_mappoint", "local_kf"):
        if fr.get(k) is None:
            raise ValueError(f"{k} is required")
    if len(m["kf_mappoint"].shape) != 2 or len(fr["frame_mappoint"].shape) != 2 or len(fr["local_kf"].shape) != 2:
        raise ValueError("kf_mappoint, frame_mappoint and local_kf must have two dimensions")
    K, M, F = int(m["kf_bad"].shape[0]), int(m["mp_bad"].shape[0]), int(fr["frame_n"].shape[0])
    d = {"K": K, "K1": K + 1, "M": M, "M1": M + 1, "F": F, "F1": F + 1, "kf_cap": int(m["kf_mappoint"].shape[1]),
         "kp_cap": int(fr["frame_mappoint"].shape[1]), "kf_list_cap": int(fr["local_kf"].shape[1]), "mp_cap": int(mp_cap)}
    if d["mp_cap"] < 1:
        raise ValueError("mp_cap must be at least 1")
    return d


def _shape(spec, d):
    return tuple(d[s] if isinstance(s, str) else s for s in spec)


def _fits(shape, want):
    return len(shape) == len(want) and all(w is None or w == s for s, w in zip(shape, want))


def _host(a, dtype, name, want):
    if a is None:
        raise ValueError(f"{name} is required")
    a = np.ascontiguousarray(a)
    if a.dtype != dtype:
        raise ValueError(f"{name} must be {np.dtype(dtype).name}, not {a.dtype.name}")
    if not _fits(a.shape, want):
        raise ValueError(f"{name} must have shape {want}, not {a.shape}")
    return a


def _dev(t, dtype, name, want):
    import torch
    tt = {np.int32: torch.int32, np.uint8: torch.uint8, np.float32: torch.float32}[dtype]
    if t is None:
        raise ValueError(f"{name} is required")
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor")
    if t.dtype != tt or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {tt} tensor")
    if not _fits(tuple(t.shape), want):
        raise ValueError(f"{name} must have shape {want}, not {tuple(t.shape)}")
    return t


def _structs(d, fr, addr, out_addr):
    """addr: the map's and the frames' arrays; out_addr: the outputs' (mp_desc is a name of both)."""
    m = OrbtlMap(d["K"], d["M"], d["kf_cap"], *[addr[k] for k in MAP_KEYS])
    f = OrbtlFrames(d["F"], d["kp_cap"], d["kf_list_cap"], d["mp_cap"], int(fr["n_levels"]), float(fr["log_scale_factor"]),
                    float(fr.get("min_view_cos", 0.5)), *[addr[k] for k in FRAME_KEYS])
    r = OrbtlResult(*[out_addr.get(k) for k in OUT_KEYS])
    return m, f, r


class LocalMap:
    """The map's slot tables (a dict with MAP_KEYS; numpy arrays for TrackLocalMap, CUDA tensors for
    track_local_map_device)."""

    def __init__(self, tables: dict):
        self.tables = tables

    def TrackLocalMap(self, frames: dict, mp_cap: int, votes: bool = True, device: int = 0) -> dict:
        """LocalMap::Update and SearchLocalPoints' frustum pass for the frames of `frames` (FRAME_KEYS, n_levels,
        log_scale_factor, min_view_cos = 0.5).  Returns OUT_KEYS plus the updated copies of mp_visible, frame_mappoint,
        local_kf and n_local_kf; self.tables["mp_visible"] is replaced by the updated copy."""
        d = _dims(self.tables, frames, mp_cap)
        a = {k: _host(self.tables.get(k), dt, k, _shape(sp, d)) for k, (dt, sp) in MAP_KEYS.items()}
        a.update({k: _host(frames.get(k), dt, k, _shape(sp, d)) for k, (dt, sp) in FRAME_KEYS.items()})
        for k in UPDATED:
            a[k] = a[k].copy()
        for k in ("kf_child_idx", "mp_obs_kf"):
            if a[k].size == 0:
                a[k] = np.zeros(1, np.int32)   # an empty list still needs an address
        if int(a["kf_child_off"][-1]) > len(a["kf_child_idx"]) or int(a["mp_obs_off"][-1]) > len(a["mp_obs_kf"]):
            raise ValueError("kf_child_idx / mp_obs_kf is shorter than its offsets say")
        out = {k: np.zeros(_shape(sp, d), dt) for k, (dt, sp) in OUT_KEYS.items() if k != "votes" or votes}
        m, f, r = _structs(d, frames, {k: ptr(v).value for k, v in a.items()}, {k: ptr(v).value for k, v in out.items()})
        check(lib().orbtl_track_local_map(C.byref(m), C.byref(f), C.byref(r), device), "orbtl_track_local_map")
        out.update({k: a[k] for k in UPDATED})
        self.tables["mp_visible"] = a["mp_visible"]
        return out

    def track_local_map_device(self, frames: dict, mp_cap: int, votes: bool = False, out: dict = None, stream=None) -> dict:
        """Device form: every array a contiguous CUDA tensor; mp_visible, frame_mappoint, local_kf and n_local_kf are
        updated in place.  Enqueue only on `stream`; returns the dict of output tensors (`out` to reuse one)."""
        import torch
        d = _dims(self.tables, frames, mp_cap)
        a = {k: _dev(self.tables.get(k), dt, k, _shape(sp, d)) for k, (dt, sp) in MAP_KEYS.items()}
        a.update({k: _dev(frames.get(k), dt, k, _shape(sp, d)) for k, (dt, sp) in FRAME_KEYS.items()})
        dev = a["kf_bad"].device
        tt = {np.int32: torch.int32, np.uint8: torch.uint8, np.float32: torch.float32}
        if out is None:
            out = {k: torch.empty(_shape(sp, d), dtype=tt[dt], device=dev) for k, (dt, sp) in OUT_KEYS.items()
                   if k != "votes" or votes}
        for k, (dt, sp) in OUT_KEYS.items():
            if k != "votes" or votes:
                _dev(out.get(k), dt, k, _shape(sp, d))
        spare = torch.zeros(4, dtype=torch.int32, device=dev)   # an empty list still needs an address
        addr = lambda t: {k: (v.data_ptr() if v.numel() else spare.data_ptr()) for k, v in t.items()}  # noqa: E731
        m, f, r = _structs(d, frames, addr(a), addr({k: v for k, v in out.items() if k in OUT_KEYS and (k != "votes" or votes)}))
        check(lib().orbtl_track_local_map_device(C.byref(m), C.byref(f), C.byref(r), stream_ptr(stream)),
              "orbtl_track_local_map_device")
        return out

    @staticmethod
    def projection_batch(result: dict, keypoints: dict, scale_factors, th: float = 1.0, nnratio: float = 0.8) -> dict:
        """The dict SearchByProjection / search_by_projection_device take, from a TrackLocalMap result and the frames'
        keypoint arrays of stride kp_cap: kp_xy (F, kp_cap, 2), kp_octave (F, kp_cap), kp_uright (F, kp_cap), kp_desc
        (F, kp_cap, 32), bounds (F, 4).  Only views are taken: nothing is copied or read back.  Rows from frame_n[f] on are
        padding (claimed, so never matched); their kp_xy must be finite."""
        F, kp_cap = result["kp_claimed"].shape
        b = {"kp_begin": result["kp_begin"], "mp_begin": result["mp_begin"], "bounds": keypoints["bounds"],
             "scale_factors": np.ascontiguousarray(scale_factors, np.float32), "th": float(th), "nnratio": float(nnratio)}
        for k, w in (("kp_xy", 2), ("kp_octave", 1), ("kp_uright", 1), ("kp_desc", 32)):
            v = keypoints[k]
            if tuple(v.shape[:2]) != (F, kp_cap):
                raise ValueError(f"{k} must have shape ({F}, {kp_cap}, ...), not {tuple(v.shape)}")
            b[k] = v.reshape(F * kp_cap, w) if w > 1 else v.reshape(F * kp_cap)
        b["kp_claimed"] = result["kp_claimed"].reshape(-1)
        for k, w in (("mp_valid", 1), ("mp_proj", 3), ("mp_view_cos", 1), ("mp_level", 1), ("mp_desc", 32), ("mp_has_obs", 1)):
            b[k] = result[k].reshape(-1, w) if w > 1 else result[k].reshape(-1)
        return b
