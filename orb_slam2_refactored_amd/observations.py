"""The insert half of the observation graph over the gfx950 C-ABI (orbmm_add_keyframe_observations, orbmm_fuse_apply,
orbmm_grow_observations; include/orbslam2_amd.h, "Observation edits"): MapPoint::AddObservation and MapPoint::Replace
(src/MapPoint.cc:109-122, 191-230) under ProcessNewKeyFrame's loop (src/LocalMapping.cc:309-326), Fuse's apply loops
(src/ORBmatcher.cc:957-976, 1070-1084 with src/LoopClosing.cc:652-657) and CorrectLoop's matched points
(src/LoopClosing.cc:617-634).

The map is a dict of slot arrays, OBSERVE_KEYS.  A point's row of the CSR keeps free entries (mp_obs_kf = -1) for inserts;
GrowObservations makes room.  The capitalised functions take numpy arrays, are synchronous and return updated copies; the
*_device functions take CUDA tensors, update them in place and only enqueue."""
import ctypes as C

import numpy as np

from ._lib import OrbmmApply, OrbmmObserve, check, lib, ptr, stream_ptr
from .local_map import _dev, _host, _shape

OK, OBS_OVERFLOW = 0, 2
APPLY_FUSE, APPLY_FUSE_SIM3, APPLY_LOOP_MATCHED = 0, 1, 2

# name: (dtype, shape); K keyframes, M map points, None = free.  The order is orbmm_observe's.
OBSERVE_KEYS = {
    "kf_n": (np.int32, ("K",)), "kf_mappoint": (np.int32, ("K", "kf_cap")), "kf_uright": (np.float32, ("K", "kf_cap")),
    "mp_bad": (np.uint8, ("M",)), "mp_nobs": (np.int32, ("M",)), "mp_found": (np.int32, ("M",)), "mp_visible": (np.int32, ("M",)),
    "mp_replaced": (np.int32, ("M",)), "mp_obs_off": (np.int32, ("M1",)), "mp_obs_kf": (np.int32, (None,)),
    "mp_obs_idx": (np.int32, (None,)),
}
NEW_KEYFRAME_KEYS = tuple(k for k in OBSERVE_KEYS if k not in ("mp_found", "mp_visible", "mp_replaced"))
NEW_KEYFRAME_UPDATED = ("mp_nobs", "mp_obs_kf", "mp_obs_idx")
APPLY_UPDATED = ("kf_mappoint", "mp_bad", "mp_nobs", "mp_found", "mp_visible", "mp_replaced", "mp_obs_kf", "mp_obs_idx")
# name: shape; I items, E entries.  The order is orbmm_apply's.
APPLY_KEYS = {"item_kf": ("I",), "mp_begin": ("I1",), "point": ("E",), "best_idx": ("E",), "replace_point": ("E",),
              "n_fused": ("I",), "touched": ("M",), "n_touched": (1,), "progress": (4,), "status": (1,)}
APPLY_STATE = ("replace_point", "n_fused", "touched", "n_touched", "progress", "status")


def _dims(t):
    for k in ("kf_mappoint", "mp_bad", "mp_obs_kf", "mp_obs_idx"):
        if t.get(k) is None:
            raise ValueError(f"{k} is required")
    if len(t["kf_mappoint"].shape) != 2:
        raise ValueError("kf_mappoint must have two dimensions")
    if t["mp_obs_kf"].shape != t["mp_obs_idx"].shape:
        raise ValueError("mp_obs_kf and mp_obs_idx must have one length")
    M = int(t["mp_bad"].shape[0])
    return {"K": int(t["kf_mappoint"].shape[0]), "M": M, "M1": M + 1, "kf_cap": int(t["kf_mappoint"].shape[1])}


def _struct(d, addr, n_obs):
    return OrbmmObserve(d["K"], d["M"], d["kf_cap"], n_obs, *[addr.get(k) for k in OBSERVE_KEYS])


def _host_tables(tables, keys, updated):
    d = _dims(tables)
    a = {k: _host(tables.get(k), OBSERVE_KEYS[k][0], k, _shape(OBSERVE_KEYS[k][1], d)) for k in keys}
    for k in updated:
        a[k] = a[k].copy()
    spare = np.zeros(4, np.int32)                            # an empty array still needs an address
    return d, a, {k: (ptr(v).value if v.size else ptr(spare).value) for k, v in a.items()}, spare


def _dev_tables(tables, keys):
    import torch
    d = _dims(tables)
    a = {k: _dev(tables.get(k), OBSERVE_KEYS[k][0], k, _shape(OBSERVE_KEYS[k][1], d)) for k in keys}
    spare = torch.zeros(4, dtype=torch.int32, device=a["mp_bad"].device)
    return d, a, {k: (v.data_ptr() if v.numel() else spare.data_ptr()) for k, v in a.items()}, spare


def AddKeyFrameObservations(tables: dict, cur: int, device: int = 0):
    """ProcessNewKeyFrame's loop for keyframe slot `cur` on `tables` (NEW_KEYFRAME_KEYS of OBSERVE_KEYS, numpy).  Returns (the
    updated copies of NEW_KEYFRAME_UPDATED, added, recent, status): the points that gained the observation, the points that
    had it (for recentAddedMapPoints_), both in keypoint order, and ORBMM_* per keypoint (OBS_OVERFLOW: that point's row is
    full)."""
    d, a, addr, spare = _host_tables(tables, NEW_KEYFRAME_KEYS, NEW_KEYFRAME_UPDATED)
    cap = d["kf_cap"]
    added, recent, counts, status = (np.full(cap, -1, np.int32), np.full(cap, -1, np.int32), np.zeros(2, np.int32),
                                     np.zeros(cap, np.int32))
    o = _struct(d, addr, len(a["mp_obs_kf"]))
    check(lib().orbmm_add_keyframe_observations(C.byref(o), int(cur), ptr(added), ptr(recent), ptr(counts), ptr(status), device),
          "orbmm_add_keyframe_observations")
    return {k: a[k] for k in NEW_KEYFRAME_UPDATED}, added[:int(counts[0])], recent[:int(counts[1])], status


def add_keyframe_observations_device(tables: dict, cur: int, out=None, stream=None):
    """Device form: NEW_KEYFRAME_KEYS contiguous CUDA tensors, NEW_KEYFRAME_UPDATED updated in place.  Returns (added, recent,
    counts, status): int32 tensors of kf_cap, kf_cap, 2 and kf_cap entries (`out` to reuse them); the lists are -1 padded.
    Enqueue only on `stream`."""
    import torch
    d, a, addr, spare = _dev_tables(tables, NEW_KEYFRAME_KEYS)
    cap, dev = d["kf_cap"], a["mp_bad"].device
    new = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    added, recent, counts, status = out if out is not None else (new(cap), new(cap), new(2), new(cap))
    for t, name, n in ((added, "added", cap), (recent, "recent", cap), (counts, "counts", 2), (status, "status", cap)):
        _dev(t, np.int32, name, (n,))
    o = _struct(d, addr, int(a["mp_obs_kf"].shape[0]))
    check(lib().orbmm_add_keyframe_observations_device(C.byref(o), int(cur), added.data_ptr(), recent.data_ptr(), counts.data_ptr(),
                                                       status.data_ptr(), stream_ptr(stream)), "orbmm_add_keyframe_observations_device")
    return added, recent, counts, status


def _apply_dims(d, item_kf, point):
    I, E = int(item_kf.shape[0]), int(point.shape[0])
    return dict(d, I=I, I1=I + 1, E=E)


def FuseApply(tables: dict, mode: int, item_kf, mp_begin, point, best_idx, state: dict = None, device: int = 0):
    """The apply loop of `mode` (APPLY_*) on `tables` (OBSERVE_KEYS, numpy) over the list (item_kf, mp_begin, point,
    best_idx) as orbm's Fuse leaves it.  state: APPLY_STATE of an interrupted walk, to resume it after GrowObservations.
    Returns (the updated copies of APPLY_UPDATED, state): state["status"][0] is OK or OBS_OVERFLOW, state["progress"] =
    (item, phase, entry, the point whose row was full), state["touched"][:state["n_touched"][0]] the points whose descriptor
    and normal are to be recomputed (the rest of touched is -1), state["n_fused"] per item."""
    d, a, addr, spare = _host_tables(tables, tuple(OBSERVE_KEYS), APPLY_UPDATED)
    lst = dict(item_kf=np.ascontiguousarray(item_kf), mp_begin=np.ascontiguousarray(mp_begin), point=np.ascontiguousarray(point),
               best_idx=np.ascontiguousarray(best_idx))
    d = _apply_dims(d, lst["item_kf"], lst["point"])
    fresh = dict(replace_point=np.full(d["E"], -1, np.int32), n_fused=np.zeros(d["I"], np.int32), touched=np.zeros(d["M"], np.int32),
                 n_touched=np.zeros(1, np.int32), progress=np.zeros(4, np.int32), status=np.zeros(1, np.int32))
    lst.update({k: np.array((state or fresh)[k], copy=True) for k in APPLY_STATE})
    lst = {k: _host(lst[k], np.int32, k, _shape(APPLY_KEYS[k], d)) for k in APPLY_KEYS}
    ap = OrbmmApply(int(mode), d["I"], d["E"], *[(ptr(lst[k]).value if lst[k].size else ptr(spare).value) for k in APPLY_KEYS])
    check(lib().orbmm_fuse_apply(C.byref(_struct(d, addr, len(a["mp_obs_kf"]))), C.byref(ap), device), "orbmm_fuse_apply")
    return {k: a[k] for k in APPLY_UPDATED}, {k: lst[k] for k in APPLY_STATE}


def fuse_apply_device(tables: dict, mode: int, item_kf, mp_begin, point, best_idx, state: dict = None, stream=None):
    """Device form: OBSERVE_KEYS and the list as contiguous CUDA tensors, APPLY_UPDATED updated in place; best_idx is what
    fuse_device returned.  state: APPLY_STATE tensors of an interrupted walk (or to reuse: progress zero, replace_point -1).
    Returns state.  Enqueue only on `stream`: read state["status"] when convenient."""
    import torch
    d, a, addr, spare = _dev_tables(tables, tuple(OBSERVE_KEYS))
    dev = a["mp_bad"].device
    lst = dict(item_kf=item_kf, mp_begin=mp_begin, point=point, best_idx=best_idx)
    for k in lst:
        _dev(lst[k], np.int32, k, (None,))
    d = _apply_dims(d, item_kf, point)
    if state is None:
        new = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=dev)  # noqa: E731
        state = dict(replace_point=new(d["E"], -1), n_fused=new(d["I"]), touched=new(d["M"]), n_touched=new(1), progress=new(4),
                     status=new(1))
    lst.update({k: state[k] for k in APPLY_STATE})
    for k in APPLY_KEYS:
        _dev(lst[k], np.int32, k, _shape(APPLY_KEYS[k], d))
    ap = OrbmmApply(int(mode), d["I"], d["E"], *[(lst[k].data_ptr() if lst[k].numel() else spare.data_ptr()) for k in APPLY_KEYS])
    check(lib().orbmm_fuse_apply_device(C.byref(_struct(d, addr, int(a["mp_obs_kf"].shape[0]))), C.byref(ap), stream_ptr(stream)),
          "orbmm_fuse_apply_device")
    return {k: lst[k] for k in APPLY_STATE}


def GrowObservations(mp_obs_off, mp_obs_kf, mp_obs_idx, slack: int = 0, extra=None, n_obs_out: int = None, device: int = 0):
    """(mp_obs_off, mp_obs_kf, mp_obs_idx, status): every row its live entries (not -1) in order followed by `slack` free
    entries, or extra[p] where `extra` is given.  n_obs_out: the capacity of the new arrays (default: what is needed)."""
    off = _host(mp_obs_off, np.int32, "mp_obs_off", (None,))
    kf = _host(mp_obs_kf, np.int32, "mp_obs_kf", (None,))
    idx = _host(mp_obs_idx, np.int32, "mp_obs_idx", (len(kf),))
    if len(off) < 1:
        raise ValueError("mp_obs_off must have at least one entry")
    M, n = len(off) - 1, len(kf)
    ex = None if extra is None else _host(extra, np.int32, "extra", (M,))
    if n_obs_out is None:
        n_obs_out = n + (int(np.maximum(ex, 0).sum()) if ex is not None else int(slack) * M)
    o_off, o_kf, o_idx, status = (np.zeros(M + 1, np.int32), np.zeros(max(n_obs_out, 1), np.int32), np.zeros(max(n_obs_out, 1), np.int32),
                                  np.zeros(1, np.int32))
    check(lib().orbmm_grow_observations(M, n, ptr(off), ptr(kf) if n else ptr(o_kf), ptr(idx) if n else ptr(o_idx), int(slack),
                                        ptr(ex) if ex is not None and M else None, int(n_obs_out), ptr(o_off), ptr(o_kf), ptr(o_idx),
                                        ptr(status), device), "orbmm_grow_observations")
    end = min(int(o_off[-1]), n_obs_out)
    return o_off, o_kf[:end], o_idx[:end], int(status[0])


def grow_observations_device(mp_obs_off, mp_obs_kf, mp_obs_idx, n_obs_out: int, slack: int = 0, extra=None, out=None, stream=None):
    """Device form.  Returns (mp_obs_off, mp_obs_kf, mp_obs_idx, status) as new tensors of M + 1, n_obs_out, n_obs_out and 1
    entries (`out` to reuse four); the lists end at mp_obs_off[M]."""
    import torch
    off = _dev(mp_obs_off, np.int32, "mp_obs_off", (None,))
    kf = _dev(mp_obs_kf, np.int32, "mp_obs_kf", (None,))
    idx = _dev(mp_obs_idx, np.int32, "mp_obs_idx", (int(kf.shape[0]),))
    if int(off.shape[0]) < 1:
        raise ValueError("mp_obs_off must have at least one entry")
    M, n = int(off.shape[0]) - 1, int(kf.shape[0])
    ex = None if extra is None else _dev(extra, np.int32, "extra", (M,))
    new = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=off.device)  # noqa: E731
    o_off, o_kf, o_idx, status = out if out is not None else (new(M + 1), new(n_obs_out), new(n_obs_out), new(1))
    _dev(o_off, np.int32, "out mp_obs_off", (M + 1,))
    _dev(o_kf, np.int32, "out mp_obs_kf", (max(n_obs_out, 1),))
    _dev(o_idx, np.int32, "out mp_obs_idx", (max(n_obs_out, 1),))
    _dev(status, np.int32, "status", (1,))
    if n and (o_kf.data_ptr() == kf.data_ptr() or o_idx.data_ptr() == idx.data_ptr()):
        raise ValueError("the outputs must be distinct from the inputs")
    check(lib().orbmm_grow_observations_device(M, n, off.data_ptr(), kf.data_ptr() if n else o_kf.data_ptr(),
                                               idx.data_ptr() if n else o_idx.data_ptr(), int(slack),
                                               ex.data_ptr() if ex is not None and M else None, int(n_obs_out), o_off.data_ptr(),
                                               o_kf.data_ptr(), o_idx.data_ptr(), status.data_ptr(), stream_ptr(stream)),
          "orbmm_grow_observations_device")
    return o_off, o_kf, o_idx, status
