"""LocalMapping's culls over the gfx950 C-ABI (orbmm_cull_*, include/orbslam2_amd.h): MapPointCulling and KeyFrameCulling
(src/LocalMapping.cc:335-369, 641-701) with MapPoint::SetBadFlag / EraseObservation and KeyFrame::SetBadFlag /
EraseConnection behind them, the observation CSR without erased entries, and the children of live keyframes.

The map is a dict of slot arrays, CULL_KEYS.  An erased observation is a -1 in mp_obs_kf until the CSR is compacted.  The
capitalised functions take numpy arrays, are synchronous and return updated copies (with the observation CSR compacted, so
that the result can go into any host entry); the *_device functions take CUDA tensors, update them in place and only
enqueue."""
import ctypes as C

import numpy as np

from ._lib import OrbmmCull, check, lib, ptr, stream_ptr
from .local_map import COVIS, _dev, _host, _shape

OK = 0

# name: (dtype, shape); K keyframes, M map points, None = free.  The order is orbmm_cull's.
CULL_KEYS = {
    "kf_id": (np.int32, ("K",)), "kf_n": (np.int32, ("K",)), "kf_mappoint": (np.int32, ("K", "kf_cap")),
    "kf_kp_octave": (np.int32, ("K", "kf_cap")), "kf_uright": (np.float32, ("K", "kf_cap")),
    "kf_depth": (np.float32, ("K", "kf_cap")), "kf_pose": (np.float32, ("K", 12)), "kf_bad": (np.uint8, ("K",)),
    "kf_not_erase": (np.uint8, ("K",)), "kf_to_be_erased": (np.uint8, ("K",)), "kf_tcp": (np.float32, ("K", 12)),
    "mp_bad": (np.uint8, ("M",)), "mp_nobs": (np.int32, ("M",)), "mp_found": (np.int32, ("M",)),
    "mp_visible": (np.int32, ("M",)), "mp_first_kf_id": (np.int32, ("M",)), "mp_ref_kf": (np.int32, ("M",)),
    "mp_obs_off": (np.int32, ("M1",)), "mp_obs_kf": (np.int32, (None,)), "mp_obs_idx": (np.int32, (None,)),
    "conn_slot": (np.int32, ("K", "conn_cap")), "conn_weight": (np.int32, ("K", "conn_cap")), "n_conn": (np.int32, ("K",)),
    "ord_slot": (np.int32, ("K", "conn_cap")), "ord_weight": (np.int32, ("K", "conn_cap")), "n_ord": (np.int32, ("K",)),
    "kf_parent": (np.int32, ("K",)), "kf_covis": (np.int32, ("K", COVIS)),
}
POINT_KEYS = ("kf_mappoint", "mp_bad", "mp_nobs", "mp_found", "mp_visible", "mp_first_kf_id", "mp_obs_off", "mp_obs_kf",
              "mp_obs_idx")                                  # what MapPointCulling takes
POINT_UPDATED = ("mp_bad", "kf_mappoint", "mp_obs_kf")
KEYFRAME_UPDATED = ("kf_bad", "kf_to_be_erased", "kf_tcp", "kf_mappoint", "mp_bad", "mp_nobs", "mp_ref_kf", "mp_obs_kf",
                    "conn_slot", "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord", "kf_parent", "kf_covis")


def _dims(t, keys):
    for k in ("kf_mappoint", "mp_bad", "mp_obs_kf", "mp_obs_idx") + (("conn_slot",) if "conn_slot" in keys else ()):
        if t.get(k) is None:
            raise ValueError(f"{k} is required")
    if len(t["kf_mappoint"].shape) != 2:
        raise ValueError("kf_mappoint must have two dimensions")
    if t["mp_obs_kf"].shape != t["mp_obs_idx"].shape:
        raise ValueError("mp_obs_kf and mp_obs_idx must have one length")
    M = int(t["mp_bad"].shape[0])
    d = {"K": int(t["kf_mappoint"].shape[0]), "M": M, "M1": M + 1, "kf_cap": int(t["kf_mappoint"].shape[1]), "conn_cap": 0}
    if "conn_slot" in keys:
        if len(t["conn_slot"].shape) != 2:
            raise ValueError("conn_slot must have two dimensions")
        d["conn_cap"] = int(t["conn_slot"].shape[1])
    return d


def _struct(d, addr, n_obs):
    return OrbmmCull(d["K"], d["M"], d["kf_cap"], d["conn_cap"], n_obs, *[addr.get(k) for k in CULL_KEYS])


def _host_tables(tables, keys, updated):
    d = _dims(tables, keys)
    a = {k: _host(tables.get(k), CULL_KEYS[k][0], k, _shape(CULL_KEYS[k][1], d)) for k in keys}
    for k in updated:
        a[k] = a[k].copy()
    spare = np.zeros(4, np.int32)                            # an empty array still needs an address
    return d, a, {k: (ptr(v).value if v.size else ptr(spare).value) for k, v in a.items()}, spare


def _dev_tables(tables, keys):
    import torch
    d = _dims(tables, keys)
    a = {k: _dev(tables.get(k), CULL_KEYS[k][0], k, _shape(CULL_KEYS[k][1], d)) for k in keys}
    spare = torch.zeros(4, dtype=torch.int32, device=a["mp_bad"].device)
    return d, a, {k: (v.data_ptr() if v.numel() else spare.data_ptr()) for k, v in a.items()}, spare


def _compacted(out, a, device):
    out["mp_obs_off"], out["mp_obs_kf"], out["mp_obs_idx"] = CompactObservations(a["mp_obs_off"], a["mp_obs_kf"], a["mp_obs_idx"],
                                                                                 device)
    return out


def MapPointCulling(tables: dict, recent, cur_kf_id: int, monocular: bool, compact: bool = True, device: int = 0):
    """MapPointCulling on `tables` (POINT_KEYS of CULL_KEYS, numpy) for the point slots `recent`.  Returns (the updated
    copies of POINT_UPDATED, the list that is left).  compact: mp_obs_off / mp_obs_kf / mp_obs_idx without the erased
    entries are returned too; otherwise mp_obs_kf holds -1 where an observation was erased."""
    d, a, addr, spare = _host_tables(tables, POINT_KEYS, POINT_UPDATED)
    rec = np.array(recent, np.int32).reshape(-1)
    n = np.zeros(1, np.int32)
    c = _struct(d, addr, len(a["mp_obs_kf"]))
    check(lib().orbmm_cull_map_points(C.byref(c), len(rec), ptr(rec) if rec.size else ptr(spare), int(cur_kf_id),
                                      1 if monocular else 0, ptr(n), device), "orbmm_cull_map_points")
    out = {k: a[k] for k in POINT_UPDATED}
    return (_compacted(out, a, device) if compact else out), rec[:int(n[0])]


def map_point_culling_device(tables: dict, recent, cur_kf_id: int, monocular: bool, n_out=None, stream=None):
    """Device form: POINT_KEYS contiguous CUDA tensors, POINT_UPDATED and `recent` (int32 point slots) updated in place.
    Returns the int32 tensor of one entry holding the length of the list that is left (`n_out` to reuse one).  Enqueue
    only on `stream`."""
    import torch
    d, a, addr, spare = _dev_tables(tables, POINT_KEYS)
    recent = _dev(recent, np.int32, "recent", (None,))
    if n_out is None:
        n_out = torch.zeros(1, dtype=torch.int32, device=recent.device)
    _dev(n_out, np.int32, "n_out", (1,))
    c = _struct(d, addr, int(a["mp_obs_kf"].shape[0]))
    check(lib().orbmm_cull_map_points_device(C.byref(c), int(recent.numel()), recent.data_ptr() if recent.numel() else spare.data_ptr(),
                                             int(cur_kf_id), 1 if monocular else 0, n_out.data_ptr(), stream_ptr(stream)),
          "orbmm_cull_map_points_device")
    return n_out


def KeyFrameCulling(tables: dict, cur: int, monocular: bool, th_depth: float, compact: bool = True, device: int = 0):
    """KeyFrameCulling(cur) on `tables` (CULL_KEYS, numpy).  Returns (the updated copies of KEYFRAME_UPDATED, the culled
    slots in order).  compact: as MapPointCulling's."""
    d, a, addr, spare = _host_tables(tables, tuple(CULL_KEYS), KEYFRAME_UPDATED)
    culled, n, status = np.full(max(d["conn_cap"], 1), -1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    c = _struct(d, addr, len(a["mp_obs_kf"]))
    check(lib().orbmm_cull_keyframes(C.byref(c), int(cur), 1 if monocular else 0, float(th_depth), ptr(culled), ptr(n), ptr(status),
                                     device), "orbmm_cull_keyframes")
    out = {k: a[k] for k in KEYFRAME_UPDATED}
    return (_compacted(out, a, device) if compact else out), culled[:int(n[0])]


def keyframe_culling_device(tables: dict, cur: int, monocular: bool, th_depth: float, out=None, stream=None):
    """Device form: CULL_KEYS contiguous CUDA tensors, KEYFRAME_UPDATED updated in place.  Returns (culled, n_culled,
    status): int32 tensors of conn_cap, 1 and 1 entries (`out` to reuse them); culled is -1 padded, as
    KeyFrameDatabase.erase_device takes it.  Enqueue only on `stream`."""
    import torch
    d, a, addr, spare = _dev_tables(tables, tuple(CULL_KEYS))
    dev = a["mp_bad"].device
    culled, n, status = out if out is not None else (torch.empty(max(d["conn_cap"], 1), dtype=torch.int32, device=dev),
                                                      torch.zeros(1, dtype=torch.int32, device=dev),
                                                      torch.zeros(1, dtype=torch.int32, device=dev))
    _dev(culled, np.int32, "culled", (max(d["conn_cap"], 1),))
    _dev(n, np.int32, "n_culled", (1,))
    _dev(status, np.int32, "status", (1,))
    c = _struct(d, addr, int(a["mp_obs_kf"].shape[0]))
    check(lib().orbmm_cull_keyframes_device(C.byref(c), int(cur), 1 if monocular else 0, float(th_depth), culled.data_ptr(),
                                            n.data_ptr(), status.data_ptr(), stream_ptr(stream)), "orbmm_cull_keyframes_device")
    return culled, n, status


def CompactObservations(mp_obs_off, mp_obs_kf, mp_obs_idx, device: int = 0):
    """(mp_obs_off, mp_obs_kf, mp_obs_idx) without the entries whose mp_obs_kf is -1, the order within a point kept."""
    off = _host(mp_obs_off, np.int32, "mp_obs_off", (None,))
    kf = _host(mp_obs_kf, np.int32, "mp_obs_kf", (None,))
    idx = _host(mp_obs_idx, np.int32, "mp_obs_idx", (len(kf),))
    if len(off) < 1:
        raise ValueError("mp_obs_off must have at least one entry")
    M, n = len(off) - 1, len(kf)
    o_off, o_kf, o_idx = np.zeros(M + 1, np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    check(lib().orbmm_compact_observations(M, n, ptr(off), ptr(kf) if n else ptr(o_kf), ptr(idx) if n else ptr(o_idx), ptr(o_off),
                                           ptr(o_kf), ptr(o_idx), device), "orbmm_compact_observations")
    end = min(int(o_off[-1]), n)
    return o_off, o_kf[:end], o_idx[:end]


def compact_observations_device(mp_obs_off, mp_obs_kf, mp_obs_idx, out=None, stream=None):
    """Device form.  Returns (mp_obs_off, mp_obs_kf, mp_obs_idx) as new tensors of the inputs' sizes (`out` to reuse three);
    the lists end at mp_obs_off[M]."""
    import torch
    off = _dev(mp_obs_off, np.int32, "mp_obs_off", (None,))
    kf = _dev(mp_obs_kf, np.int32, "mp_obs_kf", (None,))
    idx = _dev(mp_obs_idx, np.int32, "mp_obs_idx", (int(kf.shape[0]),))
    if int(off.shape[0]) < 1:
        raise ValueError("mp_obs_off must have at least one entry")
    M, n = int(off.shape[0]) - 1, int(kf.shape[0])
    new = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=off.device)  # noqa: E731
    o_off, o_kf, o_idx = out if out is not None else (new(M + 1), new(n), new(n))
    _dev(o_off, np.int32, "out mp_obs_off", (M + 1,))
    _dev(o_kf, np.int32, "out mp_obs_kf", (max(n, 1),))
    _dev(o_idx, np.int32, "out mp_obs_idx", (max(n, 1),))
    if n and (o_kf.data_ptr() == kf.data_ptr() or o_idx.data_ptr() == idx.data_ptr()):
        raise ValueError("the outputs must be distinct from the inputs")
    check(lib().orbmm_compact_observations_device(M, n, off.data_ptr(), kf.data_ptr() if n else o_kf.data_ptr(),
                                                  idx.data_ptr() if n else o_idx.data_ptr(), o_off.data_ptr(), o_kf.data_ptr(),
                                                  o_idx.data_ptr(), stream_ptr(stream)), "orbmm_compact_observations_device")
    return o_off, o_kf, o_idx


def LiveChildren(kf_parent, kf_bad, device: int = 0):
    """(kf_child_off, kf_child_idx): the GetChildren() CSR with the bad keyframes left out as children, each list
    ascending."""
    par = _host(kf_parent, np.int32, "kf_parent", (None,))
    K = len(par)
    bad = _host(kf_bad, np.uint8, "kf_bad", (K,))
    off, idx = np.zeros(K + 1, np.int32), np.zeros(max(K, 1), np.int32)
    check(lib().orbmm_children_live(K, ptr(par) if K else ptr(idx), ptr(bad) if K else ptr(idx), ptr(off), ptr(idx), device),
          "orbmm_children_live")
    return off, idx[:int(off[-1])]


def live_children_device(kf_parent, kf_bad, out=None, stream=None):
    """Device form.  Returns (kf_child_off, kf_child_idx) with K + 1 and K entries; the lists end at kf_child_off[K]."""
    import torch
    par = _dev(kf_parent, np.int32, "kf_parent", (None,))
    K = int(par.shape[0])
    bad = _dev(kf_bad, np.uint8, "kf_bad", (K,))
    off, idx = out if out is not None else (torch.empty(K + 1, dtype=torch.int32, device=par.device),
                                            torch.zeros(max(K, 1), dtype=torch.int32, device=par.device))
    _dev(off, np.int32, "kf_child_off", (K + 1,))
    _dev(idx, np.int32, "kf_child_idx", (max(K, 1),))
    check(lib().orbmm_children_live_device(K, par.data_ptr() if K else idx.data_ptr(), bad.data_ptr() if K else idx.data_ptr(),
                                           off.data_ptr(), idx.data_ptr(), stream_ptr(stream)), "orbmm_children_live_device")
    return off, idx
