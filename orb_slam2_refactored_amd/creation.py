"""Where the map grows, over the gfx950 C-ABI (orbmk_insert_keyframes, orbmk_create_points; include/orbslam2_amd.h, "Map
creation"): KeyFrame::KeyFrame(const Frame&, ...) (src/KeyFrame.cc:51-64) on a batch of frames, and MapPoint::MapPoint(Xw,
referenceKF, map) (src/MapPoint.cc:44-56) with AddObservation, ComputeDistinctiveDescriptors, KeyFrame::AddMapPoint and
Map::AddMapPoint (src/Tracking.cc:724-736, :981-997, :1104-1126; src/LocalMapping.cc:562-575) on a batch of lists, with the
allocation of the map-point slots.

Tables are dicts of slot arrays: FRAME_KEYS (a frame batch of tracking.py / frame.py; kp_un and kf_keypoint are the 28-byte
records as 7 int32), KEYFRAME_KEYS, MAP_KEYS; a list batch is a dict of LIST_KEYS.  The capitalised functions take numpy
arrays, are synchronous and return updated copies; the *_device functions take CUDA tensors, update them in place and only
enqueue."""
import ctypes as C

import numpy as np

from ._lib import OrbmkCreated, OrbmkFrames, OrbmkKeyframes, OrbmkLists, OrbmkMap, check, lib, ptr, stream_ptr
from .local_map import _dev, _host, _shape

OK, OVERFLOW = 0, 1
COVIS = 10

# name: (dtype, shape); F frames, K keyframes, M map points, I items, None = free.  The orders are the structs'.
FRAME_KEYS = {
    "frame_n": (np.int32, ("F",)), "frame_mappoint": (np.int32, ("F", "kp_cap")), "kp_un": (np.int32, ("F", "kp_cap", 7)),
    "kp_octave": (np.int32, ("F", "kp_cap")), "kp_uright": (np.float32, ("F", "kp_cap")), "kp_depth": (np.float32, ("F", "kp_cap")),
    "kp_desc": (np.uint8, ("F", "kp_cap", 32)), "pose": (np.float32, ("F", 12)), "camera": (np.float32, ("F", 5)),
}
KEYFRAME_KEYS = {
    "kf_id": (np.int32, ("K",)), "kf_n": (np.int32, ("K",)), "kf_mappoint": (np.int32, ("K", "kf_cap")),
    "kf_keypoint": (np.int32, ("K", "kf_cap", 7)), "kf_kp_octave": (np.int32, ("K", "kf_cap")), "kf_uright": (np.float32, ("K", "kf_cap")),
    "kf_depth": (np.float32, ("K", "kf_cap")), "kf_desc": (np.uint8, ("K", "kf_cap", 32)), "kf_pose": (np.float32, ("K", 12)),
    "kf_camera": (np.float32, ("K", 6)), "kf_bad": (np.uint8, ("K",)), "kf_not_erase": (np.uint8, ("K",)),
    "kf_to_be_erased": (np.uint8, ("K",)), "kf_parent": (np.int32, ("K",)), "kf_first_connection": (np.uint8, ("K",)),
    "conn_slot": (np.int32, ("K", "conn_cap")), "conn_weight": (np.int32, ("K", "conn_cap")), "n_conn": (np.int32, ("K",)),
    "ord_slot": (np.int32, ("K", "conn_cap")), "ord_weight": (np.int32, ("K", "conn_cap")), "n_ord": (np.int32, ("K",)),
    "kf_covis": (np.int32, ("K", COVIS)),
}
# what a table of KEYFRAME_KEYS is copied from
KEYFRAME_SOURCE = {"kf_n": "frame_n", "kf_mappoint": "frame_mappoint", "kf_keypoint": "kp_un", "kf_kp_octave": "kp_octave",
                   "kf_uright": "kp_uright", "kf_depth": "kp_depth", "kf_desc": "kp_desc", "kf_pose": "pose", "kf_camera": "camera"}
MAP_KEYS = {
    "kf_id": (np.int32, ("K",)), "kf_n": (np.int32, ("K",)), "kf_mappoint": (np.int32, ("K", "kf_cap")),
    "kf_uright": (np.float32, ("K", "kf_cap")), "kf_bad": (np.uint8, ("K",)), "kf_desc": (np.uint8, ("K", "kf_cap", 32)),
    "mp_bad": (np.uint8, ("M",)), "mp_xw": (np.float32, ("M", 3)), "mp_normal": (np.float32, ("M", 3)),
    "mp_max_min": (np.float32, ("M", 2)), "mp_nobs": (np.int32, ("M",)), "mp_found": (np.int32, ("M",)),
    "mp_visible": (np.int32, ("M",)), "mp_replaced": (np.int32, ("M",)), "mp_first_kf_id": (np.int32, ("M",)),
    "mp_ref_kf": (np.int32, ("M",)), "mp_desc": (np.uint8, ("M", 32)), "mp_obs_off": (np.int32, ("M1",)),
    "mp_obs_kf": (np.int32, (None,)), "mp_obs_idx": (np.int32, (None,)),
}
MAP_OPTIONAL = ("kf_bad", "kf_desc", "mp_normal", "mp_max_min", "mp_desc")
MAP_UPDATED = ("kf_mappoint", "mp_bad", "mp_xw", "mp_normal", "mp_max_min", "mp_nobs", "mp_found", "mp_visible", "mp_replaced",
               "mp_first_kf_id", "mp_ref_kf", "mp_desc", "mp_obs_kf", "mp_obs_idx")
LIST_KEYS = {
    "kf1": (np.int32, ("I",)), "kf2": (np.int32, ("I",)), "n_list": (np.int32, ("I",)), "idx1": (np.int32, ("I", "list_cap")),
    "idx2": (np.int32, ("I", "list_cap")), "xw": (np.float32, ("I", "list_cap", 3)), "normal": (np.float32, ("I", "list_cap", 3)),
    "max_distance": (np.float32, ("I", "list_cap")), "min_distance": (np.float32, ("I", "list_cap")),
    "item_frame": (np.int32, ("I",)), "frame_mappoint": (np.int32, ("F", "kp_cap")),
}
LIST_REQUIRED = ("kf1", "n_list", "idx1", "xw")
OUT_KEYS = {"alloc": (1,), "status": (1,), "needed": (2,), "created": ("I", "list_cap"), "n_created": ("I",), "recent": ("R",),
            "n_recent": (1,)}


def _frame_dims(frames):
    if frames.get("frame_n") is None:
        raise ValueError("frame_n is required")
    two = next((frames[k] for k in ("frame_mappoint", "kp_octave", "kp_uright", "kp_depth", "kp_un", "kp_desc") if frames.get(k) is not None), None)
    return {"F": int(frames["frame_n"].shape[0]), "kp_cap": int(two.shape[1]) if two is not None else 1}


def _keyframe_dims(kf):
    one = next((kf[k] for k in KEYFRAME_KEYS if kf.get(k) is not None), None)
    if one is None:
        raise ValueError("no keyframe table is given")
    two = next((kf[k] for k in KEYFRAME_KEYS if kf.get(k) is not None and KEYFRAME_KEYS[k][1][1:2] == ("kf_cap",)), None)
    rows = next((kf[k] for k in ("conn_slot", "conn_weight", "ord_slot", "ord_weight") if kf.get(k) is not None), None)
    return {"K": int(one.shape[0]), "kf_cap": int(two.shape[1]) if two is not None else 1, "conn_cap": int(rows.shape[1]) if rows is not None else 0}


def _insert_call(fn, d, addr, items, last):
    fr = OrbmkFrames(d["F"], d["kp_cap"], *[addr.get(k) for k in FRAME_KEYS])
    kf = OrbmkKeyframes(d["K"], d["kf_cap"], d["conn_cap"], *[addr.get(k) for k in KEYFRAME_KEYS])
    check(getattr(lib(), fn)(C.byref(fr), C.byref(kf), d["I"], *items, last), fn)


def InsertKeyFrames(frames: dict, keyframes: dict, item_frame, item_kf, item_id, item_baseline=None, device: int = 0):
    """The KeyFrame constructor for the items (frame, keyframe slot, KeyFrame::id, camera.baseline) on `keyframes` (any of
    KEYFRAME_KEYS, numpy) from `frames` (FRAME_KEYS: frame_n and what the given tables are copied from).  Returns updated
    copies of the given keyframe tables."""
    d = dict(_frame_dims(frames), **_keyframe_dims(keyframes))
    fr = {k: _host(frames[k], FRAME_KEYS[k][0], k, _shape(FRAME_KEYS[k][1], d)) for k in FRAME_KEYS if frames.get(k) is not None}
    kf = {k: _host(keyframes[k], KEYFRAME_KEYS[k][0], k, _shape(KEYFRAME_KEYS[k][1], d)).copy() for k in KEYFRAME_KEYS
          if keyframes.get(k) is not None}
    items = [_host(item_frame, np.int32, "item_frame", (None,))]
    d["I"] = len(items[0])
    items += [_host(item_kf, np.int32, "item_kf", (d["I"],)), _host(item_id, np.int32, "item_id", (d["I"],))]
    items.append(None if item_baseline is None else _host(item_baseline, np.float32, "item_baseline", (d["I"],)))
    spare = np.zeros(8, np.int32)                            # an empty array still needs an address
    addr = {k: (ptr(v).value if v.size else ptr(spare).value) for k, v in {**fr, **kf}.items()}
    _insert_call("orbmk_insert_keyframes", d, addr, [None if a is None else (ptr(a) if a.size else ptr(spare)) for a in items], device)
    return kf


def insert_keyframes_device(frames: dict, keyframes: dict, item_frame, item_kf, item_id, item_baseline=None, stream=None):
    """Device form: contiguous CUDA tensors, the given keyframe tables updated in place; the item arrays are tensors too.
    Enqueue only on `stream`."""
    import torch
    d = dict(_frame_dims(frames), **_keyframe_dims(keyframes))
    fr = {k: _dev(frames[k], FRAME_KEYS[k][0], k, _shape(FRAME_KEYS[k][1], d)) for k in FRAME_KEYS if frames.get(k) is not None}
    kf = {k: _dev(keyframes[k], KEYFRAME_KEYS[k][0], k, _shape(KEYFRAME_KEYS[k][1], d)) for k in KEYFRAME_KEYS
          if keyframes.get(k) is not None}
    items = [_dev(item_frame, np.int32, "item_frame", (None,))]
    d["I"] = int(items[0].shape[0])
    items += [_dev(item_kf, np.int32, "item_kf", (d["I"],)), _dev(item_id, np.int32, "item_id", (d["I"],))]
    items.append(None if item_baseline is None else _dev(item_baseline, np.float32, "item_baseline", (d["I"],)))
    spare = torch.zeros(8, dtype=torch.int32, device=items[0].device)
    addr = {k: (v.data_ptr() if v.numel() else spare.data_ptr()) for k, v in {**fr, **kf}.items()}
    _insert_call("orbmk_insert_keyframes_device", d, addr,
                 [None if a is None else (a.data_ptr() if a.numel() else spare.data_ptr()) for a in items], stream_ptr(stream))


def _map_dims(t, lists):
    for k in MAP_KEYS:
        if k not in MAP_OPTIONAL and t.get(k) is None:
            raise ValueError(f"{k} is required")
    for k in LIST_REQUIRED:
        if lists.get(k) is None:
            raise ValueError(f"{k} is required")
    if len(t["kf_mappoint"].shape) != 2 or len(lists["idx1"].shape) != 2:
        raise ValueError("kf_mappoint and idx1 must have two dimensions")
    if t["mp_obs_kf"].shape != t["mp_obs_idx"].shape:
        raise ValueError("mp_obs_kf and mp_obs_idx must have one length")
    M = int(t["mp_bad"].shape[0])
    d = {"K": int(t["kf_mappoint"].shape[0]), "M": M, "M1": M + 1, "kf_cap": int(t["kf_mappoint"].shape[1]),
         "I": int(lists["idx1"].shape[0]), "list_cap": int(lists["idx1"].shape[1]), "F": 0, "kp_cap": 1}
    fm = lists.get("frame_mappoint")
    if fm is not None:
        if len(fm.shape) != 2:
            raise ValueError("frame_mappoint must have two dimensions")
        d.update(F=int(fm.shape[0]), kp_cap=int(fm.shape[1]))
    return d


def _create_call(fn, d, n_obs, by_keypoint, addr, laddr, oaddr, last):
    m = OrbmkMap(d["K"], d["M"], d["kf_cap"], n_obs, *[addr.get(k) for k in MAP_KEYS])
    names = list(LIST_KEYS)
    lst = OrbmkLists(d["I"], d["list_cap"], int(bool(by_keypoint)), *[laddr.get(k) for k in names[:9]], d["F"], d["kp_cap"],
                     laddr.get("item_frame"), laddr.get("frame_mappoint"))
    out = OrbmkCreated(*[oaddr.get(k) for k in OUT_KEYS], d["R"])
    check(getattr(lib(), fn)(C.byref(m), C.byref(lst), C.byref(out), last), fn)


def CreatePoints(tables: dict, lists: dict, alloc: int, values_by_keypoint: bool = False, recent=None, n_recent: int = 0,
                 outputs=("created", "n_created"), device: int = 0):
    """The MapPoint constructor with AddObservation / AddMapPoint / Map::AddMapPoint for the list batch `lists` (LIST_KEYS,
    numpy; kf2 / idx2 left out: one observation) on `tables` (MAP_KEYS; MAP_OPTIONAL may be left out), `alloc` slots in use.
    recent: the array the created slots are appended to at n_recent.  Returns (updated copies of MAP_UPDATED and, where
    given, frame_mappoint; out): out["status"][0] is OK or OVERFLOW, out["alloc"][0] the slots in use afterwards,
    out["needed"] = (slots required, the first slot whose row is too short or -1), out["created"] (I, list_cap) the slot of
    every entry or -1, out["n_created"], out["recent"] / out["n_recent"]."""
    d = _map_dims(tables, lists)
    a = {k: _host(tables[k], MAP_KEYS[k][0], k, _shape(MAP_KEYS[k][1], d)) for k in MAP_KEYS if tables.get(k) is not None}
    for k in MAP_UPDATED:
        if k in a:
            a[k] = a[k].copy()
    ls = {k: _host(lists[k], LIST_KEYS[k][0], k, _shape(LIST_KEYS[k][1], d)) for k in LIST_KEYS if lists.get(k) is not None}
    if "frame_mappoint" in ls:
        ls["frame_mappoint"] = ls["frame_mappoint"].copy()
    out = dict(alloc=np.array([alloc], np.int32), status=np.zeros(1, np.int32), needed=np.zeros(2, np.int32))
    if "created" in outputs:
        out["created"] = np.full((d["I"], d["list_cap"]), -1, np.int32)
    if "n_created" in outputs:
        out["n_created"] = np.zeros(d["I"], np.int32)
    d["R"] = 0
    if recent is not None:
        out["recent"] = _host(recent, np.int32, "recent", (None,)).copy()
        out["n_recent"] = np.array([n_recent], np.int32)
        d["R"] = len(out["recent"])
    spare = np.zeros(8, np.int32)                            # an empty array still needs an address
    adr = lambda x: {k: (ptr(v).value if v.size else ptr(spare).value) for k, v in x.items()}  # noqa: E731
    _create_call("orbmk_create_points", d, len(a["mp_obs_kf"]), values_by_keypoint, adr(a), adr(ls), adr(out), device)
    updated = {k: a[k] for k in MAP_UPDATED if k in a}
    if "frame_mappoint" in ls:
        updated["frame_mappoint"] = ls["frame_mappoint"]
    return updated, out


def create_points_device(tables: dict, lists: dict, alloc, values_by_keypoint: bool = False, recent=None, n_recent=None,
                         out: dict = None, outputs=("created", "n_created"), stream=None):
    """Device form: contiguous CUDA tensors; MAP_UPDATED and lists["frame_mappoint"] are updated in place.  alloc: int32
    tensor of one entry, advanced in place; recent / n_recent: the list and its int32 count, appended to in place.  out: a
    dict returned by an earlier call, to reuse its tensors.  Returns out: alloc, status, needed, and of `outputs` created
    (I, list_cap; -1 where no point was created, which update_normal_depth_device skips) and n_created.  Enqueue only on
    `stream`: read out["status"] when convenient."""
    import torch
    d = _map_dims(tables, lists)
    a = {k: _dev(tables[k], MAP_KEYS[k][0], k, _shape(MAP_KEYS[k][1], d)) for k in MAP_KEYS if tables.get(k) is not None}
    ls = {k: _dev(lists[k], LIST_KEYS[k][0], k, _shape(LIST_KEYS[k][1], d)) for k in LIST_KEYS if lists.get(k) is not None}
    dev = a["mp_bad"].device
    new = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    o = dict(out or {})
    o["alloc"] = _dev(alloc, np.int32, "alloc", (1,))
    o.setdefault("status", new(1))
    o.setdefault("needed", new(2))
    for k, shape in (("created", (d["I"], d["list_cap"])), ("n_created", (d["I"],))):
        if k in outputs:
            o.setdefault(k, new(*shape))
        else:
            o.pop(k, None)
    d["R"] = 0
    o.pop("recent", None), o.pop("n_recent", None)
    if recent is not None:
        o["recent"] = _dev(recent, np.int32, "recent", (None,))
        o["n_recent"] = _dev(n_recent, np.int32, "n_recent", (1,))
        d["R"] = int(recent.shape[0])
    for k in o:
        _dev(o[k], np.int32, k, _shape(OUT_KEYS[k], d))
    spare = torch.zeros(8, dtype=torch.int32, device=dev)
    adr = lambda x: {k: (v.data_ptr() if v.numel() else spare.data_ptr()) for k, v in x.items()}  # noqa: E731
    _create_call("orbmk_create_points_device", d, int(a["mp_obs_kf"].shape[0]), values_by_keypoint, adr(a), adr(ls), adr(o),
                 stream_ptr(stream))
    return o
