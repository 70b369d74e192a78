"""Map maintenance over the gfx950 C-ABI (orbmm_*, include/orbslam2_amd.h): MapPoint::UpdateNormalAndDepth
(src/MapPoint.cc:341-380) batched over map points, KeyFrame::UpdateConnections with AddConnection / UpdateBestCovisibles
(src/KeyFrame.cc:94-119, 235-309) batched over keyframes, the GetChildren() CSR and the packed covisibility tables.

The tables are dicts of slot arrays: POINT_KEYS for the normals and distances, GRAPH_KEYS for the connections (STATE_KEYS of
them are read and updated).  The capitalised functions take numpy arrays, are synchronous and return updated copies; the
*_device functions take CUDA tensors, update them in place and only enqueue."""
import ctypes as C

import numpy as np

from ._lib import OrbmmCsr, OrbmmGraph, OrbmmPoints, check, lib, ptr, stream_ptr
from .local_map import COVIS, _dev, _host, _shape

OK, CONN_OVERFLOW = 0, 1
THRESHOLD = 15

# name: (dtype, shape); K keyframes, M map points, None = free
POINT_KEYS = {
    "mp_bad": (np.uint8, ("M",)), "mp_xw": (np.float32, ("M", 3)), "mp_ref_kf": (np.int32, ("M",)),
    "mp_obs_off": (np.int32, ("M1",)), "mp_obs_kf": (np.int32, (None,)), "mp_obs_idx": (np.int32, (None,)),
    "kf_pose": (np.float32, ("K", 12)), "kf_n": (np.int32, ("K",)), "kf_kp_octave": (np.int32, ("K", "kf_cap")),
    "mp_normal": (np.float32, ("M", 3)), "mp_max_min": (np.float32, ("M", 2)),
}
POINT_UPDATED = ("mp_normal", "mp_max_min")
GRAPH_KEYS = {
    "kf_id": (np.int32, ("K",)), "kf_n": (np.int32, ("K",)), "kf_mappoint": (np.int32, ("K", "kf_cap")),
    "mp_bad": (np.uint8, ("M",)), "mp_obs_off": (np.int32, ("M1",)), "mp_obs_kf": (np.int32, (None,)),
    "conn_slot": (np.int32, ("K", "conn_cap")), "conn_weight": (np.int32, ("K", "conn_cap")), "n_conn": (np.int32, ("K",)),
    "ord_slot": (np.int32, ("K", "conn_cap")), "ord_weight": (np.int32, ("K", "conn_cap")), "n_ord": (np.int32, ("K",)),
    "kf_first_connection": (np.uint8, ("K",)), "kf_parent": (np.int32, ("K",)), "kf_covis": (np.int32, ("K", COVIS)),
}
STATE_KEYS = ("conn_slot", "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord", "kf_first_connection", "kf_parent",
              "kf_covis")
ROW_KEYS = STATE_KEYS[:6]


def _need(t, *keys):
    for k in keys:
        if t.get(k) is None:
            raise ValueError(f"{k} is required")


def _point_dims(t):
    _need(t, "mp_bad", "kf_n", "kf_kp_octave", "mp_obs_kf", "mp_obs_idx")
    if len(t["kf_kp_octave"].shape) != 2:
        raise ValueError("kf_kp_octave must have two dimensions")
    K, M = int(t["kf_n"].shape[0]), int(t["mp_bad"].shape[0])
    if t["mp_obs_kf"].shape != t["mp_obs_idx"].shape:
        raise ValueError("mp_obs_kf and mp_obs_idx must have one length")
    return {"K": K, "M": M, "M1": M + 1, "kf_cap": int(t["kf_kp_octave"].shape[1])}


def _graph_dims(t, rows_only=False):
    _need(t, "n_conn", "conn_slot")
    if len(t["conn_slot"].shape) != 2:
        raise ValueError("conn_slot must have two dimensions")
    d = {"K": int(t["n_conn"].shape[0]), "conn_cap": int(t["conn_slot"].shape[1]), "M": 0, "M1": 1, "kf_cap": 0}
    if not rows_only:
        _need(t, "mp_bad", "kf_mappoint", "mp_obs_kf")
        if len(t["kf_mappoint"].shape) != 2:
            raise ValueError("kf_mappoint must have two dimensions")
        M = int(t["mp_bad"].shape[0])
        d.update(M=M, M1=M + 1, kf_cap=int(t["kf_mappoint"].shape[1]))
    return d


def _scales(scale_factors):
    s = np.ascontiguousarray(scale_factors, np.float32)
    if s.ndim != 1:
        raise ValueError("scale_factors must have one dimension")
    return s


def _points_struct(d, addr, n_obs, scales, point_addr, n_points):
    return OrbmmPoints(d["K"], d["M"], d["kf_cap"], n_obs, len(scales), ptr(scales).value,
                       *[addr[k] for k in ("mp_bad", "mp_xw", "mp_ref_kf", "mp_obs_off", "mp_obs_kf", "mp_obs_idx", "kf_pose",
                                           "kf_n", "kf_kp_octave")], n_points, point_addr, addr["mp_normal"], addr["mp_max_min"])


def _graph_struct(d, addr, n_obs, status_addr):
    return OrbmmGraph(d["K"], d["M"], d["kf_cap"], d["conn_cap"], n_obs, *[addr.get(k) for k in GRAPH_KEYS], status_addr)


def _addr_host(a):
    spare = np.zeros(4, np.int32)   # an empty list still needs an address
    return {k: (ptr(v).value if v.size else ptr(spare).value) for k, v in a.items()}, spare


def _addr_dev(a, dev):
    import torch
    spare = torch.zeros(4, dtype=torch.int32, device=dev)
    return {k: (v.data_ptr() if v.numel() else spare.data_ptr()) for k, v in a.items()}, spare


def UpdateNormalAndDepth(tables: dict, scale_factors, points=None, device: int = 0):
    """UpdateNormalAndDepth for the point slots `points` (None: every point) of `tables` (POINT_KEYS, numpy).  Returns the
    updated copies (mp_normal, mp_max_min); a bad point, one without observations and one whose reference slot is -1
    keep their rows."""
    d = _point_dims(tables)
    a = {k: _host(tables.get(k), dt, k, _shape(sp, d)) for k, (dt, sp) in POINT_KEYS.items()}
    for k in POINT_UPDATED:
        a[k] = a[k].copy()
    scales = _scales(scale_factors)
    pts = None if points is None else np.ascontiguousarray(points, np.int32).reshape(-1)
    addr, spare = _addr_host(a)
    p = _points_struct(d, addr, len(a["mp_obs_kf"]), scales, None if pts is None else (ptr(pts).value if pts.size else ptr(spare).value),
                       0 if pts is None else len(pts))
    check(lib().orbmm_update_normal_depth(C.byref(p), device), "orbmm_update_normal_depth")
    return a["mp_normal"], a["mp_max_min"]


def update_normal_depth_device(tables: dict, scale_factors, points=None, stream=None) -> None:
    """Device form: every array of POINT_KEYS a contiguous CUDA tensor (scale_factors host); mp_normal and mp_max_min are
    updated in place.  `points`: an int32 CUDA tensor of point slots, or None for every point.  Enqueue only on `stream`."""
    import torch
    d = _point_dims(tables)
    a = {k: _dev(tables.get(k), dt, k, _shape(sp, d)) for k, (dt, sp) in POINT_KEYS.items()}
    scales = _scales(scale_factors)
    addr, spare = _addr_dev(a, a["mp_bad"].device)
    if points is not None:
        points = _dev(points, np.int32, "points", (None,))
    p = _points_struct(d, addr, int(a["mp_obs_kf"].shape[0]), scales,
                       None if points is None else (points.data_ptr() if points.numel() else spare.data_ptr()),
                       0 if points is None else int(points.numel()))
    check(lib().orbmm_update_normal_depth_device(C.byref(p), stream_ptr(stream)), "orbmm_update_normal_depth_device")


def UpdateConnections(graph: dict, items, device: int = 0) -> dict:
    """UpdateConnections for the keyframe slots `items`, in order, on `graph` (GRAPH_KEYS, numpy).  Returns the updated
    copies of STATE_KEYS and status (per keyframe: OK or CONN_OVERFLOW, whose keyframe keeps its rows)."""
    d = _graph_dims(graph)
    a = {k: _host(graph.get(k), dt, k, _shape(sp, d)) for k, (dt, sp) in GRAPH_KEYS.items()}
    for k in STATE_KEYS:
        a[k] = a[k].copy()
    it = np.ascontiguousarray(items, np.int32).reshape(-1)
    status = np.zeros(d["K"], np.int32)
    addr, spare = _addr_host(a)
    g = _graph_struct(d, addr, len(a["mp_obs_kf"]), ptr(status).value if status.size else ptr(spare).value)
    check(lib().orbmm_update_connections(C.byref(g), len(it), ptr(it) if it.size else ptr(spare), device),
          "orbmm_update_connections")
    out = {k: a[k] for k in STATE_KEYS}
    out["status"] = status
    return out


def update_connections_device(graph: dict, items, status=None, stream=None):
    """Device form: every array of GRAPH_KEYS a contiguous CUDA tensor, STATE_KEYS updated in place; `items` an int32 CUDA
    tensor of keyframe slots.  Returns the status tensor (`status` to reuse one).  Enqueue only on `stream`."""
    import torch
    d = _graph_dims(graph)
    a = {k: _dev(graph.get(k), dt, k, _shape(sp, d)) for k, (dt, sp) in GRAPH_KEYS.items()}
    items = _dev(items, np.int32, "items", (None,))
    dev = a["kf_id"].device
    if status is None:
        status = torch.empty(d["K"], dtype=torch.int32, device=dev)
    _dev(status, np.int32, "status", (d["K"],))
    addr, spare = _addr_dev(a, dev)
    g = _graph_struct(d, addr, int(a["mp_obs_kf"].shape[0]), status.data_ptr() if status.numel() else spare.data_ptr())
    check(lib().orbmm_update_connections_device(C.byref(g), int(items.numel()), items.data_ptr() if items.numel() else spare.data_ptr(),
                                                stream_ptr(stream)), "orbmm_update_connections_device")
    return status


def Children(kf_parent, device: int = 0):
    """(kf_child_off, kf_child_idx): the GetChildren() CSR as the inverse of kf_parent, each list ascending."""
    par = _host(kf_parent, np.int32, "kf_parent", (None,))
    K = len(par)
    off, idx = np.zeros(K + 1, np.int32), np.zeros(max(K, 1), np.int32)
    check(lib().orbmm_children(K, ptr(par) if K else ptr(idx), ptr(off), ptr(idx), device), "orbmm_children")
    return off, idx[:int(off[-1])]


def children_device(kf_parent, out=None, stream=None):
    """Device form.  Returns (kf_child_off, kf_child_idx) with K + 1 and K entries; the lists end at kf_child_off[K]."""
    import torch
    par = _dev(kf_parent, np.int32, "kf_parent", (None,))
    K = int(par.shape[0])
    off, idx = out if out is not None else (torch.empty(K + 1, dtype=torch.int32, device=par.device),
                                            torch.zeros(max(K, 1), dtype=torch.int32, device=par.device))
    _dev(off, np.int32, "kf_child_off", (K + 1,))
    _dev(idx, np.int32, "kf_child_idx", (max(K, 1),))
    check(lib().orbmm_children_device(K, par.data_ptr() if K else idx.data_ptr(), off.data_ptr(), idx.data_ptr(), stream_ptr(stream)),
          "orbmm_children_device")
    return off, idx


def _csr_struct(addr, kf_bad, out, queries, spare_addr, append_self):
    q = 0 if queries is None else int(queries.shape[0])
    return OrbmmCsr(kf_bad, out.get("covis_begin"), out.get("covis_slot"), out.get("covis_weight"), q,
                    None if queries is None else (addr["query"] if q else spare_addr), 1 if append_self else 0,
                    out.get("conn_off"), out.get("conn_idx"))


def CovisCsr(graph: dict, kf_bad=None, queries=None, append_self: bool = False, covis: bool = True, device: int = 0) -> dict:
    """The packed forms of the rows of `graph` (ROW_KEYS, numpy).  covis: covis_begin / covis_slot / covis_weight as
    orbba_eg_tables takes them (a bad keyframe is -1).  queries: conn_off / conn_idx as orbdb_query_batch takes them, for
    these keyframe slots, each list ascending, with the query's own slot appended if append_self."""
    d = _graph_dims(graph, rows_only=True)
    K, cap = d["K"], d["conn_cap"]
    a = {k: _host(graph.get(k), GRAPH_KEYS[k][0], k, _shape(GRAPH_KEYS[k][1], d)) for k in ROW_KEYS}
    bad = None if kf_bad is None else _host(kf_bad, np.uint8, "kf_bad", (K,))
    out = {}
    if covis:
        out.update(covis_begin=np.zeros(K + 1, np.int32), covis_slot=np.full(max(K * cap, 1), -1, np.int32),
                   covis_weight=np.zeros(max(K * cap, 1), np.int32))
    if queries is not None:
        queries = np.ascontiguousarray(queries, np.int32).reshape(-1)
        a["query"] = queries
        out.update(conn_off=np.zeros(len(queries) + 1, np.int32), conn_idx=np.full(max(len(queries) * (cap + 1), 1), -1, np.int32))
    addr, spare = _addr_host(a)
    g = _graph_struct(d, addr, 0, None)
    c = _csr_struct(addr, None if bad is None or not bad.size else ptr(bad).value, {k: ptr(v).value for k, v in out.items()},
                    queries, ptr(spare).value, append_self)
    check(lib().orbmm_covis_csr(C.byref(g), C.byref(c), device), "orbmm_covis_csr")
    if covis:
        n = int(out["covis_begin"][-1])
        out["covis_slot"], out["covis_weight"] = out["covis_slot"][:n], out["covis_weight"][:n]
    if queries is not None:
        out["conn_idx"] = out["conn_idx"][:int(out["conn_off"][-1])]
    return out


def covis_csr_device(graph: dict, kf_bad=None, queries=None, append_self: bool = False, covis: bool = True, stream=None) -> dict:
    """Device form: ROW_KEYS, kf_bad and queries CUDA tensors.  Returns tensors at full capacity (covis_slot / covis_weight
    K * conn_cap entries, conn_idx len(queries) * (conn_cap + 1)); the lists end at covis_begin[K] / conn_off[-1]."""
    import torch
    d = _graph_dims(graph, rows_only=True)
    K, cap = d["K"], d["conn_cap"]
    a = {k: _dev(graph.get(k), GRAPH_KEYS[k][0], k, _shape(GRAPH_KEYS[k][1], d)) for k in ROW_KEYS}
    dev = a["n_conn"].device
    bad = None if kf_bad is None else _dev(kf_bad, np.uint8, "kf_bad", (K,))
    new = lambda n, fill: torch.full((max(n, 1),), fill, dtype=torch.int32, device=dev)  # noqa: E731
    out = {}
    if covis:
        out.update(covis_begin=new(K + 1, 0), covis_slot=new(K * cap, -1), covis_weight=new(K * cap, 0))
    if queries is not None:
        queries = _dev(queries, np.int32, "queries", (None,))
        a["query"] = queries
        out.update(conn_off=new(int(queries.shape[0]) + 1, 0), conn_idx=new(int(queries.shape[0]) * (cap + 1), -1))
    addr, spare = _addr_dev(a, dev)
    g = _graph_struct(d, addr, 0, None)
    c = _csr_struct(addr, None if bad is None or not bad.numel() else bad.data_ptr(), {k: v.data_ptr() for k, v in out.items()},
                    queries, spare.data_ptr(), append_self)
    check(lib().orbmm_covis_csr_device(C.byref(g), C.byref(c), stream_ptr(stream)), "orbmm_covis_csr_device")
    return out
