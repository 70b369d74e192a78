"""LoopCorrector::Correct (src/LoopClosing.cc:546-676) over the gfx950 C-ABI (orblc_*, orbba_essential_graph_edges_device;
include/orbslam2_amd.h, "LoopCorrector::Correct"): the connected list, the propagation of Scw to the current keyframe's
neighbours with the correction of their map points and poses, the LoopConnections sets and the edge list of
OptimizeEssentialGraph, in place on the tables of map_maintenance.py.

The map is a dict of slot arrays, MAP_KEYS: GRAPH_KEYS and POINT_KEYS of map_maintenance.py plus mp_corrected_by
(MapPoint::correctedByKF, a KeyFrame::id, initially 0) and mp_corrected_ref (correctedReference, a slot).  Where the
reference iterates a std::map<KeyFrame*, ...> the order is ascending slot.  The capitalised functions take numpy arrays, are
synchronous and return updated copies; the *_device functions take CUDA tensors, update them in place and only enqueue."""
import ctypes as C

import numpy as np

from ._lib import EssentialGraphTables, OrblcMap, check, lib, ptr, stream_ptr
from .local_map import _dev, _host, _shape
from .map_maintenance import GRAPH_KEYS, POINT_KEYS, STATE_KEYS, UpdateConnections, _addr_dev, _addr_host, update_connections_device

MAP_KEYS = dict(GRAPH_KEYS)
MAP_KEYS.update(POINT_KEYS)
MAP_KEYS.update(mp_corrected_by=(np.int32, ("M",)), mp_corrected_ref=(np.int32, ("M",)))
ROW_KEYS = ("ord_slot", "n_ord")
PROPAGATE_KEYS = ("kf_id", "kf_n", "kf_mappoint", "mp_bad", "mp_obs_off", "mp_obs_kf", "mp_obs_idx", "mp_ref_kf", "kf_kp_octave",
                  "mp_xw", "kf_pose", "mp_normal", "mp_max_min", "mp_corrected_by", "mp_corrected_ref")
PROPAGATE_UPDATED = ("mp_xw", "kf_pose", "mp_normal", "mp_max_min", "mp_corrected_by", "mp_corrected_ref")
# the order of orblc_map's pointers after scale_factors
_STRUCT_ORDER = ("kf_id", "kf_n", "kf_mappoint", "mp_bad", "mp_obs_off", "mp_obs_kf", "conn_slot", "conn_weight", "n_conn",
                 "ord_slot", "ord_weight", "n_ord", "kf_first_connection", "kf_parent", "kf_covis", "status", "mp_obs_idx",
                 "mp_ref_kf", "kf_kp_octave", "mp_xw", "kf_pose", "mp_normal", "mp_max_min", "mp_corrected_by", "mp_corrected_ref")


def _dims(t, rows_only=False):
    for k in ("n_conn", "conn_slot") + (() if rows_only else ("mp_bad", "kf_mappoint")):
        if t.get(k) is None:
            raise ValueError(f"{k} is required")
    if len(t["conn_slot"].shape) != 2:
        raise ValueError("conn_slot must have two dimensions")
    d = {"K": int(t["n_conn"].shape[0]), "conn_cap": int(t["conn_slot"].shape[1]), "M": 0, "M1": 1, "kf_cap": 1}
    if not rows_only:
        if len(t["kf_mappoint"].shape) != 2:
            raise ValueError("kf_mappoint must have two dimensions")
        M = int(t["mp_bad"].shape[0])
        d.update(M=M, M1=M + 1, kf_cap=int(t["kf_mappoint"].shape[1]))
    return d


def _struct(d, addr, n_obs, scales=None):
    """scales: the caller's float32 array, which outlives the call; None for the entries that read no scale (n_levels 1, a
    null pointer)."""
    return OrblcMap(d["K"], d["M"], d["kf_cap"], d["conn_cap"], n_obs, 1 if scales is None else len(scales),
                    None if scales is None else ptr(scales).value, *[addr.get(k) for k in _STRUCT_ORDER])


def _scales(scale_factors):
    s = np.ascontiguousarray(scale_factors, np.float32)
    if s.ndim != 1:
        raise ValueError("scale_factors must have one dimension")
    return s


def _host_map(tables, keys, updated=(), rows_only=False):
    d = _dims(tables, rows_only)
    a = {k: _host(tables.get(k), MAP_KEYS[k][0], k, _shape(MAP_KEYS[k][1], d)) for k in keys}
    for k in updated:
        a[k] = a[k].copy()
    addr, spare = _addr_host(a)
    return d, a, addr, spare


def _dev_map(tables, keys, rows_only=False):
    d = _dims(tables, rows_only)
    a = {k: _dev(tables.get(k), MAP_KEYS[k][0], k, _shape(MAP_KEYS[k][1], d)) for k in keys}
    addr, spare = _addr_dev(a, a[keys[0]].device)
    return d, a, addr, spare


def _n_obs(a):
    return int(a["mp_obs_kf"].shape[0]) if "mp_obs_kf" in a else 0


# ------------------------------------------------------------------------------------------ the connected list
def Connected(tables: dict, cur: int, device: int = 0):
    """connectedKFs of :550-552: (connected [conn_cap + 1], the ordered row of `cur`, then cur, then -1; its count)."""
    d, a, addr, _ = _host_map(tables, ("conn_slot", "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord"), rows_only=True)
    connected, n = np.full(d["conn_cap"] + 1, -1, np.int32), np.zeros(1, np.int32)
    check(lib().orblc_connected(C.byref(_struct(d, addr, 0)), int(cur), ptr(connected), ptr(n), device),
          "orblc_connected")
    return connected, int(n[0])


def connected_device(tables: dict, cur: int, out=None, stream=None):
    """Device form.  Returns (connected, n_connected) as int32 CUDA tensors of conn_cap + 1 and 1 entries (`out` to reuse)."""
    import torch
    d, a, addr, _ = _dev_map(tables, ("conn_slot", "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord"), rows_only=True)
    dev = a["n_ord"].device
    connected, n = out if out is not None else (torch.empty(d["conn_cap"] + 1, dtype=torch.int32, device=dev),
                                                torch.empty(1, dtype=torch.int32, device=dev))
    _dev(connected, np.int32, "connected", (d["conn_cap"] + 1,))
    _dev(n, np.int32, "n_connected", (1,))
    check(lib().orblc_connected_device(C.byref(_struct(d, addr, 0)), int(cur), connected.data_ptr(), n.data_ptr(),
                                       stream_ptr(stream)), "orblc_connected_device")
    return connected, n


# ------------------------------------------------------------------------------------------ the propagation
def Propagate(tables: dict, scale_factors, cur: int, scw, connected, update_connections: bool = True, device: int = 0) -> dict:
    """:554-613 on `tables` (MAP_KEYS, numpy) with scw (13: R row-major, t, s) and the list `connected` (entries of -1 are
    skipped).  Returns the updated copies of PROPAGATE_UPDATED, vertex_sim3 / edge_sim3 (K, 13), point_ref (M), items (the
    connected slots ascending, then -1) and, with update_connections (:612), STATE_KEYS and status after UpdateConnections
    of the items in that order."""
    d, a, addr, spare = _host_map(tables, PROPAGATE_KEYS, PROPAGATE_UPDATED)
    scales = _scales(scale_factors)
    scw = np.ascontiguousarray(scw, np.float32).reshape(13)
    lst = np.ascontiguousarray(connected, np.int32).reshape(-1)
    out = dict(vertex_sim3=np.zeros((d["K"], 13), np.float32), edge_sim3=np.zeros((d["K"], 13), np.float32),
               point_ref=np.zeros(max(d["M"], 1), np.int32), items=np.full(max(len(lst), 1), -1, np.int32))
    check(lib().orblc_propagate(C.byref(_struct(d, addr, _n_obs(a), scales)), int(cur), ptr(scw), ptr(lst) if lst.size else ptr(spare),
                                len(lst), ptr(out["vertex_sim3"]), ptr(out["edge_sim3"]), ptr(out["point_ref"]), ptr(out["items"]),
                                device), "orblc_propagate")
    out["point_ref"], out["items"] = out["point_ref"][:d["M"]], out["items"][:len(lst)]
    out.update({k: a[k] for k in PROPAGATE_UPDATED})
    if update_connections:
        out.update(UpdateConnections(tables, out["items"][out["items"] >= 0], device))
    return out


def propagate_device(tables: dict, scale_factors, cur: int, scw, connected, max_connected: int = None, out: dict = None,
                     update_connections: bool = True, stream=None) -> dict:
    """Device form: MAP_KEYS, scw (13 floats) and connected (conn_cap + 1, from connected_device) CUDA tensors;
    PROPAGATE_UPDATED are updated in place.  max_connected: n_connected read back, or None for conn_cap + 1.  Returns
    vertex_sim3, edge_sim3, point_ref and items as tensors (`out` to reuse them) and, with update_connections, enqueues
    update_connections_device of the items behind it (status in the result)."""
    import torch
    d, a, addr, _ = _dev_map(tables, PROPAGATE_KEYS)
    dev = a["kf_id"].device
    scales = _scales(scale_factors)
    _dev(scw, np.float32, "scw", (13,))
    _dev(connected, np.int32, "connected", (None,))
    n = int(connected.shape[0]) if max_connected is None else int(max_connected)
    if n > int(connected.shape[0]):
        raise ValueError("max_connected is larger than connected")
    out = dict(out or {})
    want = {"vertex_sim3": ((d["K"], 13), np.float32), "edge_sim3": ((d["K"], 13), np.float32), "point_ref": ((max(d["M"], 1),), np.int32),
            "items": ((max(n, 1),), np.int32)}
    for k, (shape, dt) in want.items():
        out.setdefault(k, torch.empty(shape, dtype=getattr(torch, np.dtype(dt).name), device=dev))
        _dev(out[k], dt, k, shape)
    check(lib().orblc_propagate_device(C.byref(_struct(d, addr, _n_obs(a), scales)), int(cur), scw.data_ptr(), connected.data_ptr(), n,
                                       out["vertex_sim3"].data_ptr(), out["edge_sim3"].data_ptr(), out["point_ref"].data_ptr(),
                                       out["items"].data_ptr(), stream_ptr(stream)), "orblc_propagate_device")
    if update_connections:
        out["status"] = update_connections_device(tables, out["items"][:n], out.get("status"), stream)
    return out


# ------------------------------------------------------------------------------------------ LoopConnections
_LOOP_KEYS = tuple(GRAPH_KEYS)


def LoopConnections(tables: dict, connected, device: int = 0) -> dict:
    """:661-676 on `tables` (GRAPH_KEYS, numpy): for each entry of `connected` in list order, UpdateConnections and the new
    links.  Returns (state, sets): the updated copies of STATE_KEYS with status, and conn_kf / conn_begin / conn_slot as
    orbba_eg_tables takes them (rows in ascending slot order, the rows of skipped entries cut off) with n_connections."""
    d, a, addr, spare = _host_map(tables, _LOOP_KEYS, STATE_KEYS)
    lst = np.ascontiguousarray(connected, np.int32).reshape(-1)
    C_ = len(lst)
    status = np.zeros(max(d["K"], 1), np.int32)
    addr["status"] = ptr(status).value
    out = dict(conn_kf=np.full(max(C_, 1), -1, np.int32), conn_begin=np.zeros(C_ + 1, np.int32),
               conn_slot=np.full(max(C_ * d["conn_cap"], 1), -1, np.int32))
    n = np.zeros(1, np.int32)
    check(lib().orblc_loop_connections(C.byref(_struct(d, addr, _n_obs(a))), ptr(lst) if C_ else ptr(spare), C_,
                                       ptr(out["conn_kf"]), ptr(out["conn_begin"]), ptr(out["conn_slot"]), ptr(n), device),
          "orblc_loop_connections")
    n = int(n[0])
    sets = dict(conn_kf=out["conn_kf"][:n], conn_begin=out["conn_begin"][:n + 1], conn_slot=out["conn_slot"][:int(out["conn_begin"][n])],
                n_connections=n)
    state = {k: a[k] for k in STATE_KEYS}
    state["status"] = status[:d["K"]]
    return state, sets


def loop_connections_device(tables: dict, connected, max_connected: int = None, out: dict = None, stream=None) -> dict:
    """Device form: GRAPH_KEYS and connected CUDA tensors, STATE_KEYS updated in place.  Returns conn_kf (max_connected),
    conn_begin (max_connected + 1), conn_slot (max_connected * conn_cap), n_connections (1) and status (K) as tensors."""
    import torch
    d, a, addr, _ = _dev_map(tables, _LOOP_KEYS)
    dev = a["kf_id"].device
    _dev(connected, np.int32, "connected", (None,))
    n = int(connected.shape[0]) if max_connected is None else int(max_connected)
    if n > int(connected.shape[0]):
        raise ValueError("max_connected is larger than connected")
    out = dict(out or {})
    want = {"conn_kf": max(n, 1), "conn_begin": n + 1, "conn_slot": max(n * d["conn_cap"], 1), "n_connections": 1, "status": max(d["K"], 1)}
    for k, size in want.items():
        out.setdefault(k, torch.full((size,), -1, dtype=torch.int32, device=dev))
        _dev(out[k], np.int32, k, (size,))
    addr["status"] = out["status"].data_ptr()
    check(lib().orblc_loop_connections_device(C.byref(_struct(d, addr, _n_obs(a))), connected.data_ptr(), n,
                                              out["conn_kf"].data_ptr(), out["conn_begin"].data_ptr(), out["conn_slot"].data_ptr(),
                                              out["n_connections"].data_ptr(), stream_ptr(stream)), "orblc_loop_connections_device")
    return out


# ------------------------------------------------------------------------------------------ the edge list
_EDGE_KEYS = ("kf_id", "parent", "loop_begin", "loop_slot", "covis_begin", "covis_slot", "covis_weight", "conn_kf", "conn_begin",
              "conn_slot")


def essential_graph_edges_device(tables: dict, capacity: int, min_weight: int = 100, n_connections: int = None, out: dict = None,
                                 stream=None) -> dict:
    """optimizer.essential_graph_edges on the device: `tables` holds the arrays of orbba_eg_tables (_EDGE_KEYS) as int32 CUDA
    tensors and the host integers curr_slot and loop_kf_slot; n_connections: the rows of conn_kf to read (None: all of them; a
    row of -1 is skipped).  Returns edge_i, edge_j (int32), edge_table (uint8), each `capacity` long and (-1, -1, 0) past the
    list, and n_edges (1), the full count."""
    import torch
    t = {k: _dev(tables.get(k), np.int32, k, (None,)) for k in _EDGE_KEYS}
    dev = t["kf_id"].device
    V = int(t["kf_id"].shape[0])
    if int(t["parent"].shape[0]) != V or int(t["loop_begin"].shape[0]) != V + 1 or int(t["covis_begin"].shape[0]) != V + 1:
        raise ValueError("parent, loop_begin and covis_begin need one row per keyframe")
    if t["covis_slot"].shape != t["covis_weight"].shape:
        raise ValueError("covis_slot and covis_weight must have one length")
    nc = int(t["conn_kf"].shape[0]) if n_connections is None else int(n_connections)
    if nc > int(t["conn_kf"].shape[0]) or nc + 1 > int(t["conn_begin"].shape[0]):
        raise ValueError("n_connections is larger than conn_kf / conn_begin")
    spare = torch.zeros(4, dtype=torch.int32, device=dev)
    addr = {k: (v.data_ptr() if v.numel() else spare.data_ptr()) for k, v in t.items()}
    g = EssentialGraphTables(V, addr["kf_id"], addr["parent"], addr["loop_begin"], addr["loop_slot"], addr["covis_begin"],
                             addr["covis_slot"], addr["covis_weight"], nc, addr["conn_kf"], addr["conn_begin"], addr["conn_slot"],
                             int(tables["curr_slot"]), int(tables["loop_kf_slot"]))
    out = dict(out or {})
    cap = max(int(capacity), 1)
    out.setdefault("edge_i", torch.empty(cap, dtype=torch.int32, device=dev))
    out.setdefault("edge_j", torch.empty(cap, dtype=torch.int32, device=dev))
    out.setdefault("edge_table", torch.empty(cap, dtype=torch.uint8, device=dev))
    out.setdefault("n_edges", torch.empty(1, dtype=torch.int32, device=dev))
    _dev(out["edge_i"], np.int32, "edge_i", (cap,))
    _dev(out["edge_j"], np.int32, "edge_j", (cap,))
    _dev(out["edge_table"], np.uint8, "edge_table", (cap,))
    _dev(out["n_edges"], np.int32, "n_edges", (1,))
    check(lib().orbba_essential_graph_edges_device(C.byref(g), int(t["loop_slot"].numel()), int(t["covis_slot"].numel()),
                                                   int(t["conn_slot"].numel()), int(min_weight), int(capacity),
                                                   out["edge_i"].data_ptr(), out["edge_j"].data_ptr(), out["edge_table"].data_ptr(),
                                                   out["n_edges"].data_ptr(), stream_ptr(stream)),
          "orbba_essential_graph_edges_device")
    return out
