"""Optimizer::LocalBundleAdjustment / BundleAdjustment / PoseOptimization / OptimizeSim3 / OptimizeEssentialGraph
mirrors (include/Optimizer.h:40-56) and the GlobalBA thread's map update over the gfx950 C-ABI.

The reference's graph gathering (local KFs by covisibility, local MPs, fixed KFs; Optimizer.cc:493-537)
operates on ORB-SLAM's pointer graph; callers flatten that into a `problem` dict (see
include/orbslam2_amd.h, orbba_problem) and get back optimised poses / points / outlier flags, which
they write back exactly like :677-735.
"""
import ctypes as C

import numpy as np

from ._lib import (KP_DTYPE, BAProblem, BAResult, EssentialGraph, EssentialGraphResult, EssentialGraphTables, GBAMap,
                   GBAOptions, GBAResult, OrbbaMapResult, OrbbaWindow, OrbbaWindowMap, OptSim3Batch, OptSim3Result, PoseBatch, PoseResult, check, lib, ptr, stream_ptr, tptr)


def _need(arrays: dict, counts: dict, what: str):
    """Refuse arrays with fewer elements than the C-ABI reads from them (it has no bound of its own)."""
    for name, want in counts.items():
        a = arrays[name]
        n = a.size if isinstance(a, np.ndarray) else int(a.numel()) if hasattr(a, "numel") else int(np.size(a))
        if n < want:
            raise ValueError(f"{what}: {name} has {n} elements, needs {want}")


def _ba_problem(problem: dict, keep: list, what: str) -> BAProblem:
    """orbba_problem over the dict's arrays (kept alive in `keep`), after the shape checks."""
    def k(a, dt):
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return ptr(a)

    P0, N0, E0 = len(problem["pose_R"]), len(problem["points"]), len(problem["edge_point"])
    _need(problem, {"pose_R": 9 * P0, "pose_t": 3 * P0, "pose_fixed": P0, "points": 3 * N0, "edge_pose": E0,
                    "edge_obs": 3 * E0, "edge_inv_sigma2": E0, "edge_cam": 5 * E0}, what)
    return BAProblem(len(problem["pose_R"]), k(problem["pose_R"], np.float64), k(problem["pose_t"], np.float64),
                     k(problem["pose_fixed"], np.uint8), len(problem["points"]), k(problem["points"], np.float64),
                     len(problem["edge_point"]), k(problem["edge_point"], np.int32), k(problem["edge_pose"], np.int32),
                     k(problem["edge_obs"], np.float64), k(problem["edge_inv_sigma2"], np.float64),
                     k(problem["edge_cam"], np.float64))


def _stop_flag_ptr(stop_flag, keep: list):
    if stop_flag is None:
        return None
    flag = stop_flag if isinstance(stop_flag, C.c_int32) else C.c_int32(int(stop_flag))
    keep.append(flag)
    return C.cast(C.pointer(flag), C.c_void_p)


def LocalBundleAdjustment(problem: dict, stop_flag=None, device: int = 0) -> dict:
    keep = []
    pr = _ba_problem(problem, keep, "LocalBundleAdjustment")
    P, N, E = pr.n_poses, pr.n_points, pr.n_edges
    # (np.empty: orbba_local_ba writes every element of each, also when it optimises nothing)
    out = dict(pose_R=np.empty((P, 9)), pose_t=np.empty((P, 3)), pose_q=np.empty((P, 4)), points=np.empty((N, 3)),
               edge_outlier=np.empty(E, np.uint8), edge_chi2=np.empty(E))
    res = BAResult(ptr(out["pose_R"]), ptr(out["pose_t"]), ptr(out["pose_q"]), ptr(out["points"]),
                   ptr(out["edge_outlier"]), ptr(out["edge_chi2"]))
    sf = _stop_flag_ptr(stop_flag, keep)
    check(lib().orbba_local_ba(C.byref(pr), C.byref(res), sf, device), "orbba_local_ba")
    out["iterations"] = tuple(res.iterations)
    out["chi2"] = tuple(res.chi2)
    out["ran"] = bool(res.ran)   # False: stop flag set on entry, nothing to write back (Optimizer.cc:633-634)
    return out


GBA_STEREO_RULES = {"reference": 0, "local": 1}   # ORBBA_GBA_RULE_REFERENCE / ORBBA_GBA_RULE_LOCAL


def BundleAdjustment(problem: dict, n_iterations: int = 5, robust: bool = True, stereo_rule: str = "reference",
                     stop_flag=None, device: int = 0) -> dict:
    """void Optimizer::BundleAdjustment(keyframes, mappoints, nIterations, stopFlag, loopKFId, robust)
    (src/Optimizer.cc:197-343; GlobalBundleAdjustemnt and Tracking::CreateInitialMapMonocular) on the `problem` dict
    of LocalBundleAdjustment, flattened from :212-294 with pose_fixed = (id == 0).  stereo_rule "reference" types
    the edges by the reference's `if (ur)` (any non-zero ur is a mono edge), "local" as LocalBA does.  Returns
    pose_R / pose_t / pose_q / points (float64), pose_f (P, 12) and points_f (N, 3) = what goes into TcwGBA / posGBA
    or SetPose / SetWorldPos, point_included (N; 0 = no edge, position kept), edge_chi2, iterations, trials, chi2
    and ran (False: the stop flag was set on entry)."""
    if stereo_rule not in GBA_STEREO_RULES:
        raise ValueError(f"BundleAdjustment: stereo_rule must be one of {sorted(GBA_STEREO_RULES)}")
    keep = []
    pr = _ba_problem(problem, keep, "BundleAdjustment")
    P, N, E = pr.n_poses, pr.n_points, pr.n_edges
    out = dict(pose_R=np.empty((P, 9)), pose_t=np.empty((P, 3)), pose_q=np.empty((P, 4)), points=np.empty((N, 3)),
               pose_f=np.empty((P, 12), np.float32), points_f=np.empty((N, 3), np.float32),
               point_included=np.empty(N, np.uint8), edge_chi2=np.empty(E))
    res = GBAResult(*[ptr(out[k]) for k in ("pose_R", "pose_t", "pose_q", "points", "pose_f", "points_f",
                                            "point_included", "edge_chi2")])
    opt = GBAOptions(int(n_iterations), int(bool(robust)), GBA_STEREO_RULES[stereo_rule])
    sf = _stop_flag_ptr(stop_flag, keep)
    check(lib().orbba_bundle_adjustment(C.byref(pr), C.byref(opt), C.byref(res), sf, int(device)), "orbba_bundle_adjustment")
    out.update(iterations=int(res.iterations), trials=int(res.trials), chi2=float(res.chi2), ran=bool(res.ran))
    return out


# orbba_gba_map arrays in struct order: name -> (dtype, rows, row width, updated); O origins, K keyframe slots,
# K1 = K + 1, C children, M map points
_GBA_MAP_KEYS = (("origins", np.int32, "O", 1, False), ("kf_child_off", np.int32, "K1", 1, False),
                 ("kf_child_idx", np.int32, "C", 1, False), ("kf_in_gba", np.uint8, "K", 1, True),
                 ("kf_pose", np.float32, "K", 12, True), ("kf_pose_gba", np.float32, "K", 12, True),
                 ("kf_pose_bef", np.float32, "K", 12, True), ("mp_bad", np.uint8, "M", 1, False),
                 ("mp_in_gba", np.uint8, "M", 1, False), ("mp_pos_gba", np.float32, "M", 3, False),
                 ("mp_ref_kf", np.int32, "M", 1, False), ("mp_xw", np.float32, "M", 3, True))


def _size(a):
    return a.size if isinstance(a, np.ndarray) else int(a.numel()) if hasattr(a, "numel") else int(np.size(a))


def _gba_map_dims(m: dict, what: str):
    for k, _, _, _, _ in _GBA_MAP_KEYS:
        if m.get(k) is None:
            raise ValueError(f"{what}: {k} is required")
    K, M = _size(m["kf_in_gba"]), _size(m["mp_bad"])
    dims = {"O": _size(m["origins"]), "K": K, "K1": K + 1, "M": M}
    _need(m, {k: dims[rows] * width for k, _, rows, width, _ in _GBA_MAP_KEYS if rows != "C"}, what)
    return dims


def GlobalBAUpdateMap(map: dict, device: int = 0) -> dict:
    """The map update of the GlobalBA thread (LoopClosing.cc:392-446) on host arrays in the orbba_gba_map layout
    (include/orbslam2_amd.h): origins, kf_child_off / kf_child_idx (GetChildren() as CSR), kf_in_gba, kf_pose,
    kf_pose_gba, kf_pose_bef (K, 12), mp_bad, mp_in_gba, mp_pos_gba (M, 3), mp_ref_kf and mp_xw (M, 3).  Returns the
    five updated arrays (kf_in_gba, kf_pose, kf_pose_gba, kf_pose_bef, mp_xw) as new arrays; the input is not
    written."""
    dims = _gba_map_dims(map, "GlobalBAUpdateMap")
    arr = {}
    for k, dt, rows, width, updated in _GBA_MAP_KEYS:
        a = np.array(map[k], dt) if updated else np.ascontiguousarray(map[k], dt)   # (np.array copies)
        arr[k] = np.ascontiguousarray(a)
    off = arr["kf_child_off"]
    dims["C"] = int(off[-1]) if len(off) else 0
    _need(arr, {"kf_child_idx": max(dims["C"], 0)}, "GlobalBAUpdateMap")
    gm = GBAMap(dims["K"], dims["M"], dims["O"], *[ptr(arr[k]) for k, _, _, _, _ in _GBA_MAP_KEYS])
    check(lib().orbba_gba_update_map(C.byref(gm), int(device)), "orbba_gba_update_map")
    K, M = dims["K"], dims["M"]
    return dict(kf_in_gba=arr["kf_in_gba"].reshape(K), kf_pose=arr["kf_pose"].reshape(K, 12),
                kf_pose_gba=arr["kf_pose_gba"].reshape(K, 12), kf_pose_bef=arr["kf_pose_bef"].reshape(K, 12),
                mp_xw=arr["mp_xw"].reshape(M, 3))


def global_ba_update_map_device(map: dict, stream=None) -> None:
    """Device form of GlobalBAUpdateMap: GPU tensors for the orbba_gba_map arrays; enqueues two launches on `stream`
    (default: torch's current stream), copies nothing back and updates kf_in_gba, kf_pose, kf_pose_gba, kf_pose_bef
    and mp_xw in place.  kf_child_idx must hold kf_child_off[K] entries (not checked: that would be a copy back)."""
    import torch
    dims = _gba_map_dims(map, "global_ba_update_map_device")
    for name, dt, _, _, _ in _GBA_MAP_KEYS:
        t = map[name]
        if not hasattr(t, "is_cuda") or t.dtype != getattr(torch, np.dtype(dt).name) or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"global_ba_update_map_device: {name} must be a contiguous {np.dtype(dt).name} GPU tensor")
    gm = GBAMap(dims["K"], dims["M"], dims["O"], *[tptr(map[k]) for k, _, _, _, _ in _GBA_MAP_KEYS])
    check(lib().orbba_gba_update_map_device(C.byref(gm), stream_ptr(stream)), "orbba_gba_update_map_device")


def _pose_arrays(batch: dict):
    keep = []

    def k(a, dt):
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return ptr(a)

    n = len(batch["edge_begin"]) - 1
    E = int(batch["edge_begin"][-1]) if n >= 0 and len(batch["edge_begin"]) else 0
    _need(batch, {"pose_R": 9 * n, "pose_t": 3 * n, "cam": 5 * n, "xw": 3 * E, "obs": 3 * E, "inv_sigma2": E},
          "PoseOptimization")
    pb = PoseBatch(n, k(batch["edge_begin"], np.int32), k(batch["pose_R"], np.float64), k(batch["pose_t"], np.float64),
                   k(batch["cam"], np.float64), k(batch["xw"], np.float64), k(batch["obs"], np.float64),
                   k(batch["inv_sigma2"], np.float64))
    return pb, keep


def PoseOptimization(batch: dict, device: int = 0) -> dict:
    """int Optimizer::PoseOptimization(Frame*) (include/Optimizer.h:49, src/Optimizer.cc:345-489) over a
    batch of frames.  `batch` holds, per frame f, the edges [edge_begin[f], edge_begin[f+1]) of the
    keypoints that have a map point, in keypoint order: xw (E,3) map point positions, obs (E,3)
    = (u, v, ur) with ur < 0 for monocular, inv_sigma2 (E,), plus pose_R (F,9) / pose_t (F,3) = frame->pose
    and cam (F,5) = fx, fy, cx, cy, bf.  Returns pose_R / pose_t (the frame->SetPose argument),
    n_inliers (the return value) and outlier (E,) = frame->outlier."""
    pb, keep = _pose_arrays(batch)
    n, E = pb.n_frames, int(batch["edge_begin"][-1]) if len(batch["edge_begin"]) else 0
    out = dict(pose_R=np.zeros((n, 9)), pose_t=np.zeros((n, 3)), n_inliers=np.zeros(n, np.int32),
               outlier=np.zeros(E, np.uint8))
    res = PoseResult(ptr(out["pose_R"]), ptr(out["pose_t"]), ptr(out["n_inliers"]), ptr(out["outlier"]))
    check(lib().orbba_pose_optimization(C.byref(pb), C.byref(res), device), "orbba_pose_optimization")
    return out


def pose_optimization_device(batch: dict, out: dict | None = None, stream=None) -> dict:
    """Device form: `batch` values are torch tensors on the GPU (int32 edge_begin, float64 others);
    enqueues one launch on `stream` (default: torch's current stream) and returns the output tensors."""
    import torch
    eb = batch["edge_begin"]
    n = eb.numel() - 1
    E = batch["inv_sigma2"].numel()
    _need(batch, {"pose_R": 9 * n, "pose_t": 3 * n, "cam": 5 * n, "xw": 3 * E, "obs": 3 * E},
          "pose_optimization_device")
    for name in ("pose_R", "pose_t", "cam", "xw", "obs", "inv_sigma2"):
        t = batch[name]
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"pose_optimization_device: {name} must be a contiguous float64 tensor")
    if eb.dtype != torch.int32 or not eb.is_contiguous():
        raise ValueError("pose_optimization_device: edge_begin must be a contiguous int32 tensor")
    dev = eb.device
    if out is None:
        out = dict(pose_R=torch.empty((n, 9), dtype=torch.float64, device=dev),
                   pose_t=torch.empty((n, 3), dtype=torch.float64, device=dev),
                   n_inliers=torch.empty(n, dtype=torch.int32, device=dev),
                   outlier=torch.empty(max(E, 1), dtype=torch.uint8, device=dev))
    pb = PoseBatch(n, tptr(eb), tptr(batch["pose_R"]), tptr(batch["pose_t"]), tptr(batch["cam"]), tptr(batch["xw"]),
                   tptr(batch["obs"]), tptr(batch["inv_sigma2"]))
    res = PoseResult(tptr(out["pose_R"]), tptr(out["pose_t"]), tptr(out["n_inliers"]), tptr(out["outlier"]))
    check(lib().orbba_pose_optimization_device(C.byref(pb), C.byref(res), stream_ptr(stream)),
          "orbba_pose_optimization_device")
    return out


# orbba_sim3_batch arrays in struct order: name -> (dtype, rows, row width); F pairs, K1 / K2 keypoint slots
_OPTSIM3_KEYS = (("kp1_begin", np.int32, "F1", 1), ("kp2_begin", np.int32, "F1", 1),
                 ("kp1_xy", np.float32, "K1", 2), ("kp1_octave", np.int32, "K1", 1),
                 ("kp2_xy", np.float32, "K2", 2), ("kp2_octave", np.int32, "K2", 1),
                 ("pose1", np.float32, "F", 12), ("camera1", np.float32, "F", 4),
                 ("pose2", np.float32, "F", 12), ("camera2", np.float32, "F", 4),
                 ("mp1_valid", np.uint8, "K1", 1), ("mp1_xw", np.float32, "K1", 3),
                 ("mp2_valid", np.uint8, "K2", 1), ("mp2_xw", np.float32, "K2", 3),
                 ("s12", np.float32, "F", 13), ("match12", np.int32, "K1", 1))


def _optsim3_struct(batch, conv, F, K1, K2, what):
    for k, _, _, _ in _OPTSIM3_KEYS:
        if batch.get(k) is None:
            raise ValueError(f"{what}: {k} is required")
    dims = {"F": F, "F1": F + 1, "K1": K1, "K2": K2}
    _need(batch, {k: dims[rows] * width for k, _, rows, width in _OPTSIM3_KEYS}, what)
    isig = np.ascontiguousarray(batch["inv_level_sigma2"], np.float32)
    sb = OptSim3Batch(F, K1, K2, *[conv(batch[k], dt) for k, dt, _, _ in _OPTSIM3_KEYS], len(isig), ptr(isig),
                      float(batch["max_chi2"]), int(bool(batch["fix_scale"])))
    return sb, isig


def OptimizeSim3(batch: dict, device: int = 0) -> dict:
    """int Optimizer::OptimizeSim3(keyframe1, keyframe2, matches1, S12, maxChi2, fixScale)
    (src/Optimizer.cc:944-1100; LoopClosing.cc:139) batched over (keyframe1, keyframe2, S12) pairs on host
    arrays in the orbba_sim3_batch layout (include/orbslam2_amd.h): SearchBySim3's slot arrays, its match12,
    inv_level_sigma2, max_chi2 and fix_scale.  Returns s12 (F, 13) = S12 on return (the input row when the
    pair returns 0), s12_g2o (F, 8) = q xyzw, t, s of the vertex estimate, match12 (total_kp1) = the thinned
    matches, n_inliers (F) = the return value and iterations (F, 2)."""
    for k in ("kp1_begin", "kp2_begin"):
        if batch.get(k) is None:
            raise ValueError(f"OptimizeSim3: {k} is required")
    F = len(batch["kp1_begin"]) - 1
    K1, K2 = int(batch["kp1_begin"][-1]), int(batch["kp2_begin"][-1])
    keep = []

    def k(a, dt):
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return ptr(a)

    sb, _isig = _optsim3_struct(batch, k, F, K1, K2, "OptimizeSim3")
    out = dict(s12=np.zeros((F, 13), np.float32), s12_g2o=np.zeros((F, 8)), match12=np.zeros(max(K1, 1), np.int32),
               n_inliers=np.zeros(F, np.int32), iterations=np.zeros((F, 2), np.int32))
    res = OptSim3Result(ptr(out["s12"]), ptr(out["s12_g2o"]), ptr(out["match12"]), ptr(out["n_inliers"]),
                        ptr(out["iterations"]))
    check(lib().orbba_optimize_sim3(C.byref(sb), C.byref(res), int(device)), "orbba_optimize_sim3")
    out["match12"] = out["match12"][:K1]
    return out


def optimize_sim3_device(batch: dict, out: dict | None = None, stream=None) -> dict:
    """Device form of OptimizeSim3: GPU tensors for the orbba_sim3_batch arrays (the dtypes of
    search_by_sim3_device, whose match12 output feeds in as it is), host values for inv_level_sigma2,
    max_chi2 and fix_scale; enqueues one launch on `stream` (default: torch's current stream).  `out` may
    hold the output tensors s12, s12_g2o, match12, n_inliers, iterations; out["match12"] may be
    batch["match12"], which is then thinned in place.  n_inliers[p] = -1 for a pair with more than
    ORBBA_SIM3_MAX_CORR correspondences."""
    import torch
    for k in ("kp1_begin", "kp1_xy", "kp2_xy"):
        if batch.get(k) is None:
            raise ValueError(f"optimize_sim3_device: {k} is required")
    kb = batch["kp1_begin"]
    F = kb.numel() - 1
    K1, K2 = int(batch["kp1_xy"].shape[0]), int(batch["kp2_xy"].shape[0])
    for name, dt, _, _ in _OPTSIM3_KEYS:
        t = batch.get(name)
        if t is not None and (t.dtype != getattr(torch, np.dtype(dt).name) or not t.is_contiguous() or not t.is_cuda):
            raise ValueError(f"optimize_sim3_device: {name} must be a contiguous {np.dtype(dt).name} GPU tensor")
    sb, _isig = _optsim3_struct(batch, lambda t, dt: tptr(t), F, K1, K2, "optimize_sim3_device")
    out = dict(out or {})
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=kb.device)   # noqa: E731
    out.setdefault("s12", new((F, 13), torch.float32))
    out.setdefault("s12_g2o", new((F, 8), torch.float64))
    out.setdefault("match12", new(max(K1, 1), torch.int32))
    out.setdefault("n_inliers", new(max(F, 1), torch.int32))
    out.setdefault("iterations", new((max(F, 1), 2), torch.int32))
    _need(out, {"s12": 13 * F, "s12_g2o": 8 * F, "match12": K1, "n_inliers": F, "iterations": 2 * F},
          "optimize_sim3_device")
    res = OptSim3Result(*[tptr(out[k]) for k in ("s12", "s12_g2o", "match12", "n_inliers", "iterations")])
    check(lib().orbba_optimize_sim3_device(C.byref(sb), C.byref(res), stream_ptr(stream)), "orbba_optimize_sim3_device")
    return out


EG_MAX_KEYFRAMES = 512   # ORBBA_EG_MAX_KEYFRAMES
EG_MAX_TRIALS = 200      # ORBBA_EG_MAX_TRIALS
EG_KERNELS = ("setup", "measure", "linearize", "assemble", "begin", "stage", "solve", "update", "chi", "ctl", "recover")

# orbba_essential_graph arrays: name -> (dtype, rows, row width); V keyframe slots, E edges, N points
_EG_KEYS = (("vertex_sim3", np.float32, "V", 13), ("edge_sim3", np.float32, "V", 13), ("edge_i", np.int32, "E", 1),
            ("edge_j", np.int32, "E", 1), ("edge_table", np.uint8, "E", 1), ("points", np.float32, "N", 3),
            ("point_ref", np.int32, "N", 1))


def _eg_struct(graph, conv, V, E, N, what):
    for k, _, _, _ in _EG_KEYS:
        if graph.get(k) is None:
            raise ValueError(f"{what}: {k} is required")
    dims = {"V": V, "E": E, "N": N}
    _need(graph, {k: dims[rows] * width for k, _, rows, width in _EG_KEYS}, what)
    p = {k: conv(graph[k], dt) for k, dt, _, _ in _EG_KEYS}
    return EssentialGraph(V, p["vertex_sim3"], p["edge_sim3"], int(graph["fixed_slot"]), int(bool(graph["fix_scale"])), E,
                          p["edge_i"], p["edge_j"], p["edge_table"], N, p["points"], p["point_ref"])


def _eg_dims(graph):
    size = lambda a: a.size if isinstance(a, np.ndarray) else int(a.numel()) if hasattr(a, "numel") else int(np.size(a))   # noqa: E731
    for k in ("vertex_sim3", "edge_i", "point_ref"):
        if graph.get(k) is None:
            raise ValueError(f"OptimizeEssentialGraph: {k} is required")
    return size(graph["vertex_sim3"]) // 13, size(graph["edge_i"]), size(graph["point_ref"])


def OptimizeEssentialGraph(graph: dict, device: int = 0, profile: bool = False) -> dict:
    """void Optimizer::OptimizeEssentialGraph(map, loopKF, currKF, nonCorrectedSim3, correctedSim3, loopConnections,
    fixScale) (src/Optimizer.cc:743-942; LoopClosing::CorrectLoop) on host arrays in the orbba_essential_graph layout
    (include/orbslam2_amd.h): vertex_sim3 / edge_sim3 (V, 13), fixed_slot, fix_scale, edge_i / edge_j / edge_table (E;
    essential_graph_edges builds them), points (N, 3), point_ref (N, -1 = skip).  Returns sim3_g2o (V, 8), pose (V, 12),
    points (N, 3), measurement (E, 8), iterations, trials, chi2 and accept (the trials' accept flags, in order);
    with profile=True also kernel_ms, the device time per kernel (EG_KERNELS)."""
    V, E, N = _eg_dims(graph)
    keep = []

    def k(a, dt):
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return ptr(a)

    eg = _eg_struct(graph, k, V, E, N, "OptimizeEssentialGraph")
    out = dict(sim3_g2o=np.zeros((V, 8)), pose=np.zeros((V, 12), np.float32), points=np.zeros((max(N, 1), 3), np.float32),
               measurement=np.zeros((max(E, 1), 8)))
    it, chi2, acc = np.zeros(2, np.int32), np.zeros(1), np.zeros(EG_MAX_TRIALS, np.uint8)
    res = EssentialGraphResult(ptr(out["sim3_g2o"]), ptr(out["pose"]), ptr(out["points"]), ptr(out["measurement"]), ptr(it),
                               ptr(chi2), ptr(acc))
    if profile:
        ms = np.zeros(len(EG_KERNELS), np.float32)
        check(lib().orbba_essential_graph_profile(C.byref(eg), C.byref(res), int(device), ptr(ms)), "orbba_essential_graph_profile")
        out["kernel_ms"] = dict(zip(EG_KERNELS, ms.tolist()))
    else:
        check(lib().orbba_optimize_essential_graph(C.byref(eg), C.byref(res), int(device)), "orbba_optimize_essential_graph")
    out["points"], out["measurement"] = out["points"][:N], out["measurement"][:E]
    out.update(iterations=int(it[0]), trials=int(it[1]), chi2=float(chi2[0]), accept=acc[:int(it[1])].astype(bool))
    return out


def optimize_essential_graph_device(graph: dict, out: dict | None = None, stream=None) -> dict:
    """Device form of OptimizeEssentialGraph: GPU tensors for the orbba_essential_graph arrays, host values for
    fixed_slot and fix_scale; enqueues the whole optimisation on `stream` (default: torch's current stream) and
    copies nothing back.  `out` may hold the output tensors sim3_g2o (V, 8) f64, pose (V, 12) f32, points (N, 3)
    f32, measurement (E, 8) f64, iterations (2) i32 = (iterations, trials), chi2 (1) f64 and accept
    (EG_MAX_TRIALS) u8.  An edge with an index out of range is left out of the graph."""
    import torch
    V, E, N = _eg_dims(graph)
    for name, dt, _, _ in _EG_KEYS:
        t = graph.get(name)
        if t is not None and (t.dtype != getattr(torch, np.dtype(dt).name) or not t.is_contiguous() or not t.is_cuda):
            raise ValueError(f"optimize_essential_graph_device: {name} must be a contiguous {np.dtype(dt).name} GPU tensor")
    eg = _eg_struct(graph, lambda t, dt: tptr(t), V, E, N, "optimize_essential_graph_device")
    out = dict(out or {})
    dev = graph["vertex_sim3"].device
    want = {"sim3_g2o": ((V, 8), torch.float64), "pose": ((V, 12), torch.float32), "points": ((max(N, 1), 3), torch.float32),
            "measurement": ((max(E, 1), 8), torch.float64), "iterations": ((2,), torch.int32), "chi2": ((1,), torch.float64),
            "accept": ((EG_MAX_TRIALS,), torch.uint8)}
    for name, (shape, dt) in want.items():
        out.setdefault(name, torch.empty(shape, dtype=dt, device=dev))
        t = out[name]
        if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"optimize_essential_graph_device: out[{name!r}] must be a contiguous {dt} GPU tensor")
    _need(out, {"sim3_g2o": 8 * V, "pose": 12 * V, "points": 3 * N, "measurement": 8 * E, "iterations": 2, "chi2": 1,
                "accept": EG_MAX_TRIALS}, "optimize_essential_graph_device")
    res = EssentialGraphResult(*[tptr(out[k]) for k in ("sim3_g2o", "pose", "points", "measurement", "iterations", "chi2", "accept")])
    check(lib().orbba_optimize_essential_graph_device(C.byref(eg), C.byref(res), stream_ptr(stream)),
          "orbba_optimize_essential_graph_device")
    return out


def essential_graph_edges(tables: dict, min_weight: int = 100):
    """The edge list of Optimizer.cc:798-903 from slot tables (orbba_eg_tables in include/orbslam2_amd.h): kf_id (V),
    parent (V, -1 = none), loop_edges and covisibles (V lists of slots; covisibles as (slot, weight) pairs in
    GetCovisiblesByWeight order, slot -1 for a bad keyframe), loop_connections (a list of (slot, [slots]) in the
    map's iteration order), curr_slot and loop_slot.  Children are the slots whose parent is the keyframe.  Returns
    edge_i, edge_j (int32) and edge_table (uint8) in the reference's insertion order.  Host only."""
    V = len(tables["kf_id"])

    def rows(lists):
        begin = np.zeros(len(lists) + 1, np.int32)
        begin[1:] = np.cumsum([len(l) for l in lists])
        return begin, [v for l in lists for v in l]

    lb, ls = rows(tables["loop_edges"])
    cb, cv = rows(tables["covisibles"])
    nb, ns = rows([c[1] for c in tables["loop_connections"]])
    if len(tables["parent"]) != V or len(lb) != V + 1 or len(cb) != V + 1:
        raise ValueError("essential_graph_edges: parent, loop_edges and covisibles need one row per keyframe")
    arr = lambda v, n=1: np.ascontiguousarray(np.asarray(v, np.int32).reshape(-1, n) if len(v) else np.zeros((0, n), np.int32))   # noqa: E731
    cv2 = arr(cv, 2)
    a = dict(kf_id=arr(tables["kf_id"]), parent=arr(tables["parent"]), lb=lb, ls=arr(ls), cb=cb,
             cs=np.ascontiguousarray(cv2[:, 0]), cw=np.ascontiguousarray(cv2[:, 1]),
             ck=arr([c[0] for c in tables["loop_connections"]]), nb=nb, ns=arr(ns))
    t = EssentialGraphTables(V, ptr(a["kf_id"]), ptr(a["parent"]), ptr(a["lb"]), ptr(a["ls"]), ptr(a["cb"]), ptr(a["cs"]),
                             ptr(a["cw"]), len(tables["loop_connections"]), ptr(a["ck"]), ptr(a["nb"]), ptr(a["ns"]),
                             int(tables["curr_slot"]), int(tables["loop_slot"]))
    n = np.zeros(1, np.int32)
    check(lib().orbba_essential_graph_edges(C.byref(t), int(min_weight), 0, None, None, None, ptr(n)), "orbba_essential_graph_edges")
    E = int(n[0])
    ei, ej, et = np.zeros(max(E, 1), np.int32), np.zeros(max(E, 1), np.int32), np.zeros(max(E, 1), np.uint8)
    check(lib().orbba_essential_graph_edges(C.byref(t), int(min_weight), E, ptr(ei), ptr(ej), ptr(et), ptr(n)),
          "orbba_essential_graph_edges")
    return ei[:E], ej[:E], et[:E]


# ---- LocalBundleAdjustment on the device-resident map (orbba_local_window / _apply / _map, include/orbslam2_amd.h)
WINDOW_OK, WINDOW_OVERFLOW = 0, 1
# orbba_window_map's arrays in struct order: name -> (dtype, shape); K keyframes, M map points, M1 = M + 1, L levels.
# kf_keypoint: KP_DTYPE records on the host, their bytes as (K, kf_cap, 7) float32 on the device.
WINDOW_MAP_KEYS = {
    "inv_sigma2": (np.float32, ("L",)), "scale_factors": (np.float32, ("L",)), "kf_id": (np.int32, ("K",)),
    "kf_n": (np.int32, ("K",)), "kf_bad": (np.uint8, ("K",)), "kf_mappoint": (np.int32, ("K", "kf_cap")),
    "kf_keypoint": (KP_DTYPE, ("K", "kf_cap")), "kf_kp_octave": (np.int32, ("K", "kf_cap")),
    "kf_uright": (np.float32, ("K", "kf_cap")), "kf_camera": (np.float32, ("K", 6)), "kf_pose": (np.float32, ("K", 12)),
    "ord_slot": (np.int32, ("K", "conn_cap")), "n_ord": (np.int32, ("K",)), "mp_bad": (np.uint8, ("M",)),
    "mp_xw": (np.float32, ("M", 3)), "mp_nobs": (np.int32, ("M",)), "mp_ref_kf": (np.int32, ("M",)),
    "mp_obs_off": (np.int32, ("M1",)), "mp_obs_kf": (np.int32, ("n_obs",)), "mp_obs_idx": (np.int32, ("n_obs",)),
    "mp_normal": (np.float32, ("M", 3)), "mp_max_min": (np.float32, ("M", 2)),
}
WINDOW_HOST_KEYS = ("inv_sigma2", "scale_factors")   # host memory in both forms
WINDOW_GATHER_KEYS = ("inv_sigma2", "kf_id", "kf_n", "kf_bad", "kf_mappoint", "kf_keypoint", "kf_uright", "kf_camera", "ord_slot",
                      "n_ord", "mp_bad", "mp_obs_off", "mp_obs_kf", "mp_obs_idx")
WINDOW_UPDATED = ("kf_mappoint", "kf_pose", "mp_bad", "mp_xw", "mp_nobs", "mp_ref_kf", "mp_obs_kf", "mp_normal", "mp_max_min")
# orbba_window's arrays in struct order: name -> (dtype, capacity, row width)
WINDOW_KEYS = {"counts": (np.int32, None, 8), "pose_kf": (np.int32, "poses", 1), "pose_fixed": (np.uint8, "poses", 1),
               "point": (np.int32, "points", 1), "edge_point": (np.int32, "edges", 1), "edge_pose": (np.int32, "edges", 1),
               "edge_kf": (np.int32, "edges", 1), "edge_idx": (np.int32, "edges", 1), "edge_obs": (np.float32, "edges", 3),
               "edge_inv_sigma2": (np.float32, "edges", 1), "edge_cam": (np.float32, "edges", 5)}


def _window_dims(t: dict):
    for k in ("kf_mappoint", "ord_slot", "mp_bad", "mp_obs_kf", "inv_sigma2"):
        if t.get(k) is None:
            raise ValueError(f"{k} is required")
    if len(t["kf_mappoint"].shape) != 2 or len(t["ord_slot"].shape) != 2:
        raise ValueError("kf_mappoint and ord_slot must have two dimensions")
    M = int(t["mp_bad"].shape[0])
    return {"K": int(t["kf_mappoint"].shape[0]), "M": M, "M1": M + 1, "kf_cap": int(t["kf_mappoint"].shape[1]),
            "conn_cap": int(t["ord_slot"].shape[1]), "n_obs": int(t["mp_obs_kf"].shape[0]), "L": len(t["inv_sigma2"])}


def _window_map(tables: dict, keys, on_device: bool, keep: list, updated=()):
    """(orbba_window_map, the arrays by name) over `keys` of the tables; the others stay NULL."""
    d = _window_dims(tables)
    arrays, addr = {}, {}
    for k in keys:
        dt, spec = WINDOW_MAP_KEYS[k]
        want = tuple(d[x] if isinstance(x, str) else x for x in spec)
        a = tables.get(k)
        if a is None:
            raise ValueError(f"{k} is required")
        if on_device and k not in WINDOW_HOST_KEYS:
            import torch
            tt, want = ((torch.float32, want + (7,)) if k == "kf_keypoint" else
                        ({np.int32: torch.int32, np.uint8: torch.uint8, np.float32: torch.float32}[dt], want))
            if not isinstance(a, torch.Tensor) or not a.is_cuda or a.dtype != tt or not a.is_contiguous() or tuple(a.shape) != want:
                raise ValueError(f"{k} must be a contiguous {tt} GPU tensor of shape {want}")
            addr[k] = a.data_ptr()
            if not a.numel():
                spare = torch.zeros(8, dtype=torch.int32, device=a.device)
                keep.append(spare)
                addr[k] = spare.data_ptr()
        else:
            a = np.ascontiguousarray(a)
            if a.dtype != dt or a.shape != want:
                raise ValueError(f"{k} must be {np.dtype(dt)} of shape {want}, not {a.dtype} {a.shape}")
            if k in updated:
                a = a.copy()
            keep.append(a)
            addr[k] = a.ctypes.data if a.size else ptr(np.zeros(8, np.int32)).value
        arrays[k] = a
    m = OrbbaWindowMap(d["K"], d["M"], d["kf_cap"], d["conn_cap"], d["n_obs"], d["L"], *[addr.get(k) for k in WINDOW_MAP_KEYS])
    return m, arrays, d


def _window_caps(d: dict, caps):
    caps = caps or {}
    return {"poses": int(caps.get("poses", d["K"])), "points": int(caps.get("points", d["M"])), "edges": int(caps.get("edges", d["n_obs"]))}


def _window_struct(window: dict, caps: dict, on_device: bool, keep: list):
    addr = {}
    for k, (dt, cap, width) in WINDOW_KEYS.items():
        n = (caps[cap] if cap else 1) * width
        a = window[k]
        if on_device:
            if int(a.numel()) < n or not a.is_cuda or not a.is_contiguous():
                raise ValueError(f"window {k} must be a contiguous GPU tensor of at least {n} entries")
            addr[k] = a.data_ptr()
        else:
            if a.size < n or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError(f"window {k} must be contiguous {np.dtype(dt)} of at least {n} entries")
            addr[k] = a.ctypes.data
        keep.append(a)
    return OrbbaWindow(caps["poses"], caps["points"], caps["edges"], *[addr[k] for k in WINDOW_KEYS])


def new_window(caps: dict, device=None) -> dict:
    """Buffers of an orbba_window with the capacities caps = {"poses", "points", "edges"}: numpy arrays, or GPU tensors on
    the torch device `device`.  A capacity of 0 still gets an address."""
    shape = lambda cap, width: (max(caps[cap], 1) if cap else 1) * width   # noqa: E731
    if device is None:
        return {k: np.zeros(shape(cap, w), dt) for k, (dt, cap, w) in WINDOW_KEYS.items()}
    import torch
    tt = {np.int32: torch.int32, np.uint8: torch.uint8, np.float32: torch.float32}
    return {k: torch.zeros(shape(cap, w), dtype=tt[dt], device=device) for k, (dt, cap, w) in WINDOW_KEYS.items()}


def LocalWindow(tables: dict, cur: int, caps: dict | None = None, window: dict | None = None, device: int = 0) -> dict:
    """The window of LocalBundleAdjustment(cur) (src/Optimizer.cc:493-631) on `tables` (WINDOW_GATHER_KEYS of
    WINDOW_MAP_KEYS, numpy): the arrays of WINDOW_KEYS at the capacities `caps` (default: K poses, M points, n_obs
    edges), counts = n_local, n_fixed, n_points, n_edges, status (WINDOW_*), one camera.  `window` to write into given
    buffers."""
    keep = []
    m, _, d = _window_map(tables, WINDOW_GATHER_KEYS, False, keep)
    caps = _window_caps(d, caps)
    window = window if window is not None else new_window(caps)
    w = _window_struct(window, caps, False, keep)
    check(lib().orbba_local_window(C.byref(m), int(cur), C.byref(w), device), "orbba_local_window")
    return window


def local_window_device(tables: dict, cur: int, caps: dict | None = None, window: dict | None = None, stream=None) -> dict:
    """Device form: GPU tensors but for inv_sigma2; the window's tensors (`window` to reuse them).  Enqueue only on
    `stream`."""
    keep = []
    m, a, d = _window_map(tables, WINDOW_GATHER_KEYS, True, keep)
    caps = _window_caps(d, caps)
    window = window if window is not None else new_window(caps, a["mp_bad"].device)
    w = _window_struct(window, caps, True, keep)
    check(lib().orbba_local_window_device(C.byref(m), int(cur), C.byref(w), stream_ptr(stream)), "orbba_local_window_device")
    return window


def _window_given_caps(window: dict):
    n = lambda a: int(a.numel()) if hasattr(a, "numel") else int(a.size)   # noqa: E731
    return {"poses": min(n(window["pose_kf"]), n(window["pose_fixed"])), "points": n(window["point"]),
            "edges": min(n(window["edge_point"]), n(window["edge_obs"]) // 3, n(window["edge_cam"]) // 5)}


def LocalBAApply(tables: dict, window: dict, outlier, pose_R, pose_t, points, device: int = 0) -> dict:
    """LocalBundleAdjustment's write-back (:677-735) on `tables` (WINDOW_MAP_KEYS, numpy) for the edges flagged in
    `outlier` and the estimates pose_R (P, 9), pose_t (P, 3), points (N, 3) in the window's order.  Returns the updated
    copies of WINDOW_UPDATED."""
    keep = []
    m, a, d = _window_map(tables, tuple(k for k in WINDOW_MAP_KEYS), False, keep, WINDOW_UPDATED)
    caps = _window_given_caps(window)
    w = _window_struct(window, caps, False, keep)
    fit = lambda x, dt, n: np.concatenate([np.ascontiguousarray(x, dt).reshape(-1), np.zeros(n, dt)])[:max(n, 1)].copy()   # noqa: E731
    o, R, t, X = (fit(outlier, np.uint8, caps["edges"]), fit(pose_R, np.float64, 9 * caps["poses"]),
                  fit(pose_t, np.float64, 3 * caps["poses"]), fit(points, np.float64, 3 * caps["points"]))
    check(lib().orbba_local_ba_apply(C.byref(m), C.byref(w), ptr(o), ptr(R), ptr(t), ptr(X), device), "orbba_local_ba_apply")
    return {k: a[k] for k in WINDOW_UPDATED}


def local_ba_apply_device(tables: dict, window: dict, outlier, pose_R, pose_t, points, stream=None) -> None:
    """Device form: WINDOW_UPDATED updated in place; outlier (uint8), pose_R, pose_t, points (float64) GPU tensors of at
    least the window's capacities.  Enqueue only on `stream`."""
    keep = []
    m, _, d = _window_map(tables, tuple(k for k in WINDOW_MAP_KEYS), True, keep)
    caps = _window_given_caps(window)
    w = _window_struct(window, caps, True, keep)
    for name, x, n in (("outlier", outlier, caps["edges"]), ("pose_R", pose_R, 9 * caps["poses"]),
                       ("pose_t", pose_t, 3 * caps["poses"]), ("points", points, 3 * caps["points"])):
        if not x.is_cuda or not x.is_contiguous() or int(x.numel()) < n:
            raise ValueError(f"{name} must be a contiguous GPU tensor of at least {n} entries")
    check(lib().orbba_local_ba_apply_device(C.byref(m), C.byref(w), outlier.data_ptr(), pose_R.data_ptr(), pose_t.data_ptr(),
                                            points.data_ptr(), stream_ptr(stream)), "orbba_local_ba_apply_device")


def _map_result(r: OrbbaMapResult) -> dict:
    return dict(iterations=tuple(r.iterations), chi2=tuple(r.chi2), ran=bool(r.ran), counts=tuple(r.counts), status=int(r.status))


def LocalBundleAdjustmentMap(tables: dict, cur: int, stop_flag=None, device: int = 0):
    """Optimizer::LocalBundleAdjustment(cur, stopFlag, map) as a whole (src/Optimizer.cc:491-736) on `tables`
    (WINDOW_MAP_KEYS, numpy).  Returns (the updated copies of WINDOW_UPDATED, dict(iterations, chi2, ran, counts,
    status))."""
    keep = []
    m, a, _ = _window_map(tables, tuple(k for k in WINDOW_MAP_KEYS), False, keep, WINDOW_UPDATED)
    r = OrbbaMapResult()
    sf = _stop_flag_ptr(stop_flag, keep)
    check(lib().orbba_local_ba_map(C.byref(m), int(cur), C.byref(r), sf, device), "orbba_local_ba_map")
    return {k: a[k] for k in WINDOW_UPDATED}, _map_result(r)


def local_ba_map_device(tables: dict, cur: int, window: dict | None = None, caps: dict | None = None, stop_flag=None,
                        stream=None):
    """Device form: the tables are GPU tensors updated in place, nothing of the map crosses to the host.  The LM loop is
    host-driven, so the call returns once it has ended; work enqueued on `stream` afterwards sees the applied tables.
    Returns (result dict, window)."""
    keep = []
    m, a, d = _window_map(tables, tuple(k for k in WINDOW_MAP_KEYS), True, keep)
    caps = _window_caps(d, caps) if window is None else _window_given_caps(window)
    window = window if window is not None else new_window(caps, a["mp_bad"].device)
    w = _window_struct(window, caps, True, keep)
    r = OrbbaMapResult()
    sf = _stop_flag_ptr(stop_flag, keep)
    check(lib().orbba_local_ba_map_device(C.byref(m), int(cur), C.byref(w), C.byref(r), sf, stream_ptr(stream)),
          "orbba_local_ba_map_device")
    return _map_result(r), window
