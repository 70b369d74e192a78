"""Optimizer::LocalBundleAdjustment's window (src/Optimizer.cc:493-631) and write-back (:677-735) on slot tables, one entry
after another in numpy: what orbba_local_window / orbba_local_ba_apply / orbba_local_ba_map compute (include/orbslam2_amd.h).
Slots stand for pointers, -1 is null; a slot or index outside its table is skipped.

Departure, once: the reference walks MapPoint::GetObservations(), a std::map<KeyFrame*, size_t>, in pointer order (:527,
:583), which no two runs share; here that order is the CSR's (mp_obs_off / mp_obs_kf), as in map_maintenance_ref.py and
culling_ref.py.  It decides the order of the fixed cameras and of a point's edges, and so the low bits of the solve."""
import numpy as np

import culling_ref as CR
import map_maintenance_ref as MR

OK, OVERFLOW = 0, 1
UPDATED = ("kf_mappoint", "kf_pose", "mp_bad", "mp_xw", "mp_nobs", "mp_ref_kf", "mp_obs_kf", "mp_normal", "mp_max_min")
WINDOW_ARRAYS = ("pose_kf", "pose_fixed", "point", "edge_point", "edge_pose", "edge_kf", "edge_idx", "edge_obs",
                 "edge_inv_sigma2", "edge_cam")


def _observations(t, p):
    """(entry, keyframe) of p's observations in CSR order, without the erased ones (:527)."""
    K, n_obs = len(t["kf_n"]), len(t["mp_obs_kf"])
    e0, e1 = max(int(t["mp_obs_off"][p]), 0), min(int(t["mp_obs_off"][p + 1]), n_obs)
    return [(e, int(t["mp_obs_kf"][e])) for e in range(e0, e1) if 0 <= t["mp_obs_kf"][e] < K]


def gather(t, cur, caps=None):
    """The window of LocalBundleAdjustment(cur): dict(counts = (n_local, n_fixed, n_points, n_edges), status, one_cam and
    WINDOW_ARRAYS).  caps = (poses, points, edges): past one of them the status is OVERFLOW and the arrays are None."""
    K, M, kf_cap = len(t["kf_n"]), len(t["mp_bad"]), t["kf_mappoint"].shape[1]
    conn_cap, n_levels = t["ord_slot"].shape[1], len(t["inv_sigma2"])
    # :496-504 local keyframes; BALocalForKF is `local`
    local, local_kfs = {cur}, [cur]
    for i in range(min(max(int(t["n_ord"][cur]), 0), conn_cap)):
        s = int(t["ord_slot"][cur, i])
        if not 0 <= s < K or s in local:
            continue
        local.add(s)                                         # neighborKF->BALocalForKF = id, bad or not
        if not t["kf_bad"][s]:
            local_kfs.append(s)
    # :507-521 local points
    seen, local_mps = set(), []
    for k in local_kfs:
        for i in range(min(max(int(t["kf_n"][k]), 0), kf_cap)):
            p = int(t["kf_mappoint"][k, i])
            if not 0 <= p < M or t["mp_bad"][p] or p in seen:
                continue
            seen.add(p)
            local_mps.append(p)
    # :524-537 fixed cameras; BAFixedForKF is `fixed`
    fixed, fixed_kfs = set(), []
    for p in local_mps:
        for _, o in _observations(t, p):
            if o in local or o in fixed:
                continue
            fixed.add(o)
            if not t["kf_bad"][o]:
                fixed_kfs.append(o)
    poses = local_kfs + fixed_kfs
    vertex = {k: i for i, k in enumerate(poses)}
    # :576-631 edges
    edges = []
    for j, p in enumerate(local_mps):
        for e, o in _observations(t, p):
            idx = int(t["mp_obs_idx"][e])
            if t["kf_bad"][o] or not 0 <= idx < kf_cap or not 0 <= t["kf_keypoint"][o, idx]["octave"] < n_levels:
                continue
            edges.append((j, vertex[o], o, idx))
    counts = (len(local_kfs), len(fixed_kfs), len(local_mps), len(edges))
    w = dict(counts=counts, status=OK, one_cam=1, **{k: None for k in WINDOW_ARRAYS})
    if caps is not None and (len(poses) > caps[0] or len(local_mps) > caps[1] or len(edges) > caps[2]):
        w["status"] = OVERFLOW
        return w
    kp = t["kf_keypoint"]
    w.update(pose_kf=np.array(poses, np.int32),
             pose_fixed=np.array([t["kf_id"][k] == 0 for k in local_kfs] + [1] * len(fixed_kfs), np.uint8),
             point=np.array(local_mps, np.int32),
             edge_point=np.array([e[0] for e in edges], np.int32), edge_pose=np.array([e[1] for e in edges], np.int32),
             edge_kf=np.array([e[2] for e in edges], np.int32), edge_idx=np.array([e[3] for e in edges], np.int32),
             edge_obs=np.array([(kp[o, i]["x"], kp[o, i]["y"], t["kf_uright"][o, i]) for _, _, o, i in edges], np.float32).reshape(-1, 3),
             edge_inv_sigma2=np.array([t["inv_sigma2"][kp[o, i]["octave"]] for _, _, o, i in edges], np.float32),
             edge_cam=np.array([t["kf_camera"][o, :5] for _, _, o, _ in edges], np.float32).reshape(-1, 5))
    w["one_cam"] = int(all(np.array_equal(c, t["kf_camera"][cur, :5]) for c in w["edge_cam"]))
    return w


def flatten(t, w):
    """The window as orbba_local_ba's problem (optimizer.LocalBundleAdjustment's dict): every float widened exactly."""
    pose = t["kf_pose"][w["pose_kf"]].astype(np.float64)
    return dict(pose_R=pose[:, :9].copy(), pose_t=pose[:, 9:].copy(), pose_fixed=w["pose_fixed"].copy(),
                points=t["mp_xw"][w["point"]].astype(np.float64), edge_point=w["edge_point"].copy(), edge_pose=w["edge_pose"].copy(),
                edge_obs=w["edge_obs"].astype(np.float64), edge_inv_sigma2=w["edge_inv_sigma2"].astype(np.float64),
                edge_cam=w["edge_cam"].astype(np.float64))


def apply(t, w, outlier, pose_R, pose_t, points):
    """The write-back (:677-735) for the edges flagged in `outlier` and the estimates in the window's order.  Returns the
    updated copies of UPDATED."""
    if w["status"] != OK:
        return {k: t[k].copy() for k in UPDATED}
    m = CR.Map(t)
    u = m.t
    for e in np.flatnonzero(np.asarray(outlier)[:len(w["edge_point"])]):   # :709-715, in edge order
        p, k = int(w["point"][w["edge_point"][e]]), int(w["edge_kf"][e])
        hit = [idx for _, o, idx in m.observations(p) if o == k]   # GetIndexInKeyFrame
        if not hit:                                          # a point gone bad observes nothing: both calls do nothing
            continue
        if 0 <= hit[0] < m.kf_cap:
            u["kf_mappoint"][k, hit[0]] = -1                 # EraseMapPointMatch(mappoint)
        m.erase_observation(p, k)
    n_local = w["counts"][0]
    for i in range(n_local):                                 # :721-726 FromSE3Quat narrows element by element
        u["kf_pose"][w["pose_kf"][i], :9] = np.asarray(pose_R, np.float64).reshape(-1, 9)[i].astype(np.float32)
        u["kf_pose"][w["pose_kf"][i], 9:] = np.asarray(pose_t, np.float64).reshape(-1, 3)[i].astype(np.float32)
    for j, p in enumerate(w["point"]):                       # :729-735
        u["mp_xw"][p] = np.asarray(points, np.float64).reshape(-1, 3)[j].astype(np.float32)
    u["mp_normal"], u["mp_max_min"] = MR.update_normal_depth(u, t["scale_factors"], w["point"])
    return {k: u[k] for k in UPDATED}
