"""Seeded essential-graph problems in the orbba_essential_graph layout (include/orbslam2_amd.h): a keyframe chain
whose odometry drifts, a loop edge that closes it, and map points hung on reference slots.

make_graph: keyframe k sits at the drifted pose T_k (scale 1).  LoopClosing::CorrectLoop has already moved the last
`n_corrected` keyframes (the current keyframe and its neighbours) by the loop's Sim3 `corr`: their vertex rows hold
corrected Sim3s, their edge-side rows the poses from before the correction, as correctedSim3 / nonCorrectedSim3 do.
Edges, in the reference's insertion order: the loop connection (curr = last slot, loop = slot 0, vertex table), then
per keyframe its spanning-tree edge to the previous keyframe and `covis` covisibility edges to earlier keyframes."""
import numpy as np


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def row13(R, t, s=1.0):
    return np.concatenate([np.asarray(R, np.float64).reshape(-1), np.asarray(t, np.float64).reshape(-1), [s]]).astype(np.float32)


def make_graph(seed=0, n_kf=13, n_corrected=2, corr_deg=3.0, corr_t=0.3, corr_s=1.1, covis=0, n_points=0, fix_scale=0,
               fixed_slot=0, loop=True, step_deg=8.0, isolated=(), skip_every=0):
    rng = np.random.default_rng(seed)
    R, t = np.eye(3), np.zeros(3)
    poses = []
    for k in range(n_kf):   # world -> camera, a drifting arc
        poses.append((R.copy(), t.copy()))
        dR = rot(rng.normal(size=3) * 0.2 + [0, 1, 0], step_deg + rng.normal() * 0.5)
        R = dR @ R
        t = dR @ t + np.array([0.5, 0.02, 0.1]) + rng.normal(size=3) * 0.02
    vertex = np.stack([row13(Rk, tk) for Rk, tk in poses])
    edge = vertex.copy()
    # the correction: a Sim3 on the world side, Scw' = Scw * corr^-1 (CorrectLoop propagates it to the neighbours)
    Rc, tc = rot(rng.normal(size=3), corr_deg), rng.normal(size=3) * corr_t
    for k in range(n_kf - n_corrected, n_kf):
        Rk, tk = poses[k]
        Ri = Rc.T
        vertex[k] = row13(Rk @ Ri, tk - (1.0 / corr_s) * (Rk @ Ri @ tc), 1.0 / corr_s)
    ei, ej, et = [], [], []
    live = [k for k in range(n_kf) if k not in isolated]
    if loop:
        ei.append(live[-1]); ej.append(live[0]); et.append(0)
    for n, k in enumerate(live):
        if n > 0:
            ei.append(k); ej.append(live[n - 1]); et.append(1)
        for c in range(covis):
            m = n - 2 - c
            if m >= 0 and (k + c) % 2 == 0:
                ei.append(k); ej.append(live[m]); et.append(1)
    pts = (rng.normal(size=(n_points, 3)) * 3).astype(np.float32)
    ref = rng.integers(0, n_kf, n_points).astype(np.int32)
    if skip_every:
        ref[::skip_every] = -1
    return dict(vertex_sim3=vertex, edge_sim3=edge, fixed_slot=fixed_slot, fix_scale=fix_scale,
                edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32), edge_table=np.array(et, np.uint8),
                points=pts, point_ref=ref)
