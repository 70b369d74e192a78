"""Geometrically consistent maps for LocalBundleAdjustment on slot tables: synth.make_ba_problem's geometry and noise turned
into orbba_window_map's tables with synth.local_map_tables.  The problem's local keyframes are slots 0 .. n_kf - 1 (slot 0 has
id 0), cur is the last of them and its ordered row lists the others nearest first; the problem's fixed cameras follow.  Planted
on top: a bad neighbour in cur's row and a bad keyframe outside it, both observing local points; a null entry with its
observation erased; a bad point left in the rows.  make_ba_problem's 3 % gross outliers give the erasures."""
import functools

import numpy as np

from orb_slam2_refactored_amd import KP_DTYPE, synth

N_LEVELS = 8
SCALE = np.array([1.2 ** i for i in range(N_LEVELS)], np.float32)
INV_SIGMA2 = np.array([np.float32(1.0 / ((1.2 ** i) * (1.2 ** i))) for i in range(N_LEVELS)], np.float32)   # make_ba_problem's
# name: (seed, local keyframes, points, fixed cameras, kf_cap): "small" solves in LDS, "large" (24 free keyframes) in HBM
CASES = {"small": (3, 6, 300, 3, 320), "large": (5, 24, 500, 2, 224)}
CONN_CAP = 32


@functools.lru_cache(maxsize=None)
def case(name):
    """(tables, cur)"""
    seed, n_kf, n_pts, n_fixed, kf_cap = CASES[name]
    pr = synth.make_ba_problem(seed=seed, n_kf=n_kf, n_pts=n_pts, n_fixed=n_fixed)
    rng = np.random.default_rng(seed + 100)
    P, M = n_kf + n_fixed, n_pts
    K = P + 2
    bad_nb, bad_obs = P, P + 1
    kf_mappoint = np.full((K, kf_cap), -1, np.int32)
    kf_n = np.zeros(K, np.int32)
    kp = np.zeros((K, kf_cap), KP_DTYPE)
    kp["octave"] = 0
    uright = np.full((K, kf_cap), -1, np.float32)

    def add(k, p, u, v, ur, octave):
        i = int(kf_n[k])
        assert i < kf_cap
        kf_mappoint[k, i] = p
        kp[k, i]["x"], kp[k, i]["y"], kp[k, i]["octave"] = u, v, octave
        uright[k, i] = ur
        kf_n[k] = i + 1

    for e in range(len(pr["edge_point"])):
        octave = int(np.flatnonzero(INV_SIGMA2 == np.float32(pr["edge_inv_sigma2"][e]))[0])
        add(int(pr["edge_pose"][e]), int(pr["edge_point"][e]), *pr["edge_obs"][e], octave)
    for k in (bad_nb, bad_obs):                              # the bad keyframes see a few points each, wherever
        for p in rng.choice(M, 12, replace=False):
            add(k, int(p), 100.0, 100.0, -1.0, 1)
    mp_bad = np.zeros(M, np.uint8)
    mp_bad[int(pr["edge_point"][7])] = 1                     # a bad point in the rows
    kf_bad = np.zeros(K, np.uint8)
    kf_bad[[bad_nb, bad_obs]] = 1
    t = synth.local_map_tables(kf_mappoint, kf_n, M, kf_bad=kf_bad, mp_bad=mp_bad)
    t = {k: t[k] for k in ("kf_bad", "kf_n", "kf_mappoint", "mp_bad", "mp_obs_off", "mp_obs_kf")}
    where = {(int(k), int(p)): i for k in range(K) for i, p in enumerate(kf_mappoint[k, :kf_n[k]])}
    owner = np.repeat(np.arange(M), np.diff(t["mp_obs_off"]))
    t["mp_obs_idx"] = np.array([where[(int(k), int(p))] for k, p in zip(t["mp_obs_kf"], owner)], np.int32)
    t["mp_nobs"] = np.array([sum(2 if uright[k, i] >= 0 else 1 for k, i in zip(t["mp_obs_kf"][a:b], t["mp_obs_idx"][a:b]))
                             for a, b in zip(t["mp_obs_off"][:-1], t["mp_obs_off"][1:])], np.int32)
    t["mp_ref_kf"] = np.array([t["mp_obs_kf"][a] if b > a else -1 for a, b in zip(t["mp_obs_off"][:-1], t["mp_obs_off"][1:])], np.int32)
    # an erased observation: a point with many observations loses one in a local keyframe (the cell is null)
    p = int(np.argmax(np.diff(t["mp_obs_off"]) * (mp_bad == 0)))
    e = int(t["mp_obs_off"][p]) + 1
    t["kf_mappoint"][t["mp_obs_kf"][e], t["mp_obs_idx"][e]] = -1
    t["mp_nobs"][p] -= 2 if uright[t["mp_obs_kf"][e], t["mp_obs_idx"][e]] >= 0 else 1
    t["mp_obs_kf"][e] = -1
    cur = n_kf - 1
    row = [k for k in range(n_kf - 2, -1, -1)]
    row.insert(2, bad_nb)
    assert len(row) <= CONN_CAP
    ord_slot = np.full((K, CONN_CAP), -1, np.int32)
    n_ord = np.zeros(K, np.int32)
    ord_slot[cur, :len(row)] = row
    n_ord[cur] = len(row)
    pose = np.zeros((K, 12), np.float32)
    pose[:P, :9], pose[:P, 9:] = pr["pose_R"], pr["pose_t"]
    pose[P:] = pose[0]
    cam = np.array([synth.KITTI[k] for k in ("fx", "fy", "cx", "cy", "bf")] + [synth.KITTI["bf"] / synth.KITTI["fx"]], np.float32)
    t.update(inv_sigma2=INV_SIGMA2, scale_factors=SCALE, kf_id=np.arange(K, dtype=np.int32), kf_keypoint=kp,
             kf_kp_octave=np.ascontiguousarray(kp["octave"], np.int32), kf_uright=uright, kf_camera=np.tile(cam, (K, 1)),
             kf_pose=pose, ord_slot=ord_slot, n_ord=n_ord, mp_xw=pr["points"].astype(np.float32),
             mp_normal=np.zeros((M, 3), np.float32), mp_max_min=np.zeros((M, 2), np.float32))
    for v in t.values():
        v.setflags(write=False)
    return t, cur


def dirty(name="small"):
    """(tables, cur) of `name` with entries outside their tables: neighbours outside the table and one met twice, row entries
    and an observer outside, a keypoint index past kf_cap and an octave past n_levels.  The device entries skip them; the host
    entries refuse such tables."""
    t0, cur = case(name)
    t = {k: np.array(v) for k, v in t0.items()}
    K, M = len(t["kf_n"]), len(t["mp_bad"])
    t["ord_slot"][cur, 1], t["ord_slot"][cur, 3] = K + 5, -7
    t["ord_slot"][cur, 4] = t["ord_slot"][cur, 0]
    t["kf_mappoint"][cur, 2], t["kf_mappoint"][0, 1] = M + 3, -9
    e = int(t["mp_obs_off"][int(t["kf_mappoint"][cur][t["kf_mappoint"][cur] >= 0][5])])
    t["mp_obs_kf"][e], t["mp_obs_idx"][e + 1] = K + 1, t["kf_mappoint"].shape[1] + 4
    t["kf_keypoint"][1, 3]["octave"] = 99
    return t, cur
