"""Shared generators for the map-maintenance tests (tests/test_map_maintenance_*.py).

make_map(seed, ...)  a slot-table map: keyframes on a line, every point observed by 2 to max_obs keyframes around a centre
                     (so close keyframes share many points, far ones a few: counts on both sides of the threshold) plus the
                     odd far observer, the observations of a point in shuffled (not ascending) order, the last keyframe
                     holding only a dozen points (the maximum fallback).  The connection state is what UpdateConnections of
                     three quarters of the keyframes leaves on an earlier map, one third of whose points did not exist yet.
dirty(map)           the same map with slots and indices outside their tables written over some entries.
case(name)           "clean" and "dirty", computed once; treat as read-only (graph() / points() copy what a call updates).
"""
import functools

import numpy as np

import map_maintenance_ref as R

K, KF_CAP, M, CONN_CAP, N_LEVELS = 24, 256, 1500, 24, 8
SCALE = (1.2 ** np.arange(N_LEVELS)).astype(np.float32)
GRAPH = ("kf_id", "kf_n", "kf_mappoint", "mp_bad", "mp_obs_off", "mp_obs_kf") + R.STATE_KEYS
POINTS = ("mp_bad", "mp_xw", "mp_ref_kf", "mp_obs_off", "mp_obs_kf", "mp_obs_idx", "kf_pose", "kf_n", "kf_kp_octave",
          "mp_normal", "mp_max_min")


def empty_state(n_kf, conn_cap):
    return dict(conn_slot=np.full((n_kf, conn_cap), -1, np.int32), conn_weight=np.zeros((n_kf, conn_cap), np.int32),
                n_conn=np.zeros(n_kf, np.int32), ord_slot=np.full((n_kf, conn_cap), -1, np.int32),
                ord_weight=np.zeros((n_kf, conn_cap), np.int32), n_ord=np.zeros(n_kf, np.int32),
                kf_first_connection=np.ones(n_kf, np.uint8), kf_parent=np.full(n_kf, -1, np.int32),
                kf_covis=np.full((n_kf, R.COVIS), -1, np.int32))


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_map(seed=0, n_kf=K, kf_cap=KF_CAP, n_mp=M, conn_cap=CONN_CAP, max_obs=7, warm=True):
    rng = np.random.default_rng(seed)
    kf_mappoint = np.full((n_kf, kf_cap), -1, np.int32)
    kf_n = np.zeros(n_kf, np.int32)
    off, obs_kf, obs_idx = [0], [], []
    ref = np.full(n_mp, -1, np.int32)
    last_room = 12                                     # the last keyframe's few points
    for p in range(n_mp):
        want = int(rng.integers(2, max_obs + 1))
        c = int(rng.integers(0, n_kf - 1))
        near = [k for k in sorted(range(n_kf - 1), key=lambda k: (abs(k - c), k))[:want]]
        for _ in range(int(rng.integers(0, 3))):          # the odd far observers
            near.append(int(rng.integers(0, n_kf - 1)))
        if last_room and c >= n_kf - 4:
            near.append(n_kf - 1)
            last_room -= 1
        kfs = [k for k in dict.fromkeys(near) if kf_n[k] < kf_cap]
        rng.shuffle(kfs)
        for k in kfs:
            obs_kf.append(k)
            obs_idx.append(int(kf_n[k]))
            kf_mappoint[k, kf_n[k]] = p
            kf_n[k] += 1
        off.append(len(obs_kf))
        if kfs:
            ref[p] = kfs[0] if rng.random() < 0.9 else int(rng.integers(0, n_kf))   # some references do not observe
    mp_bad = (rng.random(n_mp) < 0.05).astype(np.uint8)
    pose = np.zeros((n_kf, 12), np.float32)
    for k in range(n_kf):
        pose[k, :9] = rotation(rng).reshape(-1)
        pose[k, 9:] = rng.normal(size=3) * 2 + (0.3 * k, 0, 0)
    m = dict(kf_id=(np.arange(n_kf) * 3).astype(np.int32), kf_n=kf_n, kf_mappoint=kf_mappoint, mp_bad=mp_bad,
             mp_obs_off=np.array(off, np.int32), mp_obs_kf=np.array(obs_kf, np.int32), mp_obs_idx=np.array(obs_idx, np.int32),
             mp_ref_kf=ref, mp_xw=(rng.normal(size=(n_mp, 3)) * 4).astype(np.float32), kf_pose=pose,
             kf_kp_octave=rng.integers(0, N_LEVELS, (n_kf, kf_cap)).astype(np.int32),
             mp_normal=rng.normal(size=(n_mp, 3)).astype(np.float32), mp_max_min=rng.random((n_mp, 2)).astype(np.float32) + 1)
    m.update(empty_state(n_kf, conn_cap))
    if warm:                                           # the state an earlier map left
        early = dict(m, mp_bad=(mp_bad | (np.arange(n_mp) % 3 == 0)).astype(np.uint8))
        out = R.update_connections(early, [k for k in range(n_kf) if k % 4 != 1])   # the others never ran: first connection
        assert (out["status"] == 0).all()
        m.update({k: out[k] for k in R.STATE_KEYS})
    return m


def dirty(m):
    """Entries outside their tables: the device skips them; the host entries refuse them."""
    m = {k: v.copy() for k, v in m.items()}
    n_kf, n_mp = len(m["kf_n"]), len(m["mp_bad"])
    m["kf_mappoint"][1, 3], m["kf_mappoint"][2, 0], m["kf_mappoint"][5, 7] = n_mp + 5, -7, n_mp
    m["mp_obs_kf"][[4, 90, 301]] = n_kf + 3, -2, n_kf
    m["mp_ref_kf"][[10, 11, 12]] = n_kf + 1, -3, n_kf
    m["mp_obs_idx"][[7, 8]] = KF_CAP + 1, -4
    m["kf_kp_octave"][3, :5] = N_LEVELS, -1, 40, N_LEVELS, -2
    return m


@functools.lru_cache(maxsize=None)
def case(name):
    m = make_map(0)
    return dirty(m) if name == "dirty" else m


def graph(m, conn_cap=None):
    g = {k: m[k].copy() for k in GRAPH}
    if conn_cap is not None:                           # the same rows at another capacity (they must fit)
        assert (g["n_conn"] <= conn_cap).all()
        for k in R.STATE_KEYS[:6]:
            if g[k].ndim == 2:
                a = np.full((g[k].shape[0], conn_cap), -1 if k.endswith("slot") else 0, np.int32)
                w = min(conn_cap, g[k].shape[1])
                a[:, :w] = g[k][:, :w]
                g[k] = a
    return g


def points(m):
    return {k: m[k].copy() for k in POINTS}


@functools.lru_cache(maxsize=None)
def expected_connections(name, items, conn_cap=None):
    """The restatement's result for a batch (a tuple of slots): computed once, shared, left unchanged."""
    return R.update_connections(graph(case(name), conn_cap), list(items))


@functools.lru_cache(maxsize=None)
def expected_normals(name, pts=None):
    return R.update_normal_depth(points(case(name)), SCALE, None if pts is None else list(pts))


BATCHES = {"one": (7,), "five": (3, 13, 4, 23, 0), "all": tuple(range(K)), "repeat": (5, 9, 5, 2, 9, 5)}
