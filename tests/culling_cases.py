"""Shared generator for the culling tests (tests/test_culling_*.py), on top of map_maintenance_cases.make_map (K = 24,
kf_cap = 256, M = 1500).

make_case()  that map with the tables the culls read derived consistently: no bad point keeps observations, mp_nobs from the
             observations and kf_uright, depths on both sides of TH_DEPTH, the connection state of UpdateConnections of
             every keyframe.  A few keyframes (HOT) have their octaves raised to the top level and most of their thinly
             observed points taken out of their rows, so that they are redundant or nearly so; kf_parent around them is set
             so that the tree loop has chains to follow.
dirty(case)  the same with slots and indices outside their tables written over some entries.
case(name)   "clean" and "dirty", computed once; treat as read-only (tables() copies).
At import the module asserts, on the restatement alone, that the clean case reaches every path the tests are about."""
import functools

import numpy as np

import culling_ref as CR
import map_maintenance_cases as MC
import map_maintenance_ref as MR

K, KF_CAP, M, CONN_CAP = MC.K, MC.KF_CAP, MC.M, MC.CONN_CAP
TH_DEPTH = np.float32(3.5)
MAX_OBS = 11                              # observers of a point: thick enough for a redundant keyframe to stay so after a cull or two
CUR, CUR_KF_ID, MONOCULAR = 12, 36, False
HOT = (10, 11, 13, 14, 15, 9)             # made redundant, more or less
KEEP_THIN = {10: 0.02, 11: 0.0, 13: 0.12, 14: 0.05, 15: 0.0, 9: 0.04}   # share of a hot keyframe's thin points left in its row
NOT_ERASE = 15
TABLES = ("kf_id", "kf_n", "kf_mappoint", "kf_kp_octave", "kf_uright", "kf_depth", "kf_pose", "kf_bad", "kf_not_erase",
          "kf_to_be_erased", "kf_tcp", "mp_bad", "mp_nobs", "mp_found", "mp_visible", "mp_first_kf_id", "mp_ref_kf", "mp_obs_off",
          "mp_obs_kf", "mp_obs_idx", "conn_slot", "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord", "kf_parent",
          "kf_covis")


def make_case(seed=0):
    m = MC.make_map(seed, warm=False, max_obs=MAX_OBS)
    rng = np.random.default_rng(1000 + seed)
    obs = [[(int(m["mp_obs_kf"][e]), int(m["mp_obs_idx"][e])) for e in range(m["mp_obs_off"][p], m["mp_obs_off"][p + 1])]
           for p in range(M)]
    m["kf_kp_octave"] = rng.integers(0, 5, (K, KF_CAP)).astype(np.int32)
    for p in np.flatnonzero(m["mp_bad"]):                    # a bad point has left the rows
        for k, i in obs[p]:
            m["kf_mappoint"][k, i] = -1
        obs[p] = []
    for t in HOT:
        m["kf_kp_octave"][t] = MC.N_LEVELS - 1
        for i in range(m["kf_n"][t]):
            p = int(m["kf_mappoint"][t, i])
            if p >= 0 and len(obs[p]) < 4 and rng.random() >= KEEP_THIN[t]:
                m["kf_mappoint"][t, i] = -1
                obs[p] = [(k, j) for k, j in obs[p] if k != t]
    m["mp_obs_off"] = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32)
    m["mp_obs_kf"] = np.array([k for o in obs for k, _ in o], np.int32)
    m["mp_obs_idx"] = np.array([i for o in obs for _, i in o], np.int32)
    for p in range(M):
        if m["mp_ref_kf"][p] not in [k for k, _ in obs[p]] and rng.random() < 0.8:
            m["mp_ref_kf"][p] = obs[p][0][0] if obs[p] else -1
    m["kf_uright"] = np.where(rng.random((K, KF_CAP)) < 0.5, rng.random((K, KF_CAP)) * 600, -1).astype(np.float32)
    m["kf_depth"] = (rng.random((K, KF_CAP)) * 4).astype(np.float32)          # one in eight beyond TH_DEPTH
    m["kf_depth"][rng.random((K, KF_CAP)) < 0.05] = -1
    m["mp_nobs"] = np.array([sum(2 if m["kf_uright"][k, i] >= 0 else 1 for k, i in o) for o in obs], np.int32)
    m["mp_visible"] = rng.integers(0, 40, M).astype(np.int32)
    m["mp_found"] = np.minimum(rng.integers(0, 40, M), m["mp_visible"] + (rng.random(M) < 0.05)).astype(np.int32)
    m["mp_first_kf_id"] = (CUR_KF_ID - rng.integers(0, 5, M)).astype(np.int32)
    m["kf_bad"], m["kf_to_be_erased"] = np.zeros(K, np.uint8), np.zeros(K, np.uint8)
    m["kf_not_erase"] = np.zeros(K, np.uint8)
    m["kf_not_erase"][NOT_ERASE] = 1
    m["kf_tcp"] = rng.normal(size=(K, 12)).astype(np.float32)
    out = MR.update_connections({k: m[k] for k in MC.GRAPH}, list(range(K)))
    assert (out["status"] == 0).all()
    m.update({k: out[k] for k in MR.STATE_KEYS})
    # the tree: a chain, but 11 (under 10) has 12, 13, 14 and the last keyframe as children; the last one's links to the
    # keyframes below 18 are taken out of both rows, so nobody around 11 adopts it
    m["kf_parent"] = np.arange(-1, K - 1).astype(np.int32)
    m["kf_parent"][[13, 14, K - 1]] = 11
    G = CR.Connections(m, K)
    for k in range(18):
        G.write(k, {s: w for s, w in G.conn(k).items() if s != K - 1})
    G.write(K - 1, {s: w for s, w in G.conn(K - 1).items() if s >= 18})
    return {k: m[k] for k in TABLES}


def dirty(c):
    """Entries outside their tables: the device skips them; the host entries refuse them."""
    c = {k: v.copy() for k, v in c.items()}
    c["kf_mappoint"][1, 3], c["kf_mappoint"][10, 0], c["kf_mappoint"][13, 7] = M + 5, -7, M
    c["mp_obs_kf"][[4, 90, 301, 2000]] = K + 3, -2, K, 2 ** 30
    c["mp_ref_kf"][[10, 11, 12]] = K + 1, -3, K
    c["mp_obs_idx"][[7, 8, 2500, 2501]] = KF_CAP + 1, -4, KF_CAP, -(2 ** 31)
    c["kf_kp_octave"][3, :5] = MC.N_LEVELS, -1, 40, MC.N_LEVELS, -2
    c["conn_slot"][11, 2], c["conn_slot"][9, 0] = K, -3
    c["ord_slot"][CUR, 1], c["ord_slot"][7, 0] = K + 9, -2
    c["kf_parent"][[2, 3]] = K, -9
    c["mp_obs_off"][M] += 7                              # past the arrays
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    c = make_case(0)
    return dirty(c) if name == "dirty" else c


def tables(c):
    return {k: v.copy() for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def recent(name):
    rng = np.random.default_rng(7)
    r = rng.permutation(M)[:400].astype(np.int32)
    if name == "dirty":
        r[[3, 77, 200]] = M, -1, 2 ** 30
    return r


@functools.lru_cache(maxsize=None)
def expected_points(name):
    """The restatement's MapPointCulling: computed once, shared, left unchanged."""
    return CR.map_point_culling(case(name), recent(name), CUR_KF_ID, MONOCULAR)


@functools.lru_cache(maxsize=None)
def expected_keyframes(name):
    return CR.keyframe_culling(case(name), CUR, MONOCULAR, TH_DEPTH)


def _check():
    c = case("clean")
    out, culled, n, trace = expected_keyframes("clean")
    targets = [int(s) for s in c["ord_slot"][CUR, :c["n_ord"][CUR]]]
    assert n >= 3, n
    # a later target decided otherwise than the entry state alone would
    entry = CR.Map(c)
    differs = [k for ev, k, *cnt in [e for e in trace if e[0] == "counted"]
               if (cnt[1] > 0.9 * cnt[0]) != (lambda a: a[1] > 0.9 * a[0])(CR.redundancy(entry, k, MONOCULAR, TH_DEPTH))]
    assert differs, [e for e in trace if e[0] == "counted"]
    # a point that went bad through erasure cleared an entry of a target not yet visited
    visited, late = [], False
    for e in trace:
        if e[0] == "counted":
            visited.append(e[1])
        if e[0] == "cleared" and e[2] in targets and e[2] not in visited and any(x[0] == "erased_bad" and x[1] == e[1] for x in trace):
            late = True
    assert late
    assert any(e[0] == "adopted" and e[3] for e in trace), [e for e in trace if e[0] in ("adopted", "fell_back")]
    assert any(e[0] == "fell_back" for e in trace)
    assert ("held", NOT_ERASE) in trace and out["kf_to_be_erased"][NOT_ERASE] == 1 and not out["kf_bad"][NOT_ERASE]
    branch = expected_points("clean")[2]
    assert {"bad", "ratio", "few", "old", "kept"} <= set(branch), set(branch)


_check()
