"""Shared maps for the loop-correction tests (tests/test_loop_correct_*.py), built on tests/map_maintenance_cases.py.

case("small")       K = 12, about 200 points, conn_cap 16; cur = 6 has connected keyframes below and above it (7 connected
                    after UpdateConnections(cur)); a few points carry kf_id[cur] on entry.
case("wide")        K = 80 with 72 connected keyframes (cur's rows are planted) and about 900 claimed points: more connected
                    keyframes than a wavefront has lanes, more points than a workgroup holds; the scale of Scw is 1.7.
case("chain")       the small map with every point's observations ascending in keyframe slot and SLACK free entries behind
                    them, three holes in cur's row and the tables of orbmm_observe (OBSERVE): the map the whole chain with
                    the matched points' fuse_apply runs on.  matched() is that list: loop-side points (seen by no connected
                    keyframe) for the holes (AddObservation) and for occupied keypoints of cur (Replace).
case("dirty")       the small map with slots and indices outside their tables (map_maintenance_cases.dirty) and, in
                    case("dirty_rows"), also in cur's ordered row: for the device entries only.
Computed once; treat as read-only (tables() copies).  expected_*() are the restatement's results, shared and left unchanged."""
import functools

import numpy as np

import loop_correct_ref as LR
import observe_ref as OR
import map_maintenance_cases as MC
import map_maintenance_ref as R

SCALE = MC.SCALE
WIDE_OUTSIDE = (3, 17, 29, 44, 58, 66, 73, 79)      # the wide map's keyframes that are not connected to cur
CUR = {"small": 6, "wide": 40, "dirty": 6, "dirty_rows": 6, "chain": 6}
SLACK, HOLES = 8, (2, 9, 17)                        # free entries per observation row; the keypoints of cur left null
OBSERVE = ("kf_uright", "mp_nobs", "mp_found", "mp_visible", "mp_replaced")
KEYS = MC.GRAPH + tuple(k for k in MC.POINTS if k not in MC.GRAPH) + ("mp_corrected_by", "mp_corrected_ref")


def scw(name, s=None):
    """Scw: the pose of cur moved by a small rotation and a shift, at scale s."""
    m = case(name)
    rng = np.random.default_rng(11)
    s = (1.7 if name == "wide" else 1.0) if s is None else s
    a = rng.normal(size=3) * 0.03
    dR = np.array([[1, -a[2], a[1]], [a[2], 1, -a[0]], [-a[1], a[0], 1]])
    u, _, vt = np.linalg.svd(dR)
    pose = m["kf_pose"][CUR[name]].astype(np.float64)
    Rm = (u @ vt) @ pose[:9].reshape(3, 3)
    return np.concatenate([Rm.reshape(-1), s * pose[9:] + rng.normal(size=3) * 0.2, [s]]).astype(np.float32)


def with_corrected(m, cur, seed):
    rng = np.random.default_rng(seed)
    M = len(m["mp_bad"])
    by = np.zeros(M, np.int32)
    ref = np.full(M, -1, np.int32)
    carried = rng.choice(M, max(M // 25, 3), replace=False)           # corrected by an earlier loop of the same keyframe
    by[carried] = m["kf_id"][cur]
    ref[carried] = rng.integers(0, len(m["kf_n"]), len(carried))
    other = rng.choice(M, max(M // 25, 3), replace=False)             # and by another keyframe's loop
    other = other[by[other] == 0]
    by[other] = m["kf_id"][cur] + 1
    ref[other] = rng.integers(0, len(m["kf_n"]), len(other))
    return dict(m, mp_corrected_by=by, mp_corrected_ref=ref)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "small":
        return with_corrected(MC.make_map(6, n_kf=12, kf_cap=128, n_mp=200, conn_cap=16, max_obs=4), CUR[name], 1)
    if name == "wide":
        m = MC.make_map(5, n_kf=80, kf_cap=96, n_mp=900, conn_cap=80)
        cur = CUR[name]
        others = [k for k in range(80) if k != cur and k not in WIDE_OUTSIDE]
        n = len(others)
        m["conn_slot"][cur], m["conn_weight"][cur], m["ord_slot"][cur], m["ord_weight"][cur] = -1, 0, -1, 0
        m["conn_slot"][cur, :n], m["conn_weight"][cur, :n], m["n_conn"][cur] = others, 20, n
        m["ord_slot"][cur, :n], m["ord_weight"][cur, :n], m["n_ord"][cur] = others[::-1], 20, n
        return with_corrected(m, cur, 2)
    if name == "chain":
        return chain_map(case("small"), CUR[name])
    m = MC.dirty(case("small"))
    m["mp_corrected_ref"][np.flatnonzero(m["mp_corrected_by"] != 0)[:2]] = 99, -5     # slots outside the table
    if name == "dirty_rows":
        cur = CUR[name]
        out = R.update_connections(m, [cur])
        m.update({k: out[k] for k in R.STATE_KEYS})
        n = int(m["n_ord"][cur])
        m["ord_slot"][cur, 1], m["ord_slot"][cur, n - 1] = len(m["kf_n"]) + 3, -2
    return m


def chain_map(small, cur):
    m = {k: v.copy() for k, v in small.items()}
    K, M = len(m["kf_n"]), len(m["mp_bad"])
    rng = np.random.default_rng(21)
    rows = []
    for p in range(M):
        e0, e1 = m["mp_obs_off"][p], m["mp_obs_off"][p + 1]
        row = sorted(zip(m["mp_obs_kf"][e0:e1].tolist(), m["mp_obs_idx"][e0:e1].tolist()))
        rows.append([(k, i) for k, i in row if not (k == cur and i in HOLES)])
    for i in HOLES:
        assert i < m["kf_n"][cur] and m["kf_mappoint"][cur, i] >= 0
        m["kf_mappoint"][cur, i] = -1
    m["mp_obs_off"] = np.concatenate([[0], np.cumsum([len(r) + SLACK for r in rows])]).astype(np.int32)
    flat = [e for r in rows for e in r + [(-1, -1)] * SLACK]
    m["mp_obs_kf"], m["mp_obs_idx"] = np.array([e[0] for e in flat], np.int32), np.array([e[1] for e in flat], np.int32)
    m.update(kf_uright=np.full(m["kf_mappoint"].shape, -1, np.float32), mp_nobs=np.array([len(r) for r in rows], np.int32),
             mp_found=rng.integers(1, 30, M).astype(np.int32), mp_visible=rng.integers(30, 60, M).astype(np.int32),
             mp_replaced=np.full(M, -1, np.int32))
    return m


@functools.lru_cache(maxsize=None)
def matched():
    """CorrectLoop's matchedPoints as orbmm_apply's list (one item, cur): (item_kf, mp_begin, point, best_idx)."""
    m, cur = case("chain"), CUR["chain"]
    conn, n = expected_connected("chain")
    near = set(int(k) for k in conn[:n])
    loop_side = [p for p in range(len(m["mp_bad"])) if not m["mp_bad"][p] and m["mp_corrected_by"][p] == 0 and
                 (obs := R.observations(m, p)) and not near & {k for k, _ in obs}]
    occupied = [i for i in range(int(m["kf_n"][cur])) if m["kf_mappoint"][cur, i] >= 0][3:20:4]
    idx = list(HOLES) + occupied
    assert len(loop_side) >= len(idx) and len(occupied) == 5
    return (np.array([cur], np.int32), np.array([0, len(idx)], np.int32), np.array(loop_side[:len(idx)], np.int32),
            np.array(idx, np.int32))


def tables(m):
    return {k: m[k].copy() for k in KEYS + tuple(k for k in OBSERVE if k in m)}


def after_update(name):
    """The map after UpdateConnections(cur) (:547), as CorrectLoop sees it."""
    m = tables(case(name))
    if name in ("small", "dirty", "chain"):                        # the rows of cur of the other maps are planted
        out = R.update_connections(m, [CUR[name]])
        m.update({k: out[k] for k in R.STATE_KEYS})
    return m


@functools.lru_cache(maxsize=None)
def expected_connected(name):
    return LR.connected(after_update(name), CUR[name])


@functools.lru_cache(maxsize=None)
def expected_propagate(name, s=None):
    conn, _ = expected_connected(name)
    return LR.propagate(after_update(name), SCALE, CUR[name], scw(name, s), conn)


@functools.lru_cache(maxsize=None)
def expected_after_propagate(name):
    """The whole map behind propagate and UpdateConnections of the connected keyframes in ascending slot order (:612)."""
    m = after_update(name)
    out = expected_propagate(name)
    m.update({k: out[k] for k in LR.UPDATED})
    upd = R.update_connections(m, [int(k) for k in out["items"] if k >= 0])
    m.update({k: upd[k] for k in R.STATE_KEYS})
    return m, upd["status"]


@functools.lru_cache(maxsize=None)
def expected_loop_connections(name):
    m, _ = expected_after_propagate(name)
    conn, _ = expected_connected(name)
    return LR.loop_connections(m, conn)


@functools.lru_cache(maxsize=None)
def expected_chain():
    """The chain map behind :547-634 and :661-676: (the map after the matched points' walk, fuse_apply's result, the state
    and the sets of loop_connections)."""
    m, _ = expected_after_propagate("chain")
    fused = OR.fuse_apply(m, OR.LOOP_MATCHED, *matched())
    assert fused["status"] == OR.OK
    m = dict(m, **{k: fused[k] for k in OR.UPDATED})
    state, sets = LR.loop_connections(m, expected_connected("chain")[0])
    return m, fused, state, sets
