"""tests/loop_correct_ref.py pinned on hand-built maps (CPU): who claims a point, which centre an observer contributes,
the scale, prevNeighbors taken after the earlier updates, an overflowing row, and point_ref's three branches."""
import numpy as np

import essential_graph_ref as E
import loop_correct_ref as LR
import map_maintenance_cases as MC
import map_maintenance_ref as R

F32 = np.float32
SCALE = (1.2 ** np.arange(4)).astype(F32)


def hand_map(rows, K=5, kf_cap=6, conn_cap=6, seed=0):
    """rows: per keyframe the list of point slots (-1 = null) of kf_mappoint; a point's observers are the keyframes that
    list it, ascending."""
    rng = np.random.default_rng(seed)
    M = max(max(r) for r in rows if r) + 1
    kf_mappoint = np.full((K, kf_cap), -1, np.int32)
    kf_n = np.zeros(K, np.int32)
    for k, r in enumerate(rows):
        kf_mappoint[k, :len(r)], kf_n[k] = r, len(r)
    obs = [[(k, r.index(p)) for k, r in enumerate(rows) if p in r] for p in range(M)]
    pose = np.zeros((K, 12), F32)
    for k in range(K):
        pose[k, :9], pose[k, 9:] = MC.rotation(rng).reshape(-1), rng.normal(size=3) + (k, 0, 0)
    m = dict(kf_id=(np.arange(K) * 2 + 10).astype(np.int32), kf_n=kf_n, kf_mappoint=kf_mappoint, mp_bad=np.zeros(M, np.uint8),
             mp_obs_off=np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32),
             mp_obs_kf=np.array([k for o in obs for k, _ in o], np.int32), mp_obs_idx=np.array([i for o in obs for _, i in o], np.int32),
             mp_ref_kf=np.array([o[0][0] if o else -1 for o in obs], np.int32), mp_xw=(rng.normal(size=(M, 3)) * 3).astype(F32),
             kf_pose=pose, kf_kp_octave=rng.integers(0, 4, (K, kf_cap)).astype(np.int32), mp_normal=np.zeros((M, 3), F32),
             mp_max_min=np.ones((M, 2), F32), mp_corrected_by=np.zeros(M, np.int32), mp_corrected_ref=np.full(M, -1, np.int32))
    m.update(MC.empty_state(K, conn_cap))
    return m


def scw_of(m, cur, s):
    return np.concatenate([m["kf_pose"][cur, :9], m["kf_pose"][cur, 9:] * F32(s) + F32(0.25), [s]]).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_claims_and_point_ref():
    # point 0: listed by 1 and 3 (both connected); point 1 twice in keyframe 1's row; 2 bad; 3 carries kf_id[cur]; 4 only in
    # keyframe 4, which is not connected; 5 listed by 3 only
    m = hand_map([[4], [0, 1, -1, 1, 2], [3], [0, 5, 3], [4]])
    m["mp_bad"][2] = 1
    cur = 2
    m["mp_corrected_by"][3], m["mp_corrected_ref"][3] = m["kf_id"][cur], 4
    conn = np.array([3, 1, cur, -1], np.int32)
    out = LR.propagate(m, SCALE, cur, scw_of(m, cur, 1.7), conn)
    assert list(out["mp_corrected_ref"]) == [1, 1, -1, 4, -1, 3]                      # the lower slot; nobody for 2, 3 and 4
    assert list(out["mp_corrected_by"] == m["kf_id"][cur]) == [True, True, False, True, False, True]
    assert list(out["point_ref"]) == [1, 1, -1, 4, int(m["mp_ref_kf"][4]), 3]          # corrected, bad, carried, reference
    for p in (2, 3, 4):
        assert np.array_equal(bits(out["mp_xw"][p]), bits(m["mp_xw"][p]))
    # the point that sits twice in the row moved once
    corr = {k: E.f3(out["vertex_sim3"][k]) for k in (1, 3)}
    once = E.f3_map(E.f3_mul(E.f3_inverse(corr[1]), E.f3(out["edge_sim3"][1])), m["mp_xw"][1])
    assert np.array_equal(bits(out["mp_xw"][1]), bits(once))
    assert list(out["items"]) == [1, 2, 3, -1]
    # the poses: connected ones (R, t / s), the others untouched; the rows of the others are Sim3(pose)
    assert np.array_equal(bits(out["kf_pose"][[0, 4]]), bits(m["kf_pose"][[0, 4]]))
    assert np.array_equal(bits(out["vertex_sim3"][0, :12]), bits(m["kf_pose"][0])) and out["vertex_sim3"][0, 12] == 1
    assert np.array_equal(bits(out["vertex_sim3"][cur]), bits(scw_of(m, cur, 1.7)))
    assert np.array_equal(bits(out["edge_sim3"][:, :12]), bits(m["kf_pose"])) and (out["edge_sim3"][:, 12] == 1).all()


def test_the_centre_an_observer_contributes():
    # point 0 is claimed by 2 and observed by 1 (connected, lower: corrected centre), 3 (connected, higher: entry centre)
    # and 4 (not connected: entry centre); keyframe 0 is cur
    for s in (1.0, 1.7):
        m = hand_map([[1], [2, 0], [0], [0, 3], [0]])
        m["kf_mappoint"][1, 1] = -1                                                     # 1 observes 0 but does not list it
        cur = 0
        conn = np.array([1, 2, 3, cur], np.int32)
        out = LR.propagate(m, SCALE, cur, scw_of(m, cur, s), conn)
        assert out["mp_corrected_ref"][0] == 2
        centres = {1: R.center(out["kf_pose"][1]), 2: R.center(m["kf_pose"][2]), 3: R.center(m["kf_pose"][3]),
                   4: R.center(m["kf_pose"][4])}
        t = dict(m, mp_xw=out["mp_xw"], mp_normal=m["mp_normal"].copy(), mp_max_min=m["mp_max_min"].copy())
        LR.update_point(t, SCALE, 0, lambda o: centres[o])
        assert np.array_equal(bits(out["mp_normal"][0]), bits(t["mp_normal"][0]))
        assert np.array_equal(bits(out["mp_max_min"][0]), bits(t["mp_max_min"][0]))
        for swap in (1, 3):                                                            # the other centre gives other bits
            wrong = dict(centres)
            wrong[swap] = R.center((m if swap == 1 else out)["kf_pose"][swap])
            t2 = dict(t, mp_normal=m["mp_normal"].copy(), mp_max_min=m["mp_max_min"].copy())
            LR.update_point(t2, SCALE, 0, lambda o: wrong[o])
            assert not np.array_equal(bits(out["mp_normal"][0]), bits(t2["mp_normal"][0]))
        # SetPose: t / s in double, narrowed
        v = out["vertex_sim3"][2]
        assert np.array_equal(bits(out["kf_pose"][2, 9:]), bits([F32(np.float64(x) * (np.float64(1) / np.float64(v[12]))) for x in v[9:12]]))
        assert (s == 1.0) == np.array_equal(bits(out["kf_pose"][2, 9:]), bits(v[9:12]))


def graph_where_prev_changes():
    """Keyframes 0 and 1 are connected to cur; 2 is outside.  1 shares 16 points with 2 (a link its stale rows do not hold yet)
    and 3 with 0; 0's ordered row on entry is [1] only, but its connection row also holds 2 below the threshold.  When 1 is
    updated before 0, AddConnection(0 <- 1) rebuilds 0's ordered row from its whole connection row: 2 enters prev."""
    K, cap, kf_cap = 4, 4, 40
    rows = [[], [], [], []]
    p = 0
    for a, b, n in ((1, 2, 16), (0, 1, 20), (0, 2, 3)):
        for _ in range(n):
            rows[a].append(p); rows[b].append(p); p += 1
    m = hand_map(rows, K=K, kf_cap=kf_cap, conn_cap=cap)
    m["kf_first_connection"][:] = 0
    m["conn_slot"][0, :2], m["conn_weight"][0, :2], m["n_conn"][0] = (1, 2), (19, 3), 2     # 19: the weight with 1 is stale
    m["ord_slot"][0, :1], m["ord_weight"][0, :1], m["n_ord"][0] = 1, 19, 1
    m["conn_slot"][1, :1], m["conn_weight"][1, :1], m["n_conn"][1] = 0, 19, 1
    m["ord_slot"][1, :1], m["ord_weight"][1, :1], m["n_ord"][1] = 0, 19, 1
    return m


def test_prev_is_taken_after_the_earlier_updates():
    m = graph_where_prev_changes()
    conn = np.array([1, 0, 3], np.int32)                                  # list order: 1 before 0; 3 is cur (no points)
    state, got = LR.loop_connections(m, conn)
    _, entry = LR.loop_connections(m, conn, entry_snapshot=True)
    sets = lambda r: {int(k): list(r["conn_slot"][r["conn_begin"][i]:r["conn_begin"][i + 1]]) for i, k in enumerate(r["conn_kf"])}  # noqa: E731
    assert list(got["conn_kf"]) == [0, 1, 3]                               # ascending slot, empty sets kept
    assert sets(got) == {0: [], 1: [2], 3: []}
    assert sets(entry)[0] == [2]                                           # the entry-state snapshot gives another set
    assert (state["status"] == 0).all() and got["n_connections"] == 3


def test_an_overflowing_row_keeps_its_rows_and_its_set_comes_from_them():
    m = graph_where_prev_changes()
    narrow = dict(m)
    for k in R.STATE_KEYS[:6]:
        if m[k].ndim == 2:
            narrow[k] = m[k][:, :1].copy()
    narrow["n_conn"], narrow["n_ord"] = np.minimum(m["n_conn"], 1), np.minimum(m["n_ord"], 1)
    state, got = LR.loop_connections(narrow, np.array([1, 3], np.int32))
    assert state["status"][1] == R.CONN_OVERFLOW                           # 1 would hold 0 and 2
    assert list(state["conn_slot"][1]) == [0] and got["n_connections"] == 2 and got["conn_begin"][-1] == 0


def test_the_connected_list():
    m = graph_where_prev_changes()
    m["ord_slot"][0, :3], m["n_ord"][0] = (2, 9, 1), 3
    lst, n = LR.connected(m, 0)
    assert list(lst) == [2, 1, 0, -1, -1] and n == 3
