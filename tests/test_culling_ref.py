"""tests/culling_ref.py pinned on hand-built maps of a few keyframes whose answers are worked out by hand: every branch of
MapPointCulling, both sides of every gate of KeyFrameCulling's count, and the bookkeeping of a cull (rows, observations,
reference keyframes, the spanning tree).  CPU only."""
import numpy as np

import culling_ref as CR

TH = np.float32(3.0)


def build(K, rows, conn=None, parent=None, kf_cap=None, order=None):
    """A consistent map: rows[k] lists the points of keyframe k (index = keypoint); a point's observations are its keyframes
    ascending (or in order[p]); monocular keypoints at octave 0 and depth 1; conn[k] = {slot: weight}."""
    M = max([p for r in rows.values() for p in r if p >= 0] + [0]) + 1
    kf_cap = kf_cap or max(len(r) for r in rows.values())
    t = dict(kf_id=np.arange(1, K + 1).astype(np.int32), kf_n=np.zeros(K, np.int32), kf_mappoint=np.full((K, kf_cap), -1, np.int32),
             kf_kp_octave=np.zeros((K, kf_cap), np.int32), kf_uright=np.full((K, kf_cap), -1, np.float32),
             kf_depth=np.ones((K, kf_cap), np.float32), kf_pose=np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (K, 1)),
             kf_bad=np.zeros(K, np.uint8), kf_not_erase=np.zeros(K, np.uint8), kf_to_be_erased=np.zeros(K, np.uint8),
             kf_tcp=np.zeros((K, 12), np.float32), mp_bad=np.zeros(M, np.uint8), mp_found=np.ones(M, np.int32),
             mp_visible=np.ones(M, np.int32), mp_first_kf_id=np.zeros(M, np.int32), mp_ref_kf=np.full(M, -1, np.int32),
             conn_slot=np.full((K, K), -1, np.int32), conn_weight=np.zeros((K, K), np.int32), n_conn=np.zeros(K, np.int32),
             ord_slot=np.full((K, K), -1, np.int32), ord_weight=np.zeros((K, K), np.int32), n_ord=np.zeros(K, np.int32),
             kf_parent=np.array(parent if parent is not None else [-1] + [0] * (K - 1), np.int32),
             kf_covis=np.full((K, CR.COVIS), -1, np.int32))
    obs = [[] for _ in range(M)]
    for k in sorted(rows):
        t["kf_n"][k] = len(rows[k])
        for i, p in enumerate(rows[k]):
            t["kf_mappoint"][k, i] = p
            if p >= 0:
                obs[p].append((k, i))
    for p, ks in (order or {}).items():
        obs[p] = sorted(obs[p], key=lambda o: ks.index(o[0]))
    t["mp_obs_off"] = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32)
    t["mp_obs_kf"] = np.array([k for o in obs for k, _ in o], np.int32)
    t["mp_obs_idx"] = np.array([i for o in obs for _, i in o], np.int32)
    t["mp_nobs"] = np.array([len(o) for o in obs], np.int32)
    t["mp_ref_kf"] = np.array([o[0][0] if o else -1 for o in obs], np.int32)
    G = CR.Connections(t, K)
    for k, c in (conn or {}).items():
        G.write(k, c)
    return t


def observers(t, p):
    return [int(k) for k in t["mp_obs_kf"][t["mp_obs_off"][p]:t["mp_obs_off"][p + 1]]]


def test_map_point_culling_takes_each_branch():
    # points 0 .. 7, all seen by keyframes 0, 1, 2 (mp_nobs 3), point 6 also by keyframe 3
    t = build(4, {0: list(range(8)), 1: list(range(8)), 2: list(range(8)), 3: [6]})
    t["mp_bad"][0] = 1                                     # bad: dropped, nothing else
    t["mp_found"][1], t["mp_visible"][1] = 1, 5            # 0.2 < 0.25: SetBadFlag
    t["mp_found"][2], t["mp_visible"][2] = 1, 4            # 0.25 is not below 0.25 ...
    t["mp_first_kf_id"][2] = 8                             # ... and two keyframes old with 3 observations: SetBadFlag
    t["mp_found"][3], t["mp_visible"][3] = 3, 0            # inf: not below; young: kept
    t["mp_first_kf_id"][3] = 9
    t["mp_found"][4], t["mp_visible"][4] = 0, 0            # nan: not below; one keyframe old: kept
    t["mp_first_kf_id"][4] = 9
    t["mp_first_kf_id"][5] = 9                             # kept
    t["mp_first_kf_id"][6] = 7                             # 4 observations, three keyframes old: dropped, not bad
    t["mp_first_kf_id"][7] = 8                             # 3 observations: bad when stereo, 3 > 2 and young enough when monocular
    out, kept, branch = CR.map_point_culling(t, [0, 1, 2, 3, 4, 5, 6, 7, 8, -1], 10, monocular=False)
    assert branch == ["bad", "ratio", "few", "kept", "kept", "kept", "old", "few", "outside", "outside"]
    assert kept.tolist() == [3, 4, 5] and out["mp_bad"].tolist() == [1, 1, 1, 0, 0, 0, 0, 1]
    for p in (1, 2, 7):
        assert (out["kf_mappoint"][:3, p] == -1).all() and observers(dict(t, **out), p) == [-1, -1, -1]
    assert (out["kf_mappoint"][:3, 0] == 0).all() and observers(dict(t, **out), 0) == [0, 1, 2]   # it was bad already: untouched
    assert np.isin(out["kf_mappoint"], [3, 4, 5, 6]).sum() == 13   # dropped or kept: still in their rows
    out, kept, branch = CR.map_point_culling(t, [7, 6, 2], 10, monocular=True)
    assert branch == ["kept", "old", "kept"] and kept.tolist() == [7, 2] and out["mp_bad"].sum() == 1   # 3 > 2, two keyframes old
    t["mp_nobs"][7] = 2
    assert CR.map_point_culling(t, [7], 10, monocular=True)[2] == ["few"]


def redundant_map(n_points, n_redundant):
    """Keyframe 1 holds n_points points; the first n_redundant are also seen by keyframes 2, 3, 4, the others by 2 and 3."""
    rows = {0: [], 1: list(range(n_points)), 2: list(range(n_points)), 3: list(range(n_points)), 4: list(range(n_redundant))}
    conn = {0: {1: 20}, 1: {0: 20}}
    return build(5, rows, conn)


def test_the_ninety_percent_rule_is_strict():
    t = redundant_map(10, 9)
    assert CR.redundancy(CR.Map(t), 1, True, TH) == (10, 9)
    out, culled, n, _ = CR.keyframe_culling(t, 0, True, TH)
    assert n == 0 and not out["kf_bad"].any() and (culled == -1).all()          # 9 > 0.9 * 10 is false
    t = redundant_map(10, 10)
    out, culled, n, _ = CR.keyframe_culling(t, 0, True, TH)
    assert n == 1 and culled[0] == 1 and out["kf_bad"].tolist() == [0, 1, 0, 0, 0]
    t = redundant_map(20, 19)
    assert CR.keyframe_culling(t, 0, True, TH)[2] == 1 and CR.keyframe_culling(redundant_map(20, 18), 0, True, TH)[2] == 0


def test_the_observation_gate_counts_stereo_twice():
    # point 0: target + two others, monocular: 3 observations, gate closed.  point 1: the same, but the target's keypoint is
    # stereo: 4 > 3 opens the gate, yet only two others observe it.  point 2: target + three others: redundant.
    t = build(5, {0: [], 1: [0, 1, 2], 2: [0, 1, 2], 3: [0, 1, 2], 4: [-1, -1, 2]})
    t["kf_uright"][1, 1] = 5
    t["mp_nobs"][1] = 4
    m = CR.Map(t)
    assert CR.redundancy(m, 1, True, TH) == (3, 1)
    t["mp_nobs"][2] = 3                                    # the gate, not the observations, decides
    assert CR.redundancy(CR.Map(t), 1, True, TH) == (3, 0)
    m = CR.Map(t)
    m.erase_observation(1, 1)                              # stereo: 4 - 2 = 2 -> bad
    m.erase_observation(0, 1)                              # monocular: 3 - 1 = 2 -> bad
    assert m.t["mp_nobs"][:2].tolist() == [2, 2] and m.t["mp_bad"].tolist() == [1, 1, 0]
    assert (m.t["kf_mappoint"][2:4, :2] == -1).all() and (m.t["kf_mappoint"][1, :2] == [0, 1]).all()   # the target's row stays


def test_the_octave_gate_is_at_target_plus_one():
    t = build(5, {0: [], 1: [0], 2: [0], 3: [0], 4: [0]})
    t["kf_kp_octave"][1, 0] = 2
    t["kf_kp_octave"][[2, 3, 4], 0] = 3, 3, 0
    assert CR.redundancy(CR.Map(t), 1, True, TH) == (1, 1)
    t["kf_kp_octave"][3, 0] = 4                            # target + 2: not counted, two are left
    assert CR.redundancy(CR.Map(t), 1, True, TH) == (1, 0)


def test_the_depth_gate_only_without_monocular():
    t = build(5, {0: [], 1: [0, 1, 2, 3], 2: [0, 1, 2, 3], 3: [0, 1, 2, 3], 4: [0, 1, 2, 3]})
    t["kf_depth"][1] = TH, np.nextafter(TH, np.float32(10)), -0.5, 0.0
    assert CR.redundancy(CR.Map(t), 1, False, TH) == (2, 2)      # at th_depth and at 0: counted; beyond and negative: not
    assert CR.redundancy(CR.Map(t), 1, True, TH) == (4, 4)


def test_the_first_keyframe_a_held_one_and_a_neighbour_without_the_entry():
    t = redundant_map(10, 10)
    t["kf_id"][1] = 0
    assert CR.keyframe_culling(t, 0, True, TH)[2] == 0
    t = redundant_map(10, 10)
    t["kf_not_erase"][1] = 1
    out, culled, n, _ = CR.keyframe_culling(t, 0, True, TH)
    assert n == 0 and out["kf_to_be_erased"].tolist() == [0, 1, 0, 0, 0] and not out["kf_bad"].any()
    assert all(np.array_equal(out[k], t[k]) for k in CR.KEYFRAME_UPDATED if k != "kf_to_be_erased")
    # keyframe 1 lists 0 and 2; 2's row has no entry for 1 and stays as it is; 0's loses it and is ordered again
    t = redundant_map(10, 10)
    G = CR.Connections(t, 5)
    G.write(1, {0: 20, 2: 30})
    G.write(2, {3: 7, 4: 9})
    G.write(0, {1: 20, 3: 5, 4: 2})
    out, culled, n, _ = CR.keyframe_culling(t, 0, True, TH)
    assert n == 1
    assert out["conn_slot"][2, :2].tolist() == [3, 4] and out["ord_slot"][2, :2].tolist() == [4, 3] and out["n_conn"][2] == 2
    assert out["conn_slot"][0].tolist() == [3, 4, -1, -1, -1] and out["conn_weight"][0].tolist() == [5, 2, 0, 0, 0]
    assert out["ord_slot"][0].tolist() == [3, 4, -1, -1, -1] and out["kf_covis"][0, :3].tolist() == [3, 4, -1]
    assert out["n_conn"][1] == out["n_ord"][1] == 0 and (out["conn_slot"][1] == -1).all() and (out["kf_covis"][1] == -1).all()


def test_reference_keyframes_move_to_the_first_remaining_observation():
    # points 0 .. 9 redundant in keyframe 1; point 0's observations are stored as 3, 1, 2, 4 and its reference is 1;
    # point 10 is seen by 1 (stereo) and 2 alone: erasing 1 leaves mp_nobs 1 -> bad, its reference, 1, becomes 2 first
    rows = {0: [], 1: list(range(11)), 2: list(range(11)), 3: list(range(10)), 4: list(range(10))}
    t = build(5, rows, {0: {1: 20}, 1: {0: 20}}, order={0: [3, 1, 2, 4]})
    t["mp_ref_kf"][[0, 1, 10]] = 1, 2, 1
    t["kf_uright"][1, 10] = 4
    t["mp_nobs"][10] = 3
    assert CR.redundancy(CR.Map(t), 1, True, TH) == (11, 10)
    out, culled, n, _ = CR.keyframe_culling(t, 0, True, TH)
    assert n == 1 and out["mp_ref_kf"][[0, 1, 10]].tolist() == [3, 2, 2] and out["mp_nobs"][[0, 10]].tolist() == [3, 1]
    assert out["mp_bad"][10] == 1 and out["kf_mappoint"][2, 10] == -1 and out["kf_mappoint"][1, 10] == 10
    assert observers(dict(t, **out), 0) == [3, -1, 2, 4] and observers(dict(t, **out), 10) == [-1, -1]
    # a point seen by the culled keyframe alone: its reference becomes -1
    t = build(5, {**rows, 1: list(range(10)) + [11], 2: list(range(10))}, {0: {1: 20}, 1: {0: 20}})
    t["mp_ref_kf"][11] = 1
    t["mp_nobs"][11] = 4                                   # (whatever it says: 3 are left, no SetBadFlag)
    out, _, n, _ = CR.keyframe_culling(t, 0, True, TH)
    assert n == 1 and out["mp_ref_kf"][11] == -1 and out["mp_nobs"][11] == 3 and not out["mp_bad"][11]


def test_a_point_that_goes_bad_changes_a_later_target():
    # targets 1 then 2.  Points 0 .. 9 are seen by 1, 2, 3, 4, 5: redundant in both.  Point 10 is seen by 1 and 2 only
    # (mp_nobs 2: the gate is closed), so 1 counts (11, 10) and is culled; point 10 then has one observation, goes bad and
    # leaves 2's row, where it would have made 10 of 11 redundant: 2 now counts (10, 10) and is culled too.
    rows = {0: [], 1: list(range(11)), 2: list(range(11)), 3: list(range(10)), 4: list(range(10)), 5: list(range(10))}
    t = build(6, rows, {0: {1: 30, 2: 20}, 1: {0: 30}, 2: {0: 20}})
    m = CR.Map(t)
    assert CR.redundancy(m, 1, True, TH) == (11, 10) and CR.redundancy(m, 2, True, TH) == (11, 10)
    out, culled, n, trace = CR.keyframe_culling(t, 0, True, TH)
    assert culled[:2].tolist() == [1, 2] and n == 2 and ("counted", 2, 10, 10) in trace and ("cleared", 10, 2) in trace
    assert out["mp_bad"][10] == 1 and out["kf_mappoint"][2, 10] == -1 and out["mp_nobs"][:10].tolist() == [3] * 10
    # the other order leaves 2 at (11, 10) when it is looked at first: nothing is culled before 1
    t = build(6, rows, {0: {1: 20, 2: 30}, 1: {0: 20}, 2: {0: 30}})
    assert CR.keyframe_culling(t, 0, True, TH)[1][:2].tolist() == [2, 1]


def tree_map(weights, parent):
    """Keyframe 1 (under 0) is culled; 2, 3, 4 are its children; weights[(a, b)] connects a and b both ways."""
    t = redundant_map(10, 10)
    conn = {k: {} for k in range(5)}
    conn[0][1] = conn[1][0] = 20
    for (a, b), w in weights.items():
        conn[a][b] = conn[b][a] = w
    G = CR.Connections(t, 5)
    for k in range(5):
        G.write(k, conn[k])
    t["kf_parent"][:] = parent
    t["kf_pose"][1] = [0, -1, 0, 1, 0, 0, 0, 0, 1, 1, 2, 3]
    t["kf_pose"][0] = [1, 0, 0, 0, 0, -1, 0, 1, 0, 4, 5, 6]
    return t


def test_the_tree_passes_children_on_through_adopted_children():
    # 2 is connected to 0 (the original parent): adopted by 0.  3 is connected to 2 only: adopted by 2 once 2 is a
    # candidate.  4 is connected to nobody among them: it falls back to 0.
    t = tree_map({(2, 0): 5, (3, 2): 9}, [-1, 0, 1, 1, 1])
    out, culled, n, trace = CR.keyframe_culling(t, 0, True, TH)
    assert n == 1 and out["kf_parent"].tolist() == [-1, 0, 0, 2, 0]
    assert [e for e in trace if e[0] in ("adopted", "fell_back")] == [("adopted", 2, 0, False), ("adopted", 3, 2, True), ("fell_back", 4, 0)]
    # Tcp = T1 * T0^-1: R = R1 * R0^T, t = t1 - R * t0
    R1, R0 = t["kf_pose"][1, :9].reshape(3, 3), t["kf_pose"][0, :9].reshape(3, 3)
    R = R1 @ R0.T
    assert np.array_equal(out["kf_tcp"][1, :9].reshape(3, 3), R) and np.array_equal(out["kf_tcp"][1, 9:], t["kf_pose"][1, 9:] - R @ t["kf_pose"][0, 9:])
    assert (out["kf_tcp"][[0, 2, 3, 4]] == 0).all()
    # a bad child is no child, and a culled keyframe keeps its parent
    t["kf_bad"][3] = 1
    out = CR.keyframe_culling(t, 0, True, TH)[0]
    assert out["kf_parent"].tolist() == [-1, 0, 0, 1, 0]


def test_a_weight_tie_between_children_goes_to_the_lower_slot_first():
    # 2 and 3 are both connected to 0 with weight 7; 3 and 2 are connected with 9.  The first round meets (2, 0) first and
    # a tie does not replace it: 2 is adopted by 0; in the second round (3, 2) with 9 beats (3, 0) with 7.
    t = tree_map({(2, 0): 7, (3, 0): 7, (3, 2): 9}, [-1, 0, 1, 1, 0])
    out, _, n, trace = CR.keyframe_culling(t, 0, True, TH)
    assert n == 1 and out["kf_parent"].tolist() == [-1, 0, 0, 2, 0]
    # with the larger weight on 3's side, 3 goes first and 2 follows it
    t = tree_map({(2, 0): 7, (3, 0): 8, (3, 2): 9}, [-1, 0, 1, 1, 0])
    assert CR.keyframe_culling(t, 0, True, TH)[0]["kf_parent"].tolist() == [-1, 0, 3, 0, 0]


def test_compaction_and_live_children():
    off, kf, idx = np.array([0, 3, 3, 5, 6], np.int32), np.array([4, -1, 2, -1, 7, -1], np.int32), np.array([0, 1, 2, 3, 4, 5], np.int32)
    o, k, i = CR.compact_observations(off, kf, idx)
    assert o.tolist() == [0, 2, 2, 3, 3] and k[:3].tolist() == [4, 2, 7] and i[:3].tolist() == [0, 2, 4]
    off, kids = CR.live_children(np.array([-1, 0, 0, 1, 1, 9], np.int32), np.array([0, 0, 1, 0, 1, 0], np.uint8))
    assert off.tolist() == [0, 1, 2, 2, 2, 2, 2] and kids.tolist() == [1, 3]
