"""Pins the restatement tests/map_maintenance_ref.py on hand-built maps whose answers are written out here: the threshold, the
maximum fallback and its tie, the order of equal weights, what AddConnection does to a neighbour's ordered list, the parent,
the empty counter, and UpdateNormalAndDepth's special cases and its dependence on the observation order.  CPU only."""
import numpy as np

import map_maintenance_cases as MC
import map_maintenance_ref as R


def build(n_kf, shared, conn_cap=8, kf_cap=64, ids=None):
    """shared: {(kf, kf, ...): n} -> n points observed by exactly those keyframes."""
    obs = [list(kfs) for kfs, n in shared.items() for _ in range(n)]
    kf_mappoint, kf_n = np.full((n_kf, kf_cap), -1, np.int32), np.zeros(n_kf, np.int32)
    for p, kfs in enumerate(obs):
        for k in kfs:
            kf_mappoint[k, kf_n[k]] = p
            kf_n[k] += 1
    g = dict(kf_id=np.array(ids if ids is not None else range(1, n_kf + 1), np.int32), kf_n=kf_n, kf_mappoint=kf_mappoint,
             mp_bad=np.zeros(len(obs), np.uint8), mp_obs_off=np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32),
             mp_obs_kf=np.array([k for o in obs for k in o], np.int32))
    g.update(MC.empty_state(n_kf, conn_cap))
    return g


def row(out, name, k):
    n = out["n_conn" if name.startswith("conn") else "n_ord"][k]
    assert (out[name][k, n:] == (-1 if name.endswith("slot") else 0)).all()
    return out[name][k, :n].tolist()


def set_rows(g, k, conn, ordered):
    for name, vals in (("conn_slot", [s for s, _ in conn]), ("conn_weight", [w for _, w in conn]),
                       ("ord_slot", [s for s, _ in ordered]), ("ord_weight", [w for _, w in ordered])):
        g[name][k, :len(vals)] = vals
    g["n_conn"][k], g["n_ord"][k] = len(conn), len(ordered)
    g["kf_covis"][k, :len(ordered)] = [s for s, _ in ordered]


def test_counts_of_14_and_15_fall_on_either_side_of_the_threshold():
    g = build(3, {(0, 1): 15, (0, 2): 14})
    o = R.update_connections(g, [0])
    assert row(o, "conn_slot", 0) == [1, 2] and row(o, "conn_weight", 0) == [15, 14]     # the whole counter
    assert row(o, "ord_slot", 0) == [1] and row(o, "ord_weight", 0) == [15]              # the pairs
    assert row(o, "conn_slot", 1) == [0] and row(o, "conn_weight", 1) == [15] and row(o, "ord_slot", 1) == [0]
    assert o["n_conn"][2] == 0 and o["n_ord"][2] == 0                                     # 14: no AddConnection
    assert o["kf_covis"][0].tolist() == [1] + [-1] * 9 and o["kf_covis"][2].tolist() == [-1] * 10
    assert (o["status"] == 0).all()


def test_without_a_count_at_the_threshold_the_maximum_is_the_only_pair_and_a_tie_goes_to_the_lowest_slot():
    g = build(4, {(0, 1): 2, (0, 2): 3, (0, 3): 3})
    o = R.update_connections(g, [0])
    assert row(o, "conn_slot", 0) == [1, 2, 3] and row(o, "conn_weight", 0) == [2, 3, 3]
    assert row(o, "ord_slot", 0) == [2] and row(o, "ord_weight", 0) == [3]
    assert row(o, "conn_slot", 2) == [0] and o["n_conn"][3] == 0 and o["n_conn"][1] == 0
    assert o["kf_parent"].tolist() == [2, -1, -1, -1]


def test_equal_weights_are_ordered_by_descending_slot():
    g = build(4, {(0, 1): 15, (0, 2): 16, (0, 3): 15})
    o = R.update_connections(g, [0])
    assert row(o, "ord_slot", 0) == [2, 3, 1] and row(o, "ord_weight", 0) == [16, 15, 15]
    assert o["kf_parent"][0] == 2 and o["kf_first_connection"].tolist() == [0, 1, 1, 1]


def test_add_connection_rebuilds_the_neighbours_ordered_list_from_its_whole_row():
    g = build(4, {(0, 1): 15})
    set_rows(g, 1, [(2, 5), (3, 20)], [(3, 20)])              # as its own update left it: the pairs only
    o = R.update_connections(g, [0])
    assert row(o, "conn_slot", 1) == [0, 2, 3] and row(o, "conn_weight", 1) == [15, 5, 20]
    assert row(o, "ord_slot", 1) == [3, 0, 2] and row(o, "ord_weight", 1) == [20, 15, 5]    # the entry below 15 included
    assert o["kf_covis"][1].tolist() == [3, 0, 2] + [-1] * 7


def test_add_connection_with_an_unchanged_weight_rebuilds_nothing():
    g = build(4, {(0, 1): 15})
    set_rows(g, 1, [(0, 15), (2, 5), (3, 20)], [(3, 20)])
    o = R.update_connections(g, [0])
    assert row(o, "ord_slot", 1) == [3] and row(o, "conn_weight", 1) == [15, 5, 20]
    g["conn_weight"][1, 0] = 14                               # another weight: rebuilt
    o = R.update_connections(g, [0])
    assert row(o, "ord_slot", 1) == [3, 0, 2] and row(o, "conn_weight", 1) == [15, 5, 20]


def test_the_parent_is_set_once_and_never_for_id_0():
    g = build(3, {(0, 1): 15, (1, 2): 20, (0, 2): 15}, ids=[0, 7, 9])
    o = R.update_connections(g, [0, 1])
    assert o["kf_parent"].tolist() == [-1, 2, -1] and o["kf_first_connection"].tolist() == [1, 0, 1]   # id 0 keeps the flag
    g.update({k: o[k] for k in R.STATE_KEYS})
    g["kf_parent"][1] = 0                                     # e.g. ChangeParent
    o = R.update_connections(g, [1, 2, 1])
    assert o["kf_parent"].tolist() == [-1, 0, 1] and o["kf_first_connection"].tolist() == [1, 0, 0]


def test_an_empty_counter_changes_nothing():
    g = build(3, {(0,): 5, (1, 2): 15})
    set_rows(g, 0, [(2, 9)], [(2, 9)])
    before = {k: g[k].copy() for k in R.STATE_KEYS}
    o = R.update_connections(g, [0])
    assert all(np.array_equal(o[k], before[k]) for k in R.STATE_KEYS) and o["kf_first_connection"][0] == 1
    g["kf_id"][:] = 4                                         # every observer has the keyframe's own id
    o = R.update_connections(g, [1])
    assert all(np.array_equal(o[k], before[k]) for k in R.STATE_KEYS)


def test_a_row_wider_than_the_capacity_is_reported_and_kept():
    g = build(4, {(0, 1): 15, (0, 2): 15, (0, 3): 1}, conn_cap=2)
    o = R.update_connections(g, [0, 3])
    assert o["status"].tolist() == [R.CONN_OVERFLOW, 0, 0, 0] and o["n_conn"][0] == 0 and o["kf_first_connection"][0] == 1
    assert row(o, "conn_slot", 1) == [0] and row(o, "conn_slot", 2) == [0] and row(o, "conn_slot", 3) == [0]   # the others: as with room


def points(Xw, obs, ref, pose, octave, bad=0):
    n_kf = len(pose)
    return dict(mp_bad=np.array([bad], np.uint8), mp_xw=np.array([Xw], np.float32), mp_ref_kf=np.array([ref], np.int32),
                mp_obs_off=np.array([0, len(obs)], np.int32), mp_obs_kf=np.array([k for k, _ in obs], np.int32),
                mp_obs_idx=np.array([i for _, i in obs], np.int32), kf_pose=np.array(pose, np.float32), kf_n=np.full(n_kf, 4, np.int32),
                kf_kp_octave=np.array(octave, np.int32), mp_normal=np.full((1, 3), 7, np.float32), mp_max_min=np.full((1, 2), 7, np.float32))


EYE = [1, 0, 0, 0, 1, 0, 0, 0, 1]
SCALE = np.array([1, 2, 4, 8], np.float32)


def test_normal_and_distances_of_a_point_seen_from_two_centres():
    # Ow0 = 0, Ow1 = (2, 0, 2); X = (0, 0, 2): the unit vectors (0, 0, 1) and (-1, 0, 0)
    t = points((0, 0, 2), [(0, 1), (1, 3)], 1, [EYE + [0, 0, 0], EYE + [-2, 0, -2]], [[0, 1, 0, 0], [0, 0, 0, 2]])
    n, mm = R.update_normal_depth(t, SCALE)
    assert n.tolist() == [[-0.5, 0, 0.5]] and mm.tolist() == [[8, 1]]       # dist 2 from keyframe 1, octave 2: 4 * 2, / 8
    assert R.center(np.array([0, -1, 0, 1, 0, 0, 0, 0, 1, 1, 2, 3], np.float32)).tolist() == [-2, 1, -3]   # -R^T t


def test_a_reference_keyframe_that_does_not_observe_takes_keypoint_0():
    t = points((0, 0, 2), [(0, 1)], 1, [EYE + [0, 0, 0], EYE + [0, 0, 1]], [[0, 1, 0, 0], [3, 0, 0, 0]])
    n, mm = R.update_normal_depth(t, SCALE)
    assert n.tolist() == [[0, 0, 1]] and mm.tolist() == [[24, 3]]           # Ow1 = (0, 0, -1): dist 3, octave 3


def test_a_bad_point_an_empty_point_and_a_point_without_reference_are_left_untouched():
    for kw in (dict(bad=1), dict(obs=[]), dict(ref=-1), dict(ref=2)):
        t = points((0, 0, 2), kw.get("obs", [(0, 1)]), kw.get("ref", 0), [EYE + [0, 0, 0], EYE + [0, 0, 1]], [[0, 1, 0, 0], [3, 0, 0, 0]],
                   bad=kw.get("bad", 0))
        n, mm = R.update_normal_depth(t, SCALE)
        assert (n == 7).all() and (mm == 7).all(), kw


def test_the_order_of_the_observations_decides_the_bits():
    t = MC.points(MC.case("clean"))
    fwd, _ = R.update_normal_depth(t, MC.SCALE)
    rev, _ = R.update_normal_depth(t, MC.SCALE, reverse=True)
    differ = (fwd.view(np.uint32) != rev.view(np.uint32)).any(axis=1)
    assert differ.sum() > 20 and np.abs(fwd - rev).max() < 1e-6           # the same sums, other roundings
