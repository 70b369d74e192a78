"""tests/local_ba_window_ref.py pinned on a hand-built map of six keyframes, every list written out by hand, and the generated
maps' condition: on the oracle no edge's final chi2 is within 1e-6 relative of a threshold, so the outlier set cannot turn on
rounding.  CPU only."""
import numpy as np
import pytest

import local_ba_map_cases as LC
import local_ba_window_ref as WR
from orb_slam2_refactored_amd import KP_DTYPE


def hand_map():
    """cur = 3 (id 3) with the row [1, 2, 0]: 2 is a bad neighbour, 0 has id 0.  4 sees local points from outside the row,
    5 does too but is bad.  p2 is bad, kf3's row ends in a null entry, p5 is shared by two local keyframes and has an
    erased observation, p4 is seen by no local keyframe.  The observation of p1 in keyframe 0 is stereo."""
    rows = [[1, 3, 5, -1], [0, 3, 5, -1], [1, -1, -1, -1], [0, 1, 2, -1], [0, 3, 4, -1], [1, 4, -1, -1]]
    obs = [[(1, 0), (3, 0), (4, 0)], [(0, 0), (2, 0), (3, 1), (5, 0)], [(3, 2)], [(0, 1), (1, 1), (4, 1)], [(4, 2), (5, 1)],
           [(0, 2), (1, 2), (-1, 3)]]
    K, M, cap = 6, 6, 4
    kp = np.zeros((K, cap), KP_DTYPE)
    for k in range(K):
        for i in range(cap):
            kp[k, i]["x"], kp[k, i]["y"], kp[k, i]["octave"] = 10 * k + i, 100 + 10 * k + i, (k + i) % 3
    uright = np.full((K, cap), -1, np.float32)
    uright[0, 0] = 7.5
    pose = np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]).astype(np.float32), (K, 1))
    pose[:, 11] = np.arange(K)
    ord_slot = np.full((K, 3), -1, np.int32)
    ord_slot[3] = [1, 2, 0]
    return dict(
        inv_sigma2=np.array([1, 0.5, 0.25], np.float32), scale_factors=np.array([1, 1.2, 1.44], np.float32),
        kf_id=np.array([0, 1, 2, 3, 4, 5], np.int32), kf_n=np.array([3, 3, 1, 4, 3, 2], np.int32),
        kf_bad=np.array([0, 0, 1, 0, 0, 1], np.uint8), kf_mappoint=np.array(rows, np.int32), kf_keypoint=kp,
        kf_kp_octave=np.ascontiguousarray(kp["octave"], np.int32), kf_uright=uright,
        kf_camera=np.tile(np.array([500, 500, 320, 240, 40, 0.08], np.float32), (K, 1)), kf_pose=pose, ord_slot=ord_slot,
        n_ord=np.array([0, 0, 0, 3, 0, 0], np.int32), mp_bad=np.array([0, 0, 1, 0, 0, 0], np.uint8),
        mp_xw=np.arange(18, dtype=np.float32).reshape(6, 3) + 20, mp_nobs=np.array([3, 5, 1, 3, 2, 2], np.int32),
        mp_ref_kf=np.array([1, 0, 3, 1, 4, 0], np.int32),
        mp_obs_off=np.cumsum([0] + [len(o) for o in obs]).astype(np.int32),
        mp_obs_kf=np.array([k for o in obs for k, _ in o], np.int32), mp_obs_idx=np.array([i for o in obs for _, i in o], np.int32),
        mp_normal=np.zeros((M, 3), np.float32), mp_max_min=np.zeros((M, 2), np.float32))


def test_the_window_of_the_hand_built_map():
    t = hand_map()
    w = WR.gather(t, 3)
    assert w["counts"] == (3, 1, 4, 10) and w["status"] == WR.OK and w["one_cam"] == 1
    assert w["pose_kf"].tolist() == [3, 1, 0, 4]             # the bad neighbour 2 and the bad observer 5 are not vertices
    assert w["pose_fixed"].tolist() == [0, 0, 1, 1]          # id 0 and the fixed camera
    assert w["point"].tolist() == [0, 1, 3, 5]               # p2 is bad; p5 once, from keyframe 1
    assert w["edge_point"].tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3]
    assert w["edge_kf"].tolist() == [1, 3, 4, 0, 3, 0, 1, 4, 0, 1]   # p1 without the bad 2 and 5, p5 without the erased one
    assert w["edge_pose"].tolist() == [1, 0, 3, 2, 0, 2, 1, 3, 2, 1]
    assert w["edge_idx"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2]
    assert w["edge_obs"][3].tolist() == [0.0, 100.0, 7.5] and w["edge_obs"][4].tolist() == [31.0, 131.0, -1.0]
    assert w["edge_inv_sigma2"].tolist() == [t["inv_sigma2"][(k + i) % 3] for k, i in zip(w["edge_kf"], w["edge_idx"])]
    assert np.array_equal(w["edge_cam"], np.tile(t["kf_camera"][0, :5], (10, 1)))


def test_an_empty_row_and_cur_with_id_zero():
    t = hand_map()
    w = WR.gather(t, 0)                                      # no neighbours: the window is keyframe 0 alone, fixed
    assert w["pose_kf"].tolist() == [0, 3, 1, 4] and w["pose_fixed"].tolist() == [1, 1, 1, 1]   # p1 meets 3 first; 2, 5 bad
    assert w["counts"][0] == 1 and w["point"].tolist() == [1, 3, 5]


def test_capacities_one_short_overflow():
    t = hand_map()
    for caps in ((3, 4, 10), (4, 3, 10), (4, 4, 9)):
        w = WR.gather(t, 3, caps)
        assert w["status"] == WR.OVERFLOW and w["counts"] == (3, 1, 4, 10) and w["pose_kf"] is None
    assert WR.gather(t, 3, (4, 4, 10))["status"] == WR.OK


def test_a_camera_of_its_own_ends_the_shared_camera():
    t = hand_map()
    t["kf_camera"][4, 0] = 501
    assert WR.gather(t, 3)["one_cam"] == 0


def test_the_write_back_of_the_hand_built_map():
    t = hand_map()
    w = WR.gather(t, 3)
    P, N = 4, 4
    R = np.tile(np.eye(3).reshape(-1), (P, 1)) + 1e-9        # not representable in float: the narrowing shows
    tr, X = np.arange(3 * P, dtype=np.float64).reshape(P, 3) + 0.1, np.arange(3 * N, dtype=np.float64).reshape(N, 3) + 50.1
    outlier = np.zeros(10, np.uint8)
    outlier[[1, 2, 3, 6]] = 1
    u = WR.apply(t, w, outlier, R, tr, X)
    # edge 1 (p0 in cur): 3 mono observations down to 2 -> bad, every cell cleared; edge 2 (p0 in the fixed camera 4) then
    # does nothing: nobs stays 2
    assert u["mp_bad"].tolist() == [1, 0, 1, 1, 0, 0] and u["mp_nobs"][0] == 2
    assert u["kf_mappoint"][1, 0] == -1 and u["kf_mappoint"][3, 0] == -1 and u["kf_mappoint"][4, 0] == -1
    assert (u["mp_obs_kf"][0:3] == -1).all()
    # edge 3 (p1 in keyframe 0, stereo): nobs 5 - 2, the reference keyframe moves to the first one left, the bad 2
    assert u["mp_nobs"][1] == 3 and u["mp_ref_kf"][1] == 2 and u["kf_mappoint"][0, 0] == -1 and u["mp_obs_kf"][3] == -1
    # edge 6 (p3 in its reference keyframe 1): the reference moves to keyframe 0, then nobs 3 - 1 -> bad
    assert u["mp_nobs"][3] == 2 and u["mp_ref_kf"][3] == 0 and u["kf_mappoint"][4, 1] == -1
    assert u["kf_pose"][3, 0] == np.float32(1 + 1e-9) and u["kf_pose"][1, 9] == np.float32(3.1) and u["kf_pose"][4, 11] == 4   # fixed: kept
    assert u["kf_pose"][0, 9] == np.float32(6.1)             # id 0 is written too
    assert u["mp_xw"][5, 2] == np.float32(61.1) and u["mp_xw"][0, 0] == np.float32(50.1)   # a point gone bad still moves
    assert (u["mp_normal"][1] != 0).any() and (u["mp_normal"][0] == 0).all()   # UpdateNormalAndDepth returns early on bad
    assert np.array_equal(WR.apply(t, w, np.zeros(10, np.uint8), R, tr, X)["mp_obs_kf"], t["mp_obs_kf"])


def test_the_flattened_window_runs_on_the_oracle(oracle):
    t = hand_map()
    out = oracle.local_ba(WR.flatten(t, WR.gather(t, 3)))
    assert len(out["edge_outlier"]) == 10 and np.isfinite(out["points"]).all()


@pytest.mark.parametrize("name", list(LC.CASES))
def test_the_generated_maps_decide_far_from_rounding(oracle, name):
    t, cur = LC.case(name)
    w = WR.gather(t, cur)
    n_local, n_fixed, n_points, n_edges = w["counts"]
    assert n_local == LC.CASES[name][1] and n_fixed == LC.CASES[name][3] and n_edges > 4 * n_local
    assert len(set(w["pose_kf"])) == n_local + n_fixed and not t["kf_bad"][w["pose_kf"]].any()
    out = oracle.local_ba(WR.flatten(t, w))
    th = np.where(w["edge_obs"][:, 2] < 0, 5.991, 7.815)
    assert (np.abs(out["edge_chi2"] / th - 1) > 1e-6).all()
    assert 0 < out["edge_outlier"].sum() < n_edges // 4
