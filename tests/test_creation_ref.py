"""tests/creation_ref.py pinned on hand-built maps: what the reference's constructors and the calls after them leave
(src/KeyFrame.cc:51-64, src/MapPoint.cc:44-56, src/Tracking.cc:724-736, :1104-1126, src/LocalMapping.cc:562-575), and on the
created rows the agreement with the existing restatements of AddObservation, the distinctive descriptor and
UpdateNormalAndDepth.  CPU only."""
import numpy as np

import creation_cases as CC
import creation_ref as CR
import map_maintenance_ref as MR
import newpoints_cases as NC
import newpoints_ref as NR
import observe_ref as OR
import sim3_ref as SR


def hand_map(M=6, rows=(2, 2, 2, 2, 2, 2)):
    """Three keyframes of four keypoints; keyframe 1's keypoints 0 and 1 are stereo, everything else monocular; no point yet."""
    t = CC.make_map(K=3, kf_cap=4, M=M, alloc=0, seed=1, short_last_kf=False)
    t["kf_bad"][:] = 0
    t["kf_uright"][:] = -1
    t["kf_uright"][1, :2] = 100.0
    t["mp_obs_off"] = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    t["mp_obs_kf"] = np.full(t["mp_obs_off"][-1], -1, np.int32)
    t["mp_obs_idx"] = np.full(t["mp_obs_off"][-1], -1, np.int32)
    return t


def lists(kf1, idx1, kf2=None, idx2=None, cap=4):
    I = len(kf1)
    ls = dict(kf1=np.array(kf1, np.int32), n_list=np.array([len(r) for r in idx1], np.int32), idx1=np.full((I, cap), -1, np.int32),
              xw=np.arange(I * cap * 3, dtype=np.float32).reshape(I, cap, 3))
    for i, r in enumerate(idx1):
        ls["idx1"][i, :len(r)] = r
    if kf2 is not None:
        ls["kf2"], ls["idx2"] = np.array(kf2, np.int32), np.full((I, cap), -1, np.int32)
        for i, r in enumerate(idx2):
            ls["idx2"][i, :len(r)] = r
    return ls


def row(t, upd, p):
    e0, e1 = t["mp_obs_off"][p], t["mp_obs_off"][p + 1]
    return list(zip(upd["mp_obs_kf"][e0:e1], upd["mp_obs_idx"][e0:e1]))


def test_one_stereo_point_and_one_mono_point():
    t = hand_map()
    upd, out = CR.create_points(t, lists([1], [[1, 2]]), 0)
    assert list(out["created"][0]) == [0, 1, -1, -1] and out["alloc"][0] == 2 and out["status"][0] == CR.OK
    assert list(upd["mp_nobs"][:3]) == [2, 1, 0] and row(t, upd, 0) == [(1, 1), (-1, -1)] and row(t, upd, 1) == [(1, 2), (-1, -1)]
    assert list(upd["kf_mappoint"][1]) == [-1, 0, 1, -1]
    for k, v in dict(mp_bad=0, mp_replaced=-1, mp_found=1, mp_visible=1, mp_first_kf_id=t["kf_id"][1], mp_ref_kf=1).items():
        assert (upd[k][:2] == v).all() and (upd[k][2:] == t[k][2:]).all(), k
    assert not upd["mp_normal"][:2].any() and not upd["mp_max_min"][:2].any()   # the constructor's zeros
    assert np.array_equal(upd["mp_xw"][1], [3, 4, 5]) and np.array_equal(upd["mp_desc"][1], t["kf_desc"][1, 2])


def test_two_observations_ascend_in_slot_whichever_keyframe_is_the_reference():
    t = hand_map()
    upd, out = CR.create_points(t, lists([2], [[3]], [1], [[0]]), 0)      # kf1 > kf2
    assert row(t, upd, 0) == [(1, 0), (2, 3)] and upd["mp_ref_kf"][0] == 2 and upd["mp_first_kf_id"][0] == t["kf_id"][2]
    assert upd["mp_nobs"][0] == 3 and upd["kf_mappoint"][2, 3] == 0 and upd["kf_mappoint"][1, 0] == 0
    assert np.array_equal(upd["mp_desc"][0], t["kf_desc"][1, 0])          # the first in map order, not the reference keyframe's


def test_the_descriptor_skips_bad_keyframes():
    t = hand_map()
    ls = lists([2], [[3]], [1], [[0]])
    upd, _ = CR.create_points(dict(t, kf_bad=np.array([0, 1, 0], np.uint8)), ls, 0)
    assert np.array_equal(upd["mp_desc"][0], t["kf_desc"][2, 3])
    upd, _ = CR.create_points(dict(t, kf_bad=np.array([0, 1, 1], np.uint8)), ls, 0)
    assert np.array_equal(upd["mp_desc"][0], t["mp_desc"][0])             # descriptors.empty(): return


def test_a_dropped_entry_takes_no_slot():
    t = hand_map()
    t["kf_n"][0] = 2
    upd, out = CR.create_points(t, lists([0, 5, 1], [[0, 2, 1], [0], [3, -1, 0]]), 0)
    assert [list(r) for r in out["created"]] == [[0, -1, 1, -1], [-1] * 4, [2, -1, 3, -1]] and list(out["n_created"]) == [2, 0, 2]
    upd, out = CR.create_points(t, lists([1], [[0]], [1], [[1]]), 0)      # kf1 == kf2
    assert out["alloc"][0] == 0 and (out["created"] == -1).all()


def test_the_exact_fit_and_one_short_of_every_capacity():
    ls = lists([0, 1], [[0, 1], [2, 3]], [2, 2], [[0, 1], [2, 3]])        # four points of two observations
    t = hand_map(M=6)
    for alloc, status, needed in ((2, CR.OK, [6, -1]), (3, CR.OVERFLOW, [7, -1])):
        upd, out = CR.create_points(t, ls, alloc)
        assert out["status"][0] == status and list(out["needed"]) == needed and out["alloc"][0] == (6 if status == CR.OK else 3)
        if status == CR.OVERFLOW:
            CC.assert_same(upd, {k: t[k] for k in upd})
            assert (out["created"] == -1).all() and not out["n_created"].any()
    short = hand_map(rows=(2, 2, 2, 1, 2, 2))
    upd, out = CR.create_points(short, ls, 1)                             # slot 3 is the third of the batch
    assert out["status"][0] == CR.OVERFLOW and list(out["needed"]) == [5, 3]
    CC.assert_same(upd, {k: short[k] for k in upd})
    assert CR.create_points(short, lists([0, 1], [[0, 1], [2, 3]]), 1)[1]["status"][0] == CR.OK   # one observation fits it
    for cap, status in ((5, CR.OK), (4, CR.OVERFLOW)):
        upd, out = CR.create_points(t, ls, 0, recent=np.full(cap, -2, np.int32), n_recent=1)
        assert out["status"][0] == status and list(out["recent"]) == ([-2, 0, 1, 2, 3] if status == CR.OK else [-2] * 4)
        assert out["n_recent"][0] == (5 if status == CR.OK else 1)


def test_the_constructor_state_of_a_keyframe_row_with_padding():
    fr, kf = CC.make_frames(F=2, kp_cap=5), CC.make_keyframes(K=3, kf_cap=7, conn_cap=4)
    fr["frame_n"][:] = (3, 5)
    got = CR.insert_keyframes(fr, kf, np.array([0], np.int32), np.array([2], np.int32), np.array([41], np.int32), np.array([0.5], np.float32))
    assert list(got["kf_mappoint"][2]) == list(fr["frame_mappoint"][0, :3]) + [-1] * 4 and got["kf_n"][2] == 3 and got["kf_id"][2] == 41
    for dst, src in CR.PER_KEYPOINT[1:]:
        assert np.array_equal(got[dst][2, :3], fr[src][0, :3]) and np.array_equal(got[dst][2, 3:], kf[dst][2, 3:]), dst
    assert [got[k][2] for k in ("kf_bad", "kf_not_erase", "kf_to_be_erased", "kf_parent", "kf_first_connection", "n_conn", "n_ord")] == [0, 0, 0, -1, 1, 0, 0]
    assert (got["conn_slot"][2] == -1).all() and (got["ord_slot"][2] == -1).all() and not got["conn_weight"][2].any() and not got["ord_weight"][2].any()
    assert (got["kf_covis"][2] == -1).all() and np.array_equal(got["kf_pose"][2], fr["pose"][0])
    assert np.array_equal(got["kf_camera"][2], np.append(fr["camera"][0], np.float32(0.5)))
    assert all(np.array_equal(got[k][:2], kf[k][:2]) for k in kf)         # the other keyframes are not touched


def test_the_existing_restatements_agree_on_the_created_rows():
    t = CC.make_map(K=6, kf_cap=64, M=200, alloc=9, seed=2)
    ls = CC.make_lists(t, (20, 0, 31, 7), 64, two=True, drops=2)
    upd, out = CR.create_points(t, ls, 9)
    # observe_ref's AddObservation on the empty rows
    m = OR.Map({k: t[k] for k in ("kf_n", "kf_mappoint", "kf_uright", "mp_bad", "mp_nobs", "mp_found", "mp_visible", "mp_replaced",
                                  "mp_obs_off", "mp_obs_kf", "mp_obs_idx")})
    begin, rows = [0], []
    for i in range(4):
        for j in range(64):
            p = out["created"][i, j]
            if p < 0:
                continue
            for k, idx in ((ls["kf1"][i], ls["idx1"][i, j]), (ls["kf2"][i], ls["idx2"][i, j])):
                assert m.add_observation(p, int(k), int(idx))
            live = [(k, idx) for k, idx in m.observations(p) if not t["kf_bad"][k]]
            rows += [t["kf_desc"][k, idx] for k, idx in live]
            begin.append(len(rows))
    n = int(out["alloc"][0]) - 9
    assert n == CC.n_valid(t, ls) > 50
    for k in ("mp_obs_kf", "mp_obs_idx", "mp_nobs"):
        assert np.array_equal(m.t[k], upd[k]), k
    # sim3_ref's distinctive descriptor over the live rows (the points are in slot order: begin follows it)
    order = np.argsort(out["created"][out["created"] >= 0])
    assert np.array_equal(order, np.arange(n))
    best, _ = SR.distinctive_descriptors(np.array(rows), begin)
    for r in range(n):
        want = rows[begin[r] + best[r]] if best[r] >= 0 else t["mp_desc"][9 + r]
        assert np.array_equal(upd["mp_desc"][9 + r], want), r
    assert (best == 0).sum() > 10 and (np.diff(begin) == 1).sum() > 5      # points with a bad keyframe among the two


def test_update_normal_depth_on_the_created_points_equals_the_triangulation():
    b = NC.flat(NC.cases()["stereo_loop"])
    pairs = NR.prepare(b)
    tri = NR.triangulate(b, pairs, NC.nearest_matches(b, pairs))
    K, cap = b["kps1"].shape
    assert b["kps2"].shape == (K, cap) and np.array_equal(b["pose1"], b["pose2"])   # one set of keyframes
    seen, keep = set(), np.zeros(len(pairs["frame1"]), bool)               # the plan entries that share no keypoint
    for p in range(len(keep)):
        used = {(int(pairs["frame1"][p]), int(i)) for i in tri["new_idx1"][p, :tri["n_created"][p]]} | \
               {(int(pairs["frame2"][p]), int(i)) for i in tri["new_idx2"][p, :tri["n_created"][p]]}
        if pairs["skip"][p] == 0 and not used & seen:
            keep[p] = True
            seen |= used
    n = int(tri["n_created"][keep].sum())
    assert n > 20
    t = CC.make_map(K=K, kf_cap=cap, M=n + 2, alloc=0, seed=3, rows=(2, 2), short_last_kf=False)
    t["kf_n"] = b["counts1"].astype(np.int32)
    t["kf_uright"] = b["uright1"] if b.get("uright1") is not None else np.full((K, cap), -1, np.float32)
    ls = dict(kf1=pairs["frame1"][keep], kf2=pairs["frame2"][keep], n_list=tri["n_created"][keep], idx1=tri["new_idx1"][keep],
              idx2=tri["new_idx2"][keep], xw=tri["xw"][keep])
    upd, out = CR.create_points(t, ls, 0, by_keypoint=True)
    assert out["alloc"][0] == n and not upd["mp_normal"][:n].any()
    T34 = b["pose1"].reshape(K, 3, 4)                                     # orblm_batch holds Tcw as 3 x 4; kf_pose is Rcw, then tcw
    kf_pose = np.concatenate([T34[:, :, :3].reshape(K, 9), T34[:, :, 3]], axis=1).astype(np.float32)
    pts = dict(t, **upd, kf_pose=kf_pose, kf_kp_octave=b["kps1"]["octave"].astype(np.int32))
    normal, max_min = MR.update_normal_depth(pts, b["scale_factors2"], points=np.arange(n))
    full, _ = CR.create_points(t, dict(ls, normal=tri["normal"][keep], max_distance=tri["max_distance"][keep],
                                       min_distance=tri["min_distance"][keep]), 0, by_keypoint=True)
    assert np.array_equal(CC.bits(normal[:n]), CC.bits(full["mp_normal"][:n]))
    assert np.array_equal(CC.bits(max_min[:n]), CC.bits(full["mp_max_min"][:n]))
