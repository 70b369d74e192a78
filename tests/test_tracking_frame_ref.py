"""tests/tracking_frame_ref.py pinned on hand-built frames: both sides of every gate of the cited reference lines.  CPU only."""
import numpy as np
import pytest

import tracking_frame_ref as R
from orb_slam2_refactored_amd import tracking as T

f32 = np.float32
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)
CAM = np.array([500, 500, 320, 240, 40], f32)


def frame(mappoint, **kw):
    """One frame whose frame_n is len(mappoint) in a row two slots longer (the padding holds 7s that must survive)."""
    n = len(mappoint)
    cap = n + 2
    pad = lambda a, fill, dt: np.concatenate([np.asarray(a, dt), np.full(2, fill, dt)]).reshape(1, cap)   # noqa: E731
    fr = dict(frame_n=np.array([n], np.int32), frame_mappoint=pad(mappoint, 7, np.int32),
              frame_outlier=pad(kw.pop("outlier", np.zeros(n)), 7, np.uint8), pose=IDENT.reshape(1, 12).copy(),
              camera=CAM.reshape(1, 5).copy(), bounds=np.array([[0, 640, 0, 480]], f32),
              kp_xy=np.zeros((1, cap, 2), f32), kp_octave=pad(kw.pop("octave", np.zeros(n)), 0, np.int32),
              kp_uright=pad(kw.pop("uright", np.full(n, -1.0)), 0, f32), kp_depth=pad(kw.pop("depth", np.zeros(n)), 5.0, f32),
              kp_angle=pad(np.zeros(n), 0, f32))
    assert not kw
    return fr


def the_map(nobs, **kw):
    M = len(nobs)
    return dict(mp_nobs=np.asarray(nobs, np.int32), mp_xw=np.arange(3 * M, dtype=f32).reshape(M, 3) + f32(0.5),
                mp_bad=np.asarray(kw.get("bad", np.zeros(M)), np.uint8), mp_found=np.zeros(M, np.int32),
                mp_replaced=np.asarray(kw.get("replaced", np.full(M, -1)), np.int32), mp_desc=np.arange(32 * M).reshape(M, 32).astype(np.uint8),
                kf_n=np.asarray(kw.get("kf_n", [0]), np.int32), kf_mappoint=np.asarray(kw.get("kf_mappoint", [[-1]]), np.int32))


def test_constants_are_the_library_s():
    assert (R.MERGE, R.REPLACE, R.DISCARD, R.LOCAL_MAP, R.KEYFRAME, R.VO, R.INIT) == \
        (T.MERGE, T.REPLACE, T.DISCARD, T.LOCAL_MAP, T.KEYFRAME, T.VO, T.INIT)


def test_apply_matches_merge_keeps_and_replace_clears():
    src = np.array([[10, 11, -1, 99]], np.int32)
    for mode, want in ((R.MERGE, [10, 1, -1, 3, -1, 5]), (R.REPLACE, [10, -1, -1, -1, -1, -1])):
        fr = frame([0, 1, 2, 3, 4, 5])
        R.apply_matches(fr, mode, np.array([[0, -1, 2, 4, 3, -5, 0, 0]], np.int32), src, None, 50)   # 4: outside the row; 99 >= M
        assert list(fr["frame_mappoint"][0]) == want + [7, 7]
    fr = frame([0, 1])
    R.apply_matches(fr, R.REPLACE, np.array([[1, 1, 1, 1]], np.int32), np.array([[1, 2], [3, 4]], np.int32), np.array([1], np.int32), 50)
    assert list(fr["frame_mappoint"][0]) == [4, 4, 7, 7]
    fr = frame([0, 1])
    R.apply_matches(fr, R.MERGE, np.array([[1, 1, 1, 1]], np.int32), np.array([[1, 2]], np.int32), np.array([3], np.int32), 50)
    assert list(fr["frame_mappoint"][0]) == [0, 1, 7, 7]   # a row outside the table: no match


@pytest.mark.parametrize("n_edges", [0, 2, 3, 9, 10])
def test_pose_edges_gathers_in_keypoint_order(n_edges):
    n = 12
    mp = np.full(n, -1)
    idx = np.arange(n)[::-1][:n_edges][::-1] if n_edges else np.zeros(0, int)   # the last n_edges keypoints
    mp[idx] = np.arange(n_edges) % 4
    ur = np.resize(np.array([-1.0, -0.0, 0.0, 3.5], f32), n)
    fr = frame(mp, outlier=np.ones(n), uright=ur, octave=np.arange(n) % 3)
    fr["kp_xy"][0, :, 0], fr["kp_xy"][0, :, 1] = np.arange(n + 2) + 0.25, np.arange(n + 2) * 2
    m = the_map([1, 1, 1, 1])
    table = np.array([1.0, 0.69444, 0.48225], f32)
    e = R.pose_edges(fr, m, table)
    assert list(e["edge_begin"]) == [0, n_edges] and list(e["edge_kp"][:n_edges]) == list(idx)
    assert list(fr["frame_outlier"][0]) == [0 if i in idx else 1 for i in range(n)] + [7, 7]   # cleared for exactly those
    for j, i in enumerate(idx):
        assert np.array_equal(e["xw"][j], m["mp_xw"][mp[i]].astype(np.float64))
        assert e["obs"][j, 0] == i + 0.25 and e["obs"][j, 1] == 2 * i
        assert e["obs"][j, 2].tobytes() == np.float64(ur[i]).tobytes()   # -0.0 stays -0.0: the optimiser types at ur < 0
        assert e["inv_sigma2"][j] == np.float64(table[i % 3])
    assert np.array_equal(e["pose_R"][0], IDENT[:9].astype(np.float64)) and np.array_equal(e["cam"][0], CAM.astype(np.float64))
    # the result taken back: fewer than 3 edges keep the pose and the zero flags
    res = dict(pose_R=e["pose_R"] + 1e-9, pose_t=e["pose_t"] + 0.1, outlier=np.ones(len(e["edge_kp"]), np.uint8))
    out = R.finish_pose(fr, m, R.DISCARD, e, res)
    if n_edges < 3:
        assert np.array_equal(fr["pose"][0], IDENT) and out["n_discarded"][0] == 0 and out["n_inliers"][0] == n_edges
    else:
        assert np.array_equal(fr["pose"][0, 9:], np.full(3, 0.1).astype(f32)) and fr["pose"][0, 0] == f32(1 + 1e-9)
        assert out["n_discarded"][0] == n_edges and list(out["discarded"][0, :n_edges]) == list(mp[idx]) and out["n_inliers"][0] == 0
        assert (fr["frame_mappoint"][0, :n] == -1).all() and (fr["frame_outlier"][0, idx] == 0).all()


def test_pose_edges_all_null_and_all_matched_rows():
    m = the_map([1, 1])
    e = R.pose_edges(frame([-1] * 5), m, np.ones(1, f32))
    assert list(e["edge_begin"]) == [0, 0]
    e = R.pose_edges(frame([0, 1, 0, 1, 9]), m, np.ones(1, f32))   # 9 is outside the table: null
    assert list(e["edge_begin"]) == [0, 4] and list(e["edge_kp"][:4]) == [0, 1, 2, 3]
    mp = [0, 1, 1, 0, 1, 0, 0]                                       # every keypoint below frame_n holds a point
    fr = frame(mp, outlier=np.ones(7))
    e = R.pose_edges(fr, m, np.ones(1, f32))
    assert list(e["edge_begin"]) == [0, 7] and list(e["edge_kp"][:7]) == list(range(7)) and not e["edge_kp"][7:].any()
    assert list(fr["frame_outlier"][0]) == [0] * 7 + [7, 7]          # edge count == frame_n; the padding holds no edge
    assert np.array_equal(e["xw"][:7], m["mp_xw"][mp].astype(np.float64)) and not e["xw"][7:].any()


def test_finish_pose_discard_and_local_map():
    m = the_map([2, 0, 1, 1])
    mp, flags = [0, 1, -1, 2, 3, 3], [0, 0, 0, 1, 1, 0]

    def run(mode, **kw):
        fr = frame(mp)
        e = R.pose_edges(fr, m, np.ones(1, f32))
        res = dict(pose_R=e["pose_R"], pose_t=e["pose_t"], outlier=np.array([flags[i] for i in e["edge_kp"][:5]] + [0] * 3, np.uint8))
        return fr, R.finish_pose(fr, m, mode, e, res, **kw)

    fr, out = run(R.DISCARD)
    assert list(fr["frame_mappoint"][0, :6]) == [0, 1, -1, -1, -1, 3] and not fr["frame_outlier"][0, :6].any()
    assert out["n_inliers"][0] == 2 and list(out["discarded"][0, :2]) == [2, 3] and out["n_discarded"][0] == 2   # point 1: no obs
    m["mp_found"][:] = 0
    fr, out = run(R.LOCAL_MAP, localization=False, stereo=False)
    assert list(fr["frame_mappoint"][0, :6]) == mp and list(fr["frame_outlier"][0, :6]) == flags
    assert out["n_inliers"][0] == 2 and list(m["mp_found"]) == [1, 1, 0, 1]
    m["mp_found"][:] = 0
    fr, out = run(R.LOCAL_MAP, localization=True, stereo=True)
    assert list(fr["frame_mappoint"][0, :6]) == [0, 1, -1, -1, -1, 3] and list(fr["frame_outlier"][0, :6]) == flags
    assert out["n_inliers"][0] == 3 and list(m["mp_found"]) == [1, 1, 0, 1]


def test_pose_product_keeps_the_operand_order_and_the_zero_start():
    A = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], f32) / f32(7)
    B = np.array([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8], f32) / f32(3)
    C = R.pose_product(A, B)
    RA, RB = A[:9].reshape(3, 3), B[:9].reshape(3, 3)
    assert C[1] == f32(f32(f32(RA[0, 0] * RB[0, 1]) + f32(RA[0, 1] * RB[1, 1])) + f32(RA[0, 2] * RB[2, 1]))
    assert C[9] == f32(f32(f32(f32(RA[0, 0] * B[9]) + f32(RA[0, 1] * B[10])) + f32(RA[0, 2] * B[11])) + A[9])
    Z = R.pose_product(np.array([-0.0] * 9 + [-0.0] * 3, f32), np.abs(B))
    assert not np.signbit(Z[:9]).any() and np.signbit(Z[9:]).sum() == 0   # 0 + (-0) = +0; +0 + (-0) = +0
    assert R.pose_product(IDENT, B).tolist() == B.tolist()


def test_motion_is_forward_backward_or_neither():
    L = IDENT.copy()
    for tz, mono, want in ((-0.5, False, 1), (0.5, False, 2), (-0.05, False, 0), (-0.5, True, 0), (-0.08, False, 0)):
        V = IDENT.copy()
        V[11] = tz
        assert R.motion_of(L, R.pose_product(V, L), f32(0.08), mono) == want, tz


def test_motion_project_gates_and_the_one_step_replacement():
    m = the_map([1, 0, 1, 1, 1, 1], replaced=[-1, -1, 3, 4, -1, -1])
    m["mp_xw"][:] = [[0, 0, 5], [0.1, 0, 5], [0, 0, -5], [0, 0.1, 5], [90, 0, 5], [0, 0, 0]]
    last = frame([0, 1, 2, -1, 3, 0, 5, 9], outlier=[0, 0, 0, 0, 0, 1, 0, 0], octave=[1, 2, 3, 4, 5, 6, 7, 0])
    cur = frame([5, 5, 5])
    o = R.motion_project(cur, last, m, IDENT.reshape(1, 12), np.array([0.08], f32), False)
    assert list(last["frame_mappoint"][0, :8]) == [0, 1, 3, -1, 4, 0, 5, 9]   # 2 -> 3 (not on to 4), 3 -> 4
    assert list(cur["frame_mappoint"][0]) == [-1, -1, -1, 7, 7] and list(o["kp_claimed"][0]) == [0, 0, 0, 1, 1]
    # 0: in view; 1: in view, no observation; 3 (was 2): in view; null; 4: outside the image; an outlier; z = 0 -> u is NaN; 9: null
    assert list(o["mp_valid"][0, :8]) == [1, 1, 1, 0, 0, 0, 0, 0] and list(o["mp_has_obs"][0, :8]) == [1, 0, 1, 0, 1, 1, 1, 0]
    assert o["mp_proj"][0, 0].tolist() == [320, 240, 312] and list(o["mp_octave"][0, :8]) == [1, 2, 3, 4, 5, 6, 7, 0]
    assert np.array_equal(o["mp_desc"][0, 2], m["mp_desc"][3]) and not o["mp_desc"][0, 3].any()
    m["mp_xw"][0] = [0, 0, -0.0]   # z = -0.0 is not < 0: it goes on to the bounds test, where u = NaN fails
    assert R.project(IDENT, CAM, [0, 640, 0, 480], m["mp_xw"][0])[0] == 0
    assert R.project(IDENT, CAM, [0, 640, 0, 480], [-3.2, 0, 5])[:2] == (1, f32(0)) and R.project(IDENT, CAM, [0, 640, 0, 480], [3.2, 0, 5])[0] == 0


def test_end_frame_orders_the_score_before_the_clean():
    m = the_map([2, 0, 3, 1], bad=[0, 0, 1, 0], kf_n=[5, 2], kf_mappoint=[[0, 1, 2, 3, 9, 0], [3, -1, 0, 0, 0, 0]])
    fr = frame([0, 1, -1, 2, 1, 3], outlier=[0, 0, 0, 1, 1, 0], depth=[1.0, 2.0, 3.0, 4.0, 7.999, 8.0])
    nobs, counts = R.end_frame(fr, m, 8.0, np.array([0], np.int32), np.array([2], np.int32))
    assert list(nobs[0]) == [2, 0, -1, -1, -1, 1, -1, -1]                                   # point 1 scores its 0 before it goes
    assert list(fr["frame_mappoint"][0]) == [0, -1, -1, 2, -1, 3, 7, 7] and list(fr["frame_outlier"][0]) == [0, 0, 0, 1, 0, 0, 7, 7]
    assert list(counts[0]) == [1, 4, 1]   # close: 0 tracked; 1, 2, 3 (outlier), 4 not; depth 8.0 is not close.  Row 0: only point 0
    for min_obs, k, want in ((0, 0, 3), (-1, 0, 3), (1, 0, 2), (3, 0, 0), (1, 1, 1), (1, -1, 0), (1, 2, 0)):
        assert R.tracked_map_points(m, k, min_obs) == want, (min_obs, k)
    fr = frame([0], depth=[1.0])
    del fr["kp_depth"]
    assert list(R.end_frame(fr, m, 8.0, np.array([-1], np.int32), np.array([0], np.int32))[1][0]) == [0, 0, 0]


def test_drop_outliers():
    fr = frame([0, 1, -1, 2], outlier=[1, 0, 1, 0])
    R.drop_outliers(fr)
    assert list(fr["frame_mappoint"][0]) == [-1, 1, -1, 2, 7, 7] and list(fr["frame_outlier"][0, :4]) == [1, 0, 1, 0]


def stereo(depth, th, mode=R.KEYFRAME, mappoint=None, nobs=(1,)):
    fr = frame(mappoint if mappoint is not None else [-1] * len(depth), depth=depth)
    o = R.stereo_points(fr, the_map(list(nobs)), mode, th)
    return fr, o, list(o["created_kp"][0, :o["n_created"][0]])


def test_stereo_points_limits():
    assert stereo([0.0, -1.0, np.nan, -0.0], 5.0)[1]["n_processed"][0] == 0                       # no Z > 0
    for n in (99, 100, 101):                                                                    # all close: all processed
        d = np.linspace(1, 4, n)[::-1].astype(f32)
        _, o, made = stereo(d, 5.0)
        assert o["n_processed"][0] == n and made == list(range(n))[::-1]
    d = np.concatenate([np.linspace(1, 4, 99), [6.0, 7.0, 8.0]]).astype(f32)                    # rank 99 far: not the 101st yet
    assert stereo(d, 5.0)[1]["n_processed"][0] == 101                                           # rank 100 far: the loop leaves there
    d = np.concatenate([np.linspace(1, 4, 100), [6.0, 7.0]]).astype(f32)
    assert stereo(d, 5.0)[1]["n_processed"][0] == 101
    d = np.concatenate([np.linspace(1, 4, 101), [6.0, 7.0]]).astype(f32)                        # rank 101 is the first far one
    assert stereo(d, 5.0)[1]["n_processed"][0] == 102
    d = np.concatenate([np.linspace(1, 4, 100), [5.0, 5.0, 6.0]]).astype(f32)                   # Z == th_depth is not far
    assert stereo(d, 5.0)[1]["n_processed"][0] == 103
    d = np.concatenate([np.linspace(6, 9, 150)]).astype(f32)                                    # all far: the 100 closest and one
    assert stereo(d, 5.0)[1]["n_processed"][0] == 101


def test_stereo_points_order_and_edge_values():
    _, o, made = stereo([3.0, 2.0, 3.0, 2.0, 1.0], 5.0)
    assert made == [4, 1, 3, 0, 2]                                                              # equal depths by index
    _, o, made = stereo([np.inf, np.nan, -0.0, 1e-42, 2.0, 0.0], 5.0)
    assert made == [3, 4, 0] and o["n_processed"][0] == 3                                       # a denormal is > 0; +inf stays in
    assert not np.isfinite(o["created_xw"][0, 2]).any()                                         # (0 * inf in the rotation)
    _, o, made = stereo([3.0, 0.0, 1.0, 2.0], 5.0, R.INIT, mappoint=[0, 0, 0, -1])
    assert made == [0, 2, 3] and o["n_processed"][0] == 3                                       # keypoint order, map point or not


@pytest.mark.parametrize("mode", [R.KEYFRAME, R.VO, R.INIT])
def test_stereo_points_a_point_without_observations(mode):
    fr, o, made = stereo([2.0, 1.0, 3.0, 4.0], 5.0, mode, mappoint=[0, 1, -1, 7], nobs=(0, 2))
    if mode == R.INIT:
        assert made == [0, 1, 2, 3] and list(fr["frame_mappoint"][0, :4]) == [0, 1, -1, 7]
    else:
        assert made == [0, 2, 3]                                                                # 1 has observations; 7 is no slot
        assert list(fr["frame_mappoint"][0, :4]) == ([-1, 1, -1, 7] if mode == R.KEYFRAME else [0, 1, -1, 7])
    assert np.array_equal(o["created_xw"][0, made.index(0)], R.unproject(IDENT, CAM, 0, 0, 2.0, vo=mode == R.VO))
    # the two operand orders, at a keypoint and depth where they round differently
    u, v, Z = f32(123.456), f32(77.7), f32(3.3333)
    invf = f32(1) / f32(500)
    first = [f32(f32(invf * f32(u - f32(320))) * Z), f32(f32(invf * f32(v - f32(240))) * Z)]      # uvZToCamera
    second = [f32(f32(f32(u - f32(320)) * Z) * invf), f32(f32(f32(v - f32(240)) * Z) * invf)]     # UnprojectStereo
    assert first != second
    for vo, xy in ((False, first), (True, second)):
        xw = R.unproject(IDENT, CAM, u, v, Z, vo=vo)
        assert [xw[0], xw[1], xw[2]] == xy + [Z], vo                                                # identity pose: Xw = Xc
