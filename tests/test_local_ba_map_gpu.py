"""LocalBundleAdjustment on the device-resident map (orbba_local_window / orbba_local_ba_apply / orbba_local_ba_map) against
tests/local_ba_window_ref.py on the maps of tests/local_ba_map_cases.py and the hand-built map: the window through the host
and the device entries (floats as bits), the write-back on planted flags, and the whole call against orbba_local_ba on the
restatement's flattened problem with its outputs applied by the restatement."""
import ctypes

import numpy as np
import pytest

import local_ba_map_cases as LC
import local_ba_window_ref as WR
from orb_slam2_refactored_amd import optimizer as O
from test_local_ba_window_ref import hand_map

pytestmark = pytest.mark.gpu

MAPS = ["hand", "small", "large"]


def the_map(name):
    return (hand_map(), 3) if name == "hand" else LC.case(name)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def to_device(t):
    import torch
    out = {}
    for k, v in t.items():
        if k in O.WINDOW_HOST_KEYS:
            out[k] = v
        elif k == "kf_keypoint":
            out[k] = torch.from_numpy(np.ascontiguousarray(v).view(np.float32).reshape(v.shape + (7,)).copy()).cuda()
        else:
            out[k] = torch.from_numpy(np.array(v)).cuda()
    return out


def assert_window(got, want, n_total=None):
    c = [int(x) for x in np.asarray(got["counts"])[:6]]
    assert tuple(c[:4]) == want["counts"] and c[4] == want["status"]
    if want["status"] != WR.OK:
        return
    assert c[5] == want["one_cam"]
    for k in WR.WINDOW_ARRAYS:
        w = want[k].reshape(-1)
        assert np.array_equal(bits(np.asarray(got[k]).reshape(-1)[:len(w)]), bits(w)), k


@pytest.mark.parametrize("name", MAPS)
def test_window_host_and_device_entries_equal_the_restatement(name):
    t, cur = the_map(name)
    want = WR.gather(t, cur)
    assert_window(O.LocalWindow(t, cur), want)
    d = to_device(t)
    w1 = {k: v.cpu().numpy() for k, v in O.local_window_device(d, cur).items()}
    assert_window(w1, want)
    w2 = {k: v.cpu().numpy() for k, v in O.local_window_device(d, cur).items()}
    n = {"pose": sum(want["counts"][:2]), "point": want["counts"][2], "edge": want["counts"][3]}
    for k, (_, cap, width) in O.WINDOW_KEYS.items():         # a rerun is byte-identical
        m = 8 if cap is None else n[cap[:-1]] * width
        assert w1[k][:m].tobytes() == w2[k][:m].tobytes(), k


def test_window_capacities_one_short_overflow_and_write_nothing():
    t, cur = the_map("small")
    want = WR.gather(t, cur)
    full = (sum(want["counts"][:2]), want["counts"][2], want["counts"][3])
    for short in range(3):
        caps = dict(zip(("poses", "points", "edges"), [c - (i == short) for i, c in enumerate(full)]))
        win = O.new_window(caps)
        for v in win.values():
            v[...] = 77
        got = O.LocalWindow(t, cur, caps=caps, window=win)
        assert_window(got, WR.gather(t, cur, tuple(caps.values())))
        assert got["counts"][4] == O.WINDOW_OVERFLOW and all((v == 77).all() for k, v in got.items() if k != "counts")
    assert O.LocalWindow(t, cur, caps=dict(zip(("poses", "points", "edges"), full)))["counts"][4] == O.WINDOW_OK


def test_entries_outside_their_tables_stay_harmless():
    import torch
    t, cur = LC.dirty("small")
    want = WR.gather(t, cur)
    d = to_device(t)
    got = {k: v.cpu().numpy() for k, v in O.local_window_device(d, cur).items()}
    torch.cuda.synchronize()
    assert_window(got, want)
    from orb_slam2_refactored_amd._lib import OrbError
    with pytest.raises(OrbError, match="status -1"):
        O.LocalWindow(t, cur)                                # the host entry refuses such tables (test_local_ba_map_validation.py)


def planted(want, seed):
    rng = np.random.default_rng(seed)
    P, N, E = sum(want["counts"][:2]), want["counts"][2], want["counts"][3]
    outlier = (rng.random(E) < 0.15).astype(np.uint8)
    return outlier, rng.normal(size=(P, 9)), rng.normal(size=(P, 3)), rng.normal(size=(N, 3)) * 10


@pytest.mark.parametrize("name", MAPS)
def test_write_back_on_planted_flags_equals_the_restatement(name):
    import torch
    t, cur = the_map(name)
    want_w = WR.gather(t, cur)
    outlier, R, tr, X = planted(want_w, 11)
    if name == "hand":
        outlier[:] = 0
        outlier[[1, 2, 3, 6]] = 1
    want = WR.apply(t, want_w, outlier, R, tr, X)
    assert want["mp_bad"].sum() > t["mp_bad"].sum() and (want["mp_ref_kf"] != t["mp_ref_kf"]).any()
    win = O.LocalWindow(t, cur)
    got = O.LocalBAApply(t, win, outlier, R, tr, X)
    for k in WR.UPDATED:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    d = to_device(t)
    dwin = O.local_window_device(d, cur)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    pad = lambda a, n: np.concatenate([np.asarray(a).reshape(-1), np.zeros(n, np.asarray(a).dtype)])   # noqa: E731
    caps = O._window_given_caps(dwin)
    O.local_ba_apply_device(d, dwin, dev(pad(outlier, caps["edges"])), dev(pad(R, 9 * caps["poses"])), dev(pad(tr, 3 * caps["poses"])),
                            dev(pad(X, 3 * caps["points"])))
    for k in WR.UPDATED:
        assert np.array_equal(bits(d[k].cpu().numpy()), bits(want[k])), k


def expected_whole(t, cur, **kw):
    w = WR.gather(t, cur)
    out = O.LocalBundleAdjustment(WR.flatten(t, w), **kw)
    return w, out, WR.apply(t, w, out["edge_outlier"], out["pose_R"], out["pose_t"], out["points"])


@pytest.mark.parametrize("name", ["small", "large"])
def test_whole_call_equals_local_ba_on_the_flattened_window(name):
    t, cur = the_map(name)
    w, out, want = expected_whole(t, cur)
    assert out["ran"] and out["edge_outlier"].sum() > 0
    got, res = O.LocalBundleAdjustmentMap(t, cur)
    assert res["iterations"] == out["iterations"] and res["ran"] and res["status"] == O.WINDOW_OK and res["counts"] == w["counts"]
    assert np.array_equal(got["mp_obs_kf"] == -1, want["mp_obs_kf"] == -1)   # the outlier set
    for k in WR.UPDATED:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    d = to_device(t)
    res_d, _ = O.local_ba_map_device(d, cur)
    assert res_d["iterations"] == out["iterations"] and res_d["chi2"] == out["chi2"]
    for k in WR.UPDATED:
        assert np.array_equal(bits(d[k].cpu().numpy()), bits(want[k])), k


def test_stop_flag_at_entry_leaves_every_table():
    t, cur = the_map("small")
    d = to_device(t)
    res, _ = O.local_ba_map_device(d, cur, stop_flag=ctypes.c_int32(1))
    assert not res["ran"] and res["status"] == O.WINDOW_OK
    for k, v in t.items():
        if k not in O.WINDOW_HOST_KEYS and k != "kf_keypoint":
            assert d[k].cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes(), k


def test_debug_stop_after_the_first_trials_still_classifies_and_applies(monkeypatch):
    t, cur = the_map("small")
    monkeypatch.setenv("ORBBA_DEBUG_STOP_AFTER_TRIALS", "2")
    w, out, want = expected_whole(t, cur)
    assert out["ran"] and out["iterations"][1] == 0
    got, res = O.LocalBundleAdjustmentMap(t, cur)
    assert res["iterations"] == out["iterations"] and res["ran"]
    for k in WR.UPDATED:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert (got["kf_pose"] != t["kf_pose"]).any()


def chain_tables():
    """test_observe_gpu's chain map with what LocalBundleAdjustment reads besides: a camera, keypointsUn at the projection of
    the point each cell holds (where it lies in front of the keyframe), and the pyramid's tables."""
    from test_observe_gpu import chain_case
    c, t, fr, cur, item_kf, point, b = chain_case()
    from orb_slam2_refactored_amd import KP_DTYPE
    K, kf_cap = t["kf_mappoint"].shape
    scale = np.asarray(c["keypoints"]["scale_factors"], np.float32)
    cam = np.array([500, 500, 320, 240, 40, 0.08], np.float32)
    kp = np.zeros((K, kf_cap), KP_DTYPE)
    kp["x"], kp["y"], kp["octave"] = 320, 240, t["kf_kp_octave"]
    for k in range(K):
        R, tr = t["kf_pose"][k, :9].reshape(3, 3).astype(np.float64), t["kf_pose"][k, 9:].astype(np.float64)
        for i in np.flatnonzero(t["kf_mappoint"][k] >= 0):
            xc = R @ t["mp_xw"][t["kf_mappoint"][k, i]].astype(np.float64) + tr
            if xc[2] > 0.5:
                kp[k, i]["x"], kp[k, i]["y"] = cam[0] * xc[0] / xc[2] + cam[2], cam[1] * xc[1] / xc[2] + cam[3]
    t = dict(t, kf_keypoint=kp, kf_camera=np.tile(cam, (K, 1)), scale_factors=scale,
             inv_sigma2=(1 / (scale.astype(np.float64) ** 2)).astype(np.float32))
    return c, t, fr, cur, item_kf, point, b


def test_the_chain_on_one_stream_equals_the_restatements_in_the_same_order():
    """fuse_apply_device -> update_connections_device -> local_ba_map_device -> keyframe_culling_device -> the compaction and
    the live children -> TrackLocalMap on one stream with nothing copied between the steps, against observe_ref ->
    map_maintenance_ref -> this file's whole-call expectation -> culling_ref -> local_map_ref.  The local BA starts behind
    what the stream holds, and the cull enqueued behind it sees the applied tables."""
    import torch
    import culling_cases as CC
    import culling_ref as CR
    import fuse_ref
    import local_map_ref as LR
    import map_maintenance_cases as MC
    import map_maintenance_ref as MR
    import observe_cases as OC
    import observe_ref as OR
    from orb_slam2_refactored_amd import culling as CU
    from orb_slam2_refactored_amd import map_maintenance as MM
    from orb_slam2_refactored_amd import observations as OB
    from orb_slam2_refactored_amd.local_map import OUT_KEYS, LocalMap
    c, t, fr, cur, item_kf, point, b = chain_tables()
    best_idx = fuse_ref.fuse(b)[0]
    # the restatements, chained
    r = OR.fuse_apply({k: t[k] for k in OC.TABLES}, OR.FUSE, item_kf, b["mp_begin"], point, best_idx)
    assert r["status"] == OR.OK and len(r["touched"]) >= 10
    after = dict(t, **{k: r[k] for k in OR.UPDATED})
    conn = MR.update_connections({k: after[k] for k in MC.GRAPH}, [int(k) for k in item_kf])
    assert (conn["status"] == 0).all()
    after.update({k: conn[k] for k in MR.STATE_KEYS})
    w, out, ba = expected_whole(after, cur)
    assert out["ran"] and 0 < out["edge_outlier"].sum() and w["counts"][1] > 0
    after.update(ba)
    cull, culled, n, _ = CR.keyframe_culling({k: after[k] for k in CC.TABLES}, cur, True, CC.TH_DEPTH)
    after.update(cull)
    packed = dict(after)
    packed["mp_obs_off"], kf, idx = CR.compact_observations(after["mp_obs_off"], after["mp_obs_kf"], after["mp_obs_idx"])
    packed["mp_obs_kf"], packed["mp_obs_idx"] = kf[:packed["mp_obs_off"][-1]], idx[:packed["mp_obs_off"][-1]]
    off, kids = CR.live_children(after["kf_parent"], after["kf_bad"])
    packed.update(kf_child_off=off, kf_child_idx=kids if len(kids) else np.zeros(1, np.int32))
    want = LR.track_local_map({k: v.copy() for k, v in packed.items() if k != "kf_keypoint"},
                              {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fr.items()}, c["mp_cap"])
    # the device chain
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()   # noqa: E731
    dt = dict(to_device({k: v for k, v in t.items() if isinstance(v, np.ndarray)}), **{k: v for k, v in t.items() if not isinstance(v, np.ndarray)})
    dfr = {k: (up(v) if isinstance(v, np.ndarray) else v) for k, v in fr.items()}
    d_item, d_begin, d_point, d_best = up(item_kf), up(b["mp_begin"]), up(point), up(best_idx)
    window = O.new_window(dict(zip(("poses", "points", "edges"), (sum(w["counts"][:2]), w["counts"][2], w["counts"][3]))), "cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        st = OB.fuse_apply_device(dt, OB.APPLY_FUSE, d_item, d_begin, d_point, d_best, stream=s)
        status = MM.update_connections_device(dt, d_item, stream=s)
        res, _ = O.local_ba_map_device(dt, cur, window=window, stream=s)
        got_culled, got_n, _ = CU.keyframe_culling_device(dt, cur, True, CC.TH_DEPTH, stream=s)
        dp = dict(dt)
        dp["mp_obs_off"], dp["mp_obs_kf"], dp["mp_obs_idx"] = CU.compact_observations_device(dt["mp_obs_off"], dt["mp_obs_kf"],
                                                                                              dt["mp_obs_idx"], stream=s)
        dp["kf_child_off"], dp["kf_child_idx"] = CU.live_children_device(dt["kf_parent"], dt["kf_bad"], stream=s)
        track = LocalMap(dp).track_local_map_device(dfr, c["mp_cap"], votes=True, stream=s)
    s.synchronize()
    assert int(st["status"].cpu()[0]) == OB.OK and (status.cpu().numpy() == 0).all()
    assert res["status"] == O.WINDOW_OK and res["ran"] and res["iterations"] == out["iterations"] and res["counts"] == w["counts"]
    assert int(got_n.cpu()[0]) == n and np.array_equal(got_culled.cpu().numpy(), culled)
    for k in set(OR.UPDATED + WR.UPDATED + MR.STATE_KEYS + CR.KEYFRAME_UPDATED) - {"mp_visible"}:
        assert np.array_equal(bits(dt[k].cpu().numpy()), bits(after[k])), k
    for k in ("mp_obs_off", "mp_obs_kf", "mp_obs_idx"):
        m = len(packed[k])
        assert np.array_equal(dp[k].cpu().numpy()[:m], packed[k]), k
    for k in OUT_KEYS:
        assert np.array_equal(bits(track[k].cpu().numpy()), bits(want[k])), k
