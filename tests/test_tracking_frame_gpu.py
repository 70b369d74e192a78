"""Tracking's per-frame state on the GPU (orbtf_*, orb_slam2_refactored_amd/tracking.py) against the sequential restatement
tests/tracking_frame_ref.py, through the host entries (clean cases) and the device entries (cases with entries outside their
tables): every output and every updated table identical, floats compared as bits, no tolerance.  A batch of 5 equals its
frames run one at a time with mp_found carried along; a rerun is byte-identical.  Chain A (TrackLocalMap) and chain B
(TrackWithMotionModel) run on one stream with nothing copied in between and are compared with the restatement chain run with
the oracle's searches and PoseOptimization; stereo_points(KEYFRAME) follows chain A."""
import numpy as np
import pytest

import local_map_cases as LC
import tracking_frame_cases as TC
import tracking_frame_ref as R
from orb_slam2_refactored_amd import tracking as T

pytestmark = pytest.mark.gpu

PATHS = ("host", "device")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        a, b = a.view(np.uint32 if a.dtype == np.float32 else np.uint64), b.view(np.uint32 if b.dtype == np.float32 else np.uint64)
    return np.array_equal(a, b)


def put(d, on_device):
    """numpy copies, or CUDA tensors of them."""
    if not on_device:
        return {k: (np.ascontiguousarray(v).copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    import torch
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def get(d):
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in d.items() if hasattr(v, "shape")}


def one(a, on_device):
    return put({"a": a}, on_device)["a"]


def zeros(keys, d, on_device):
    return put({k: np.zeros(T._shape(sp, d), dt) for k, (dt, sp) in keys.items()}, on_device)


def the_case(name, path):
    c = TC.case(name)
    return TC.dirty(c) if path == "device" else c


def assert_all_same(got, want, what=""):
    for k, w in want.items():
        assert same(got[k], w), (what, k)


# ---- one runner per entry: (library result, restatement result), each a dict of outputs and updated tables
def run_apply(c, dev, mode, by_row):
    fr = put(c["frames"], dev)
    rfr, _ = TC.ref_frames(c)
    M = len(c["map"]["mp_nobs"])
    row = c["src_row"] if by_row else None
    T.apply_matches(fr, mode, one(c["kp_match"], dev), one(c["src"], dev), M, src_row=None if row is None else one(row, dev))
    R.apply_matches(rfr, mode, c["kp_match"], c["src"], row, M)
    return {"frame_mappoint": get(fr)["frame_mappoint"]}, {"frame_mappoint": rfr["frame_mappoint"]}


def run_edges(c, dev):
    fr, m = put(c["frames"], dev), put(c["map"], dev)
    rfr, rm = TC.ref_frames(c)
    out = T.pose_edges(fr, m, one(c["inv_sigma2"], dev), out=zeros(T.EDGE_KEYS, T._dims(c["frames"], c["map"]), dev))
    want = R.pose_edges(rfr, rm, c["inv_sigma2"])
    return dict(get(out), frame_outlier=get(fr)["frame_outlier"]), dict(want, frame_outlier=rfr["frame_outlier"])


def run_finish(c, dev, mode, localization=False, stereo=False, mp_found=None):
    rfr, rm = TC.ref_frames(c)
    if mp_found is not None:
        rm["mp_found"] = mp_found.copy()
    edges = R.pose_edges(rfr, rm, c["inv_sigma2"])
    result = TC.fake_result(edges, c["seed"], c.get("frame_ids"))
    if dev and len(c["frames"]["frame_n"]) > 1:   # an edge that names a keypoint outside its frame is skipped
        edges["edge_kp"][edges["edge_begin"][1]:edges["edge_begin"][1] + 2] = (-1, 1 << 20)
    fr, m = put(rfr, dev), put(rm, dev)
    out = T.finish_pose(fr, m, mode, put(edges, dev), put(result, dev), localization, stereo,
                        out=zeros(T.FINISH_KEYS, T._dims(rfr, rm), dev))
    want = R.finish_pose(rfr, rm, mode, edges, result, localization, stereo)
    keys = ("frame_mappoint", "frame_outlier", "pose")
    got = dict(get(out), mp_found=get(m)["mp_found"], **{k: get(fr)[k] for k in keys})
    if mode == T.LOCAL_MAP:
        want = {"n_inliers": want["n_inliers"]}
    return got, dict(want, mp_found=rm["mp_found"], **{k: rfr[k] for k in keys})


def run_motion(c, dev, monocular=False):
    last0 = c["last"] if "last" in c else TC.last_frames(c["name"])
    if dev:
        last0 = dict(last0, frame_mappoint=c["frames"]["frame_mappoint"], kp_octave=c["frames"]["kp_octave"])   # the dirty ones
    cur, last, m = put(c["frames"], dev), put(last0, dev), put(c["map"], dev)
    rcur, rm = TC.ref_frames(c)
    rlast = TC.copy(last0)
    d = T._dims(c["frames"], c["map"])
    d["last_cap"] = d["kp_cap"]
    out = T.motion_project(cur, last, m, one(c["velocity"], dev), one(c["baseline"], dev), monocular, out=zeros(T.MOTION_KEYS, d, dev))
    want = R.motion_project(rcur, rlast, rm, c["velocity"], c["baseline"], monocular)
    got = dict(get(out), pose=get(cur)["pose"], frame_mappoint=get(cur)["frame_mappoint"], last_mappoint=get(last)["frame_mappoint"])
    return got, dict(want, pose=rcur["pose"], frame_mappoint=rcur["frame_mappoint"], last_mappoint=rlast["frame_mappoint"])


def run_end(c, dev, depth=True):
    frames = c["frames"] if depth else {k: v for k, v in c["frames"].items() if k != "kp_depth"}
    fr, m = put(frames, dev), put(c["map"], dev)
    rfr, rm = TC.copy(frames), TC.copy(c["map"])
    out = T.end_frame(fr, m, TC.TH_DEPTH, one(c["reference_kf"], dev), one(c["min_obs"], dev))
    nobs, counts = R.end_frame(rfr, rm, TC.TH_DEPTH, c["reference_kf"], c["min_obs"])
    keys = ("frame_mappoint", "frame_outlier")
    return (dict(get(out), **{k: get(fr)[k] for k in keys}),
            dict(n_observations=nobs, counts=counts, **{k: rfr[k] for k in keys}))


def run_drop(c, dev):
    fr = put(c["frames"], dev)
    rfr, _ = TC.ref_frames(c)
    T.drop_outliers(fr)
    R.drop_outliers(rfr)
    return {"frame_mappoint": get(fr)["frame_mappoint"]}, {"frame_mappoint": rfr["frame_mappoint"]}


def run_stereo(c, dev, mode, th=TC.TH_DEPTH):
    fr, m = put(c["frames"], dev), put(c["map"], dev)
    rfr, rm = TC.ref_frames(c)
    out = T.stereo_points(fr, m, mode, th, out=zeros(T.CREATED_KEYS, T._dims(c["frames"], c["map"]), dev))
    want = R.stereo_points(rfr, rm, mode, th)
    return dict(get(out), frame_mappoint=get(fr)["frame_mappoint"]), dict(want, frame_mappoint=rfr["frame_mappoint"])


ALL = tuple(TC.CASES)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ALL)
def test_apply_matches_pose_edges_end_frame_and_drop_outliers_equal_the_restatement(name, path):
    c, dev = the_case(name, path), path == "device"
    for mode in (T.MERGE, T.REPLACE):
        for by_row in (False, True):
            assert_all_same(*run_apply(c, dev, mode, by_row), what=("apply", mode, by_row))
    got, want = run_edges(c, dev)
    assert_all_same(got, want, "pose_edges")
    assert_all_same(*run_end(c, dev), what="end_frame")
    assert_all_same(*run_end(c, dev, depth=False), what="end_frame without depth")
    assert_all_same(*run_drop(c, dev), what="drop_outliers")
    if max(TC.CASES[name]) >= 63:
        assert want["edge_begin"][-1] > 10
    if name == TC.FULL:   # the whole row became edges: two compaction steps in which every lane takes
        assert list(want["edge_begin"]) == [0, 512] and np.array_equal(want["edge_kp"][:512], np.arange(512))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ALL)
def test_finish_pose_and_motion_project_equal_the_restatement(name, path):
    c, dev = the_case(name, path), path == "device"
    assert_all_same(*run_finish(c, dev, T.DISCARD), what="finish DISCARD")
    for localization, stereo in ((False, False), (True, True)):
        assert_all_same(*run_finish(c, dev, T.LOCAL_MAP, localization, stereo), what=("finish LOCAL_MAP", localization, stereo))
    for monocular in (False, True):
        got, want = run_motion(c, dev, monocular)
        assert_all_same(got, want, ("motion_project", monocular))
    if len(TC.CASES[name]) > 1:
        assert set(want["motion"]) == {0} and {1, 2} <= set(run_motion(c, dev)[1]["motion"])
    if max(TC.CASES[name]) >= 257:
        assert want["mp_valid"].sum() > 10 and (want["last_mappoint"] != c["frames"]["frame_mappoint"]).any()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ALL)
def test_stereo_points_equals_the_restatement(name, path):
    c, dev = the_case(name, path), path == "device"
    for mode in (T.KEYFRAME, T.VO, T.INIT):
        got, want = run_stereo(c, dev, mode)
        assert_all_same(got, want, ("stereo_points", mode))
    if name == "lds":
        assert want["n_processed"][0] > 3000 and c["frames"]["frame_n"][0] == c["frames"]["frame_mappoint"].shape[1] == T.MAX_KP


PER_EDGE = ("xw", "obs", "inv_sigma2", "edge_kp")
NOT_PER_FRAME = ("kp_begin", "mp_begin", "edge_begin", "mp_found")


def assert_frame_in_batch(one, five, f, what):
    """Every output and updated table of frame f run alone equals its part of the batch's (the edges re-based)."""
    for k, v in one.items():
        if k in NOT_PER_FRAME:
            continue
        if k in PER_EDGE:
            e0, e1 = five["edge_begin"][f], five["edge_begin"][f + 1]
            assert one["edge_begin"][1] == e1 - e0 and same(v[:e1 - e0], five[k][e0:e1]), (what, k, f)
        else:
            assert same(v[0], five[k][f]), (what, k, f)


@pytest.mark.parametrize("name", TC.BATCH_CASES)
def test_a_batch_of_five_equals_its_frames_one_at_a_time_and_a_rerun(name):
    c = TC.case(name)
    runs = {"apply MERGE": (run_apply, (T.MERGE, True)), "apply REPLACE": (run_apply, (T.REPLACE, True)), "pose_edges": (run_edges, ()),
            "finish DISCARD": (run_finish, (T.DISCARD,)), "finish LOCAL_MAP": (run_finish, (T.LOCAL_MAP, True, True)),
            "motion_project": (run_motion, ()), "end_frame": (run_end, ()), "drop_outliers": (run_drop, ()),
            "stereo KEYFRAME": (run_stereo, (T.KEYFRAME,)), "stereo VO": (run_stereo, (T.VO,))}
    for what, (run, args) in runs.items():
        five, again = run(c, False, *args)[0], run(c, False, *args)[0]
        assert_all_same(again, five, ("rerun", what))
        found = c["map"]["mp_found"].copy()
        for f in range(5):
            kw = dict(mp_found=found) if run is run_finish else {}
            one = run(TC.one_frame(c, f), False, *args, **kw)[0]
            assert_frame_in_batch(one, five, f, what)
            found = one.get("mp_found", found)   # carried along
        if what == "finish LOCAL_MAP":
            assert same(found, five["mp_found"]) and (found != c["map"]["mp_found"]).any()


def chain_a_inputs():
    """The "mixed" local-map case with stereo observations that agree with the map, and the tables the new entries add."""
    c = LC.case("mixed")
    m, fr, kp = LC.batch(c, 5)
    rng = np.random.default_rng(7)
    M = len(m["mp_bad"])
    kp["kp_uright"], depth = TC.consistent_stereo(dict(fr, kp_xy=kp["kp_xy"]), m, rng)
    extra = dict(frame_outlier=np.zeros_like(kp["kp_octave"], dtype=np.uint8),
                 kp_depth=np.where(depth > 0, depth, rng.uniform(1, 20, depth.shape)).astype(np.float32),
                 kp_angle=rng.uniform(0, 360, depth.shape).astype(np.float32))
    mp = dict(mp_found=rng.integers(0, 30, M).astype(np.int32), mp_replaced=np.full(M, -1, np.int32))
    inv_sigma2 = (1.0 / kp["scale_factors"].astype(np.float32) ** 2).astype(np.float32)
    return c, m, fr, kp, extra, mp, inv_sigma2


def frames_of(fr, kp, extra):
    return dict({k: fr[k] for k in ("frame_n", "frame_mappoint", "pose", "camera", "bounds")},
                **{k: kp[k] for k in ("kp_xy", "kp_octave", "kp_uright", "kp_desc")}, **extra)


def oracle_local_search(oracle, want, fr, kp, mp_cap, th):
    """The oracle's SearchByProjection on the restatement's local-map arrays, frame by frame without the padding."""
    from orb_slam2_refactored_amd.local_map import OUT_KEYS, LocalMap
    F, cap = fr["frame_mappoint"].shape
    km = np.full((F, cap), -1, np.int32)
    for f in range(F):
        n = int(fr["frame_n"][f])
        hb = LocalMap.projection_batch({k: want[k][f:f + 1] for k in OUT_KEYS},
                                       {k: (v[f:f + 1] if k != "scale_factors" else v) for k, v in kp.items()}, kp["scale_factors"], th=th)
        for k in ("kp_xy", "kp_octave", "kp_uright", "kp_desc", "kp_claimed"):
            hb[k] = np.ascontiguousarray(hb[k][:n])
        hb["kp_begin"], hb["mp_begin"] = np.array([0, n], np.int32), np.array([0, mp_cap], np.int32)
        km[f, :n] = oracle.search_by_projection(hb)[0][:n]
    return km


def test_chain_a_track_local_map_on_one_stream(oracle):
    import torch
    from orb_slam2_refactored_amd.local_map import LocalMap
    from orb_slam2_refactored_amd.matcher import search_by_projection_device
    from orb_slam2_refactored_amd.optimizer import pose_optimization_device
    c, m, fr, kp, extra, mp, inv_sigma2 = chain_a_inputs()
    F, th = 5, 3.0
    K = len(m["kf_bad"])
    rng = np.random.default_rng(8)
    min_obs = rng.integers(0, 4, F).astype(np.int32)
    # ---- the restatement chain
    want = LC.R.track_local_map({k: v.copy() for k, v in m.items()}, {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fr.items()},
                                c["mp_cap"])
    rfr = TC.copy(frames_of(dict(fr, frame_mappoint=want["frame_mappoint"]), kp, extra))
    rm = dict({k: m[k] for k in ("mp_xw", "mp_bad", "mp_nobs", "mp_desc", "kf_n", "kf_mappoint")}, **TC.copy(mp))
    km = oracle_local_search(oracle, want, fr, kp, c["mp_cap"], th)
    R.apply_matches(rfr, R.MERGE, km, want["local_mp"], None, len(m["mp_bad"]))
    redges = R.pose_edges(rfr, rm, inv_sigma2)
    E = int(redges["edge_begin"][-1])
    ores = oracle.pose_optimization({k: (v[:E] if k in ("xw", "obs", "inv_sigma2") else v) for k, v in redges.items() if k != "edge_kp"})
    rfin = R.finish_pose(rfr, rm, R.LOCAL_MAP, redges, ores, localization=False, stereo=True)
    rnobs, rcounts = R.end_frame(rfr, rm, TC.TH_DEPTH, want["reference_kf"], min_obs)
    R.drop_outliers(rfr)
    rpts = R.stereo_points(rfr, rm, R.KEYFRAME, TC.TH_DEPTH)
    # ---- the device chain: nothing copied between the calls
    dm, dfr, dkp = put(m, True), put({k: v for k, v in fr.items() if isinstance(v, np.ndarray)}, True), put(kp, True)
    dfr.update({k: v for k, v in fr.items() if not isinstance(v, np.ndarray)})
    dkp["scale_factors"] = kp["scale_factors"]
    tfr = frames_of(dfr, dkp, put(extra, True))
    tm = dict({k: dm[k] for k in ("mp_xw", "mp_bad", "mp_nobs", "mp_desc", "kf_n", "kf_mappoint")}, **put(mp, True))
    d_min_obs, d_table = one(min_obs, True), one(inv_sigma2, True)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        res = LocalMap(dm).track_local_map_device(dfr, c["mp_cap"], stream=s)
        b = LocalMap.projection_batch(res, dkp, kp["scale_factors"], th=th)
        kp_match, _ = search_by_projection_device(b, stream=s)
        T.apply_matches(tfr, T.MERGE, kp_match, res["local_mp"], len(m["mp_bad"]), stream=s)
        edges = T.pose_edges(tfr, tm, d_table, stream=s)
        po = pose_optimization_device(edges, stream=s)
        fin = T.finish_pose(tfr, tm, T.LOCAL_MAP, edges, po, localization=False, stereo=True, stream=s)
        end = T.end_frame(tfr, tm, TC.TH_DEPTH, res["reference_kf"], d_min_obs, stream=s)
        T.drop_outliers(tfr, stream=s)
        pts = T.stereo_points(tfr, tm, T.KEYFRAME, TC.TH_DEPTH, stream=s)
    s.synchronize()
    g, ge, gpo = get(tfr), get(edges), get(po)
    assert E > 100 and ge["edge_begin"][-1] == E
    for k in ("edge_begin", "pose_R", "pose_t", "cam"):
        assert same(ge[k], redges[k]), k
    for k in ("xw", "obs", "inv_sigma2", "edge_kp"):
        assert same(ge[k][:E], redges[k][:E]), k
    assert same(gpo["outlier"][:E], ores["outlier"]) and 0 < ores["outlier"].sum() < E
    assert np.abs(gpo["pose_t"] - ores["pose_t"]).max() < 1e-6 and np.abs(gpo["pose_R"] - ores["pose_R"]).max() < 1e-6
    assert same(g["pose"], np.concatenate([gpo["pose_R"], gpo["pose_t"]], 1).astype(np.float32))
    assert same(g["frame_mappoint"], rfr["frame_mappoint"]) and same(g["frame_outlier"], rfr["frame_outlier"])
    assert same(get(fin)["n_inliers"], rfin["n_inliers"]) and rfin["n_inliers"].sum() > 100
    assert same(get(tm)["mp_found"], rm["mp_found"]) and (rm["mp_found"] != mp["mp_found"]).any()
    assert same(get(end)["counts"], rcounts) and same(get(end)["n_observations"], rnobs) and K > 0
    gp = get(pts)
    assert same(gp["n_created"], rpts["n_created"]) and same(gp["n_processed"], rpts["n_processed"]) and rpts["n_created"].sum() > 50
    for f in range(F):
        n = rpts["n_created"][f]
        assert same(gp["created_kp"][f, :n], rpts["created_kp"][f, :n]) and same(gp["created_xw"][f, :n], rpts["created_xw"][f, :n]), f


def test_chain_b_track_with_motion_model_on_one_stream(oracle):
    import torch
    from orb_slam2_refactored_amd.matcher import search_by_projection_motion_device
    from orb_slam2_refactored_amd.optimizer import pose_optimization_device
    c, m, fr, kp, extra, mp, inv_sigma2 = chain_a_inputs()
    F, th = 5, 7.0
    rng = np.random.default_rng(9)
    M = len(m["mp_bad"])
    mp["mp_replaced"][rng.permutation(M)[:40]] = rng.integers(0, M, 40).astype(np.int32)
    rm = dict({k: m[k] for k in ("mp_xw", "mp_bad", "mp_nobs", "mp_desc", "kf_n", "kf_mappoint")}, **mp)
    last = frames_of(fr, kp, extra)
    last["frame_outlier"] = (rng.random(last["frame_outlier"].shape) < 0.05).astype(np.uint8)
    cur = TC.copy(last)   # the same keypoints seen again after a small motion
    cur["frame_mappoint"] = rng.integers(-1, M, cur["frame_mappoint"].shape).astype(np.int32)   # cleared by the call
    cur["kp_xy"] = (cur["kp_xy"] + rng.normal(0, 0.3, cur["kp_xy"].shape)).astype(np.float32)
    cur["kp_angle"] = (cur["kp_angle"] + rng.normal(0, 2, cur["kp_angle"].shape)).astype(np.float32) % np.float32(360)
    vel = np.tile(np.concatenate([np.eye(3).reshape(-1), [0, 0, 0]]).astype(np.float32), (F, 1))
    vel[:, 9:] = rng.normal(0, 0.004, (F, 3))
    baseline = np.full(F, 0.08, np.float32)
    # ---- the restatement chain
    rcur, rlast, rmap = TC.copy(cur), TC.copy(last), TC.copy(rm)
    proj = R.motion_project(rcur, rlast, rmap, vel, baseline, False)
    okm, on = oracle.search_by_projection_motion(T.motion_batch(proj, rcur, kp["scale_factors"], th))
    assert on.sum() > 100
    R.apply_matches(rcur, R.REPLACE, okm.reshape(F, -1), rlast["frame_mappoint"], None, M)
    redges = R.pose_edges(rcur, rmap, inv_sigma2)
    E = int(redges["edge_begin"][-1])
    ores = oracle.pose_optimization({k: (v[:E] if k in ("xw", "obs", "inv_sigma2") else v) for k, v in redges.items() if k != "edge_kp"})
    rfin = R.finish_pose(rcur, rmap, R.DISCARD, redges, ores)
    # ---- the device chain
    dcur, dlast, dmap = put(cur, True), put(last, True), put(rm, True)
    d_vel, d_base, d_table = one(vel, True), one(baseline, True), one(inv_sigma2, True)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dproj = T.motion_project(dcur, dlast, dmap, d_vel, d_base, False, stream=s)
        kp_match, n_matches = search_by_projection_motion_device(T.motion_batch(dproj, dcur, kp["scale_factors"], th), stream=s)
        T.apply_matches(dcur, T.REPLACE, kp_match, dlast["frame_mappoint"], M, stream=s)
        edges = T.pose_edges(dcur, dmap, d_table, stream=s)
        po = pose_optimization_device(edges, stream=s)
        fin = T.finish_pose(dcur, dmap, T.DISCARD, edges, po, stream=s)
    s.synchronize()
    assert_all_same(get(dproj), proj, "motion_project")
    assert same(n_matches.cpu().numpy()[:F], on) and same(kp_match.cpu().numpy(), okm)
    g, ge, gpo, gf = get(dcur), get(edges), get(po), get(fin)
    assert E > 100 and ge["edge_begin"][-1] == E
    for k in ("edge_begin", "pose_R", "pose_t", "cam"):
        assert same(ge[k], redges[k]), k
    for k in ("xw", "obs", "inv_sigma2", "edge_kp"):
        assert same(ge[k][:E], redges[k][:E]), k
    assert same(gpo["outlier"][:E], ores["outlier"])
    assert np.abs(gpo["pose_t"] - ores["pose_t"]).max() < 1e-6 and np.abs(gpo["pose_R"] - ores["pose_R"]).max() < 1e-6
    assert same(g["pose"], np.concatenate([gpo["pose_R"], gpo["pose_t"]], 1).astype(np.float32))
    assert same(g["frame_mappoint"], rcur["frame_mappoint"]) and same(g["frame_outlier"], rcur["frame_outlier"])
    assert same(get(dlast)["frame_mappoint"], rlast["frame_mappoint"])
    assert same(gf["n_inliers"], rfin["n_inliers"]) and same(gf["n_discarded"], rfin["n_discarded"])
    for f in range(F):
        n = rfin["n_discarded"][f]
        assert same(gf["discarded"][f, :n], rfin["discarded"][f, :n]), f
