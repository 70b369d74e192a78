"""The culls on the GPU (orbmm_cull_*, orb_slam2_refactored_amd/culling.py) against the restatement tests/culling_ref.py:
every table after MapPointCulling and after KeyFrameCulling identical through the host and the device entries, kf_tcp as
bits, the observation CSR with its erased entries and compacted; the case with entries outside their tables on the device
entries; a rerun; the children of live keyframes; the culled list into the keyframe database's erase; and the chain cull ->
compact -> live children -> UpdateConnections -> TrackLocalMap on one stream."""
import numpy as np
import pytest

import culling_cases as CC
import culling_ref as CR
import local_map_cases as LC
import local_map_ref as LR
import map_maintenance_cases as MC
import map_maintenance_ref as MR
from orb_slam2_refactored_amd import culling as CU
from orb_slam2_refactored_amd import map_maintenance as MM
from orb_slam2_refactored_amd.local_map import OUT_KEYS, LocalMap

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return a.shape == b.shape and np.array_equal(a, b)


def dev(d):
    import torch
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def points_device(name):
    """map_point_culling_device on a fresh device copy; (the tables, recent, n) back as numpy."""
    import torch
    t = dev(CC.tables(CC.case(name)))
    recent = torch.from_numpy(CC.recent(name).copy()).cuda()
    n = CU.map_point_culling_device(t, recent, CC.CUR_KF_ID, CC.MONOCULAR)
    torch.cuda.synchronize()
    return host(t), recent.cpu().numpy(), int(n.cpu()[0])


def keyframes_device(t, cur=CC.CUR, monocular=CC.MONOCULAR):
    import torch
    t = dev(t)
    culled, n, status = CU.keyframe_culling_device(t, cur, monocular, CC.TH_DEPTH)
    torch.cuda.synchronize()
    return host(t), culled.cpu().numpy(), int(n.cpu()[0]), int(status.cpu()[0])


@pytest.mark.parametrize("name", ["clean", "dirty"])
def test_map_point_culling_equals_the_restatement(name):
    want, kept, _ = CC.expected_points(name)
    got, recent, n = points_device(name)
    for k in CC.TABLES:
        assert same(got[k], want.get(k, CC.case(name)[k])), k
    assert n == len(kept) and same(recent[:n], kept) and 0 < n < len(recent)
    again = points_device(name)
    assert all(same(got[k], again[0][k]) for k in CC.TABLES) and same(recent[:n], again[1][:n]) and n == again[2]
    off, kf, idx = CR.compact_observations(want["mp_obs_off"] if "mp_obs_off" in want else CC.case(name)["mp_obs_off"],
                                           want["mp_obs_kf"], CC.case(name)["mp_obs_idx"])
    if name == "clean":                                  # the host form, which validates: the clean map only
        t = {k: CC.case(name)[k] for k in CU.POINT_KEYS}
        raw, left = CU.MapPointCulling(t, CC.recent(name), CC.CUR_KF_ID, CC.MONOCULAR, compact=False)
        for k in CR.POINT_UPDATED:
            assert same(raw[k], want[k]), k
        assert same(left, kept) and (raw["mp_obs_kf"] == -1).any()
        packed, left = CU.MapPointCulling(t, CC.recent(name), CC.CUR_KF_ID, CC.MONOCULAR)
        assert same(left, kept) and same(packed["mp_obs_off"], off)
        assert same(packed["mp_obs_kf"], kf[:off[-1]]) and same(packed["mp_obs_idx"], idx[:off[-1]])


@pytest.mark.parametrize("monocular", [False, True])
@pytest.mark.parametrize("name", ["clean", "dirty"])
def test_keyframe_culling_equals_the_restatement(name, monocular):
    import torch
    want, culled, n, _ = (CC.expected_keyframes(name) if not monocular else
                          CR.keyframe_culling(CC.case(name), CC.CUR, True, CC.TH_DEPTH))
    got, got_culled, got_n, status = keyframes_device(CC.tables(CC.case(name)), monocular=monocular)
    for k in CC.TABLES:
        assert same(got[k], want.get(k, CC.case(name)[k])), k
    assert got_n == n and same(got_culled, culled) and status == CU.OK and n >= 3
    again = keyframes_device(CC.tables(CC.case(name)), monocular=monocular)
    assert all(same(got[k], again[0][k]) for k in CC.TABLES) and same(got_culled, again[1])
    # the compacted CSR, on the device
    off, kf, idx = CR.compact_observations(want.get("mp_obs_off", CC.case(name)["mp_obs_off"]), want["mp_obs_kf"], CC.case(name)["mp_obs_idx"])
    d = dev({k: got[k] for k in ("mp_obs_off", "mp_obs_kf", "mp_obs_idx")})
    o_off, o_kf, o_idx = (x.cpu().numpy() for x in CU.compact_observations_device(d["mp_obs_off"], d["mp_obs_kf"], d["mp_obs_idx"]))
    end = min(int(off[-1]), len(kf))
    assert same(o_off, off) and same(o_kf[:end], kf[:end]) and same(o_idx[:end], idx[:end]) and (want["mp_obs_kf"] == -1).sum() > 100
    if name == "clean":                                  # the host forms
        raw, host_culled = CU.KeyFrameCulling(CC.case(name), CC.CUR, monocular, CC.TH_DEPTH, compact=False)
        for k in CR.KEYFRAME_UPDATED:
            assert same(raw[k], want[k]), k
        assert same(host_culled, culled[:n])
        packed, _ = CU.KeyFrameCulling(CC.case(name), CC.CUR, monocular, CC.TH_DEPTH)
        assert same(packed["mp_obs_off"], off) and same(packed["mp_obs_kf"], kf[:end]) and same(packed["mp_obs_idx"], idx[:end])
        h_off, h_kf, h_idx = CU.CompactObservations(want.get("mp_obs_off", CC.case(name)["mp_obs_off"]), want["mp_obs_kf"], CC.case(name)["mp_obs_idx"])
        assert same(h_off, off) and same(h_kf, kf[:end]) and same(h_idx, idx[:end])


def test_live_children_leave_the_culled_out_and_children_is_unchanged():
    import torch
    want, culled, n, _ = CC.expected_keyframes("clean")
    parent, bad = want["kf_parent"], want["kf_bad"]
    woff, widx = CR.live_children(parent, bad)
    off, idx = CU.live_children_device(torch.from_numpy(parent).cuda(), torch.from_numpy(bad).cuda())
    assert same(off.cpu().numpy(), woff) and same(idx.cpu().numpy()[:woff[-1]], widx)
    hoff, hidx = CU.LiveChildren(parent, bad)
    assert same(hoff, woff) and same(hidx, widx) and not set(widx.tolist()) & set(culled[:n].tolist())
    poff, pidx = MR.children(parent)
    coff, cidx = MM.children_device(torch.from_numpy(parent).cuda())
    assert same(coff.cpu().numpy(), poff) and same(cidx.cpu().numpy()[:poff[-1]], pidx)
    assert set(pidx.tolist()) & set(culled[:n].tolist())     # there a culled keyframe is still listed
    dirty = parent.copy()
    dirty[[2, 9]] = 30, -5                                   # outside the table: no parent
    doff, didx = CU.live_children_device(torch.from_numpy(dirty).cuda(), torch.from_numpy(bad).cuda())
    woff, widx = CR.live_children(dirty, bad)
    assert same(doff.cpu().numpy(), woff) and same(didx.cpu().numpy()[:woff[-1]], widx)


def test_the_culled_list_erases_exactly_the_culled_from_the_database():
    import torch
    import keyframe_db_cases as KC
    from orb_slam2_refactored_amd.keyframe_db import KeyFrameDatabase
    from orb_slam2_refactored_amd.synth import make_vocabulary
    from orb_slam2_refactored_amd.vocabulary import ORBVocabulary
    v = make_vocabulary(0, k=4, L=2)
    voc = ORBVocabulary.from_arrays(v["k"], v["L"], v["scoring"], v["weighting"], v["parent"], v["is_leaf"], v["desc"], v["weight"])
    c = KC.case("plain")
    db = KeyFrameDatabase(voc, c["max_keyframes"], c["word_cap"])
    db.add(c["slot"], c["bow_word"], c["bow_weight"], c["n_words"])
    live = lambda: set(np.flatnonzero(db.slots()[0]).tolist())  # noqa: E731
    before = live()
    _, culled, n, _ = CC.expected_keyframes("clean")
    _, got_culled, _, _ = keyframes_device(CC.tables(CC.case("clean")))
    assert len(got_culled) == CC.CONN_CAP and set(culled[:n].tolist()) <= before
    db.erase_device(torch.from_numpy(got_culled).cuda())     # n = conn_cap: the -1 padding is ignored
    torch.cuda.synchronize()
    assert live() == before - set(culled[:n].tolist())


def chain_map():
    """local_map_cases' mixed map with the tables the culls read: three covisibles of `cur` at the top octave, their thinly
    observed points taken out of their rows."""
    c = LC.case("mixed")
    m, fr, _ = LC.batch(c, 3)
    m = {k: v.copy() for k, v in m.items()}
    K, M, kf_cap = len(m["kf_bad"]), len(m["mp_bad"]), m["kf_mappoint"].shape[1]
    rng = np.random.default_rng(5)
    n_levels = fr["n_levels"]
    obs = [[] for _ in range(M)]
    for p in range(M):                                       # the keypoint index of each observation
        for e in range(m["mp_obs_off"][p], m["mp_obs_off"][p + 1]):
            k = int(m["mp_obs_kf"][e])
            hit = np.flatnonzero(m["kf_mappoint"][k] == p)
            if len(hit) and k not in [o for o, _ in obs[p]]:
                obs[p].append((k, int(hit[0])))
    m["kf_bad"][:] = 0
    t = dict(m, kf_id=np.arange(K, dtype=np.int32), kf_kp_octave=rng.integers(0, 3, (K, kf_cap)).astype(np.int32))
    t.update(MC.empty_state(K, K))
    cur = int(np.argmax(m["kf_n"]))
    for p in range(M):                                       # rows and observations agree; no bad point is observed
        if m["mp_bad"][p]:
            obs[p] = []
    rows = np.full_like(m["kf_mappoint"], -1)
    for p in range(M):
        for k, i in obs[p]:
            rows[k, i] = p
    t["kf_mappoint"] = rows
    csr = lambda: dict(mp_obs_off=np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32),  # noqa: E731
                       mp_obs_kf=np.array([k for o in obs for k, _ in o], np.int32),
                       mp_obs_idx=np.array([i for o in obs for _, i in o], np.int32))
    t.update(csr())
    first = MR.update_connections({k: t[k] for k in MC.GRAPH}, list(range(K)))
    hot = [int(s) for s in first["ord_slot"][cur, :3]]
    for k in hot:
        t["kf_kp_octave"][k] = n_levels - 1
        for i in range(kf_cap):
            p = int(t["kf_mappoint"][k, i])
            if p >= 0 and len(obs[p]) < 5:
                t["kf_mappoint"][k, i] = -1
                obs[p] = [(o, j) for o, j in obs[p] if o != k]
    t.update(csr())
    t.update({k: v for k, v in MR.update_connections({k: t[k] for k in MC.GRAPH}, list(range(K))).items() if k != "status"})
    t["kf_id"] = (np.arange(K) + 1).astype(np.int32)
    pose = np.zeros((K, 12), np.float32)
    for k in range(K):
        pose[k, :9] = MC.rotation(rng).reshape(-1)
        pose[k, 9:] = rng.normal(size=3) * 3
    t.update(kf_pose=pose, kf_uright=np.full((K, kf_cap), -1, np.float32), kf_depth=np.ones((K, kf_cap), np.float32),
             kf_not_erase=np.zeros(K, np.uint8), kf_to_be_erased=np.zeros(K, np.uint8), kf_tcp=np.zeros((K, 12), np.float32),
             mp_nobs=np.array([len(o) for o in obs], np.int32), mp_found=m["mp_visible"].copy(),
             mp_first_kf_id=np.zeros(M, np.int32), mp_ref_kf=np.array([o[0][0] if o else -1 for o in obs], np.int32))
    return c, t, fr, cur


def test_the_chain_on_one_stream_feeds_the_local_map():
    """KeyFrameCulling, the compaction, the live children and UpdateConnections of the current keyframe, then TrackLocalMap
    reading the arrays they wrote, all on one stream."""
    import torch
    c, t, fr, cur = chain_map()
    K = len(t["kf_bad"])
    # the restatement's tables
    cull, culled, n, _ = CR.keyframe_culling({k: t[k] for k in CC.TABLES}, cur, True, CC.TH_DEPTH)
    assert n >= 1
    after = dict(t, **cull)
    after["mp_obs_off"], kf, idx = CR.compact_observations(t["mp_obs_off"], cull["mp_obs_kf"], t["mp_obs_idx"])
    after["mp_obs_kf"], after["mp_obs_idx"] = kf[:after["mp_obs_off"][-1]], idx[:after["mp_obs_off"][-1]]
    conn = MR.update_connections({k: after[k] for k in MC.GRAPH}, [cur])
    after.update({k: conn[k] for k in MR.STATE_KEYS})
    off, kids = CR.live_children(after["kf_parent"], after["kf_bad"])
    after.update(kf_child_off=off, kf_child_idx=kids if len(kids) else np.zeros(1, np.int32))
    fr_w = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fr.items()}
    want = LR.track_local_map({k: v.copy() for k, v in after.items()}, fr_w, c["mp_cap"])
    # the device chain
    dt, dfr = dev(t), dev(fr)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got_culled, got_n, _ = CU.keyframe_culling_device(dt, cur, True, CC.TH_DEPTH, stream=s)
        dt["mp_obs_off"], dt["mp_obs_kf"], dt["mp_obs_idx"] = CU.compact_observations_device(dt["mp_obs_off"], dt["mp_obs_kf"],
                                                                                              dt["mp_obs_idx"], stream=s)
        dt["kf_child_off"], dt["kf_child_idx"] = CU.live_children_device(dt["kf_parent"], dt["kf_bad"], stream=s)
        status = MM.update_connections_device(dt, torch.tensor([cur], dtype=torch.int32, device="cuda"), stream=s)
        res = LocalMap(dt).track_local_map_device(dfr, c["mp_cap"], votes=True, stream=s)
    s.synchronize()
    assert (status.cpu().numpy() == 0).all() and int(got_n.cpu()[0]) == n and same(got_culled.cpu().numpy(), culled)
    for k in MR.STATE_KEYS + ("kf_bad", "mp_bad", "mp_nobs", "kf_mappoint"):
        assert same(dt[k].cpu().numpy(), after[k]), k
    for k in OUT_KEYS:
        assert same(res[k].cpu().numpy(), want[k]), k
    assert want["n_local_mp"].min() > 0
