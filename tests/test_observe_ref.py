"""tests/observe_ref.py pinned on hand-built maps: every branch of AddObservation, Replace and the three apply loops, both
sides of every gate, and a walk stopped by a full row at its first, a middle and its last step and resumed.  CPU only."""
import numpy as np
import pytest

import observe_cases as OC
import observe_ref as OR

K, CAP = 5, 4


def tiny(obs, room, stereo=(), bad=()):
    """obs[p]: [(keyframe, index)] ascending; room[p]: entries of p's row; stereo: (keyframe, index) with a right coordinate."""
    M = len(obs)
    kf_mappoint = np.full((K, CAP), -1, np.int32)
    uright = np.full((K, CAP), -1, np.float32)
    for k, i in stereo:
        uright[k, i] = 10
    rows = []
    for p, o in enumerate(obs):
        for k, i in o:
            kf_mappoint[k, i] = p
        rows.append(list(o) + [(-1, -1)] * (room[p] - len(o)))
    t = dict(kf_n=np.full(K, CAP, np.int32), kf_mappoint=kf_mappoint, kf_uright=uright, mp_bad=np.zeros(M, np.uint8),
             mp_nobs=np.array([sum(2 if (k, i) in stereo else 1 for k, i in o) for o in obs], np.int32),
             mp_found=np.arange(1, M + 1).astype(np.int32), mp_visible=(10 * np.arange(1, M + 1)).astype(np.int32),
             mp_replaced=np.full(M, -1, np.int32), mp_obs_off=np.concatenate([[0], np.cumsum(room)]).astype(np.int32),
             mp_obs_kf=np.array([k for r in rows for k, _ in r], np.int32), mp_obs_idx=np.array([i for r in rows for _, i in r], np.int32))
    t["mp_bad"][list(bad)] = 1
    return t


def row(t, p):
    return [(int(k), int(i)) for k, i in zip(t["mp_obs_kf"][t["mp_obs_off"][p]:t["mp_obs_off"][p + 1]],
                                              t["mp_obs_idx"][t["mp_obs_off"][p]:t["mp_obs_off"][p + 1]])]


def walk(t, mode, kf, entries, **kw):
    """entries: [(point, best_idx)] of one item on keyframe kf."""
    return OR.fuse_apply(t, mode, [kf], [0, len(entries)], [p for p, _ in entries], [b for _, b in entries], **kw)


def test_add_observation_inserts_in_slot_order_packs_the_row_and_counts_mono_and_stereo():
    t = tiny([[(1, 0), (3, 0)]], [4], stereo={(2, 1)})
    t["mp_obs_kf"][:4], t["mp_obs_idx"][:4] = [1, -1, 3, -1], [0, 7, 0, 7]      # a hole inside the row
    m = OR.Map(t)
    assert m.add_observation(0, 2, 1) and row(m.t, 0) == [(1, 0), (2, 1), (3, 0), (-1, -1)] and m.t["mp_nobs"][0] == 4   # stereo: + 2
    assert m.add_observation(0, 4, 2) and row(m.t, 0) == [(1, 0), (2, 1), (3, 0), (4, 2)] and m.t["mp_nobs"][0] == 5     # mono: + 1, last
    before = {k: v.copy() for k, v in m.t.items()}
    assert not m.add_observation(0, 3, 3)                                      # present: nothing, though the row is full
    assert all(np.array_equal(before[k], m.t[k]) for k in before)
    with pytest.raises(OR.Overflow):
        m.add_observation(0, 0, 3)
    assert all(np.array_equal(before[k], m.t[k]) for k in before)
    m2 = OR.Map(tiny([[(1, 0)]], [2]))
    assert m2.add_observation(0, 0, 3) and row(m2.t, 0) == [(0, 3), (1, 0)]     # first


def test_replace_moves_or_erases_and_leaves_the_loser_as_the_reference_does():
    # the loser observes keyframes 0, 1, 2; the survivor observes 1 (erase) and 3
    t = tiny([[(0, 0), (1, 0), (2, 0)], [(1, 1), (3, 0)]], [3, 4], stereo={(0, 0)})
    m = OR.Map(t)
    assert m.replace(0, 1)
    assert row(m.t, 1) == [(0, 0), (1, 1), (2, 0), (3, 0)] and row(m.t, 0) == [(-1, 0), (-1, 0), (-1, 0)]
    assert m.t["kf_mappoint"][0, 0] == 1 and m.t["kf_mappoint"][2, 0] == 1 and m.t["kf_mappoint"][1, 0] == -1 and m.t["kf_mappoint"][1, 1] == 1
    assert m.t["mp_nobs"].tolist() == [4, 2 + 2 + 1]                           # the loser's stays; stereo + mono gained
    assert m.t["mp_found"][1] == 2 + 1 and m.t["mp_visible"][1] == 20 + 10 and m.t["mp_bad"].tolist() == [1, 0] and m.t["mp_replaced"].tolist() == [1, -1]
    before = {k: v.copy() for k, v in m.t.items()}
    assert not m.replace(1, 1)                                                 # the id test
    assert all(np.array_equal(before[k], m.t[k]) for k in before)
    # the survivor's bad flag is not tested; a union that does not fit writes nothing
    m = OR.Map(tiny([[(0, 0), (2, 0)], [(1, 1)]], [2, 2], bad=[1]))
    before = {k: v.copy() for k, v in m.t.items()}
    with pytest.raises(OR.Overflow) as e:
        m.replace(0, 1)
    assert e.value.point == 1 and all(np.array_equal(before[k], m.t[k]) for k in before)
    m = OR.Map(tiny([[(0, 0)], [(1, 1)]], [1, 2], bad=[1]))
    assert m.replace(0, 1) and row(m.t, 1) == [(0, 0), (1, 1)] and m.t["mp_bad"].tolist() == [1, 1]


def test_fuse_mode_gates():
    # keyframe 4 holds point 1 at keypoint 0 and point 2 at keypoint 1; keypoint 2 is free
    obs = [[(0, 0)], [(1, 0), (4, 0)], [(4, 1)], [(0, 1), (1, 1)], [(0, 2)]]
    t = tiny(obs, [4] * 5)
    # more observations in the keyframe's point: the candidate is replaced
    r = walk(t, OR.FUSE, 4, [(0, 0)])
    assert r["mp_bad"].tolist() == [1, 0, 0, 0, 0] and r["mp_replaced"][0] == 1 and r["touched"].tolist() == [1] and r["n_fused"].tolist() == [1]
    # equal counts: the keyframe's point is replaced (the > of ORBmatcher.cc:964)
    r = walk(t, OR.FUSE, 4, [(0, 1)])
    assert r["mp_bad"].tolist() == [0, 0, 1, 0, 0] and r["mp_replaced"][2] == 0 and r["kf_mappoint"][4, 1] == 0 and r["touched"].tolist() == [0]
    # fewer: the keyframe's point is replaced
    r = walk(t, OR.FUSE, 4, [(3, 1)])
    assert r["mp_replaced"][2] == 3 and r["mp_nobs"][3] == 3
    # a free keypoint: AddObservation and AddMapPoint; nothing is touched
    r = walk(t, OR.FUSE, 4, [(0, 2)])
    assert r["kf_mappoint"][4, 2] == 0 and r["mp_nobs"][0] == 2 and r["touched"].tolist() == [] and r["n_fused"].tolist() == [1]
    # misses, null points, a bad candidate, a candidate that observes the keyframe, a bad point in the keyframe
    r = walk(dict(t, mp_bad=np.array([0, 0, 1, 0, 1], np.uint8)), OR.FUSE, 4, [(0, -1), (-1, 0), (4, 0), (1, 1), (3, 1)])
    assert r["n_fused"].tolist() == [1] and all(np.array_equal(r[k], t[k]) for k in OR.UPDATED if k != "mp_bad")
    assert [e[0] for e in r["trace"]] == ["skipped_bad", "skipped_observes", "in_kf_bad"]


def test_a_chain_and_points_that_change_earlier_in_the_walk():
    obs = [[(0, 0)], [(1, 0), (4, 0)], [(2, 0), (3, 0), (4, 1)], [(0, 1)]]
    t = tiny(obs, [5] * 4)
    # A = 0 -> B = 1 (B has more), then on keyframe 2 B -> C = 2 (C counts 4 with its stereo observation, B 3 by then): A's
    # observation ends in C
    r = OR.fuse_apply(tiny(obs, [5] * 4, stereo={(2, 0)}), OR.FUSE, [4, 2], [0, 1, 2], [0, 1], [0, 0])
    assert r["mp_replaced"].tolist() == [1, 2, -1, -1] and r["kf_mappoint"][0, 0] == 2 and r["touched"].tolist() == [2] and r["mp_nobs"][2] == 6
    # a point that went bad earlier in the walk is skipped at its turn
    r = walk(t, OR.FUSE, 4, [(0, 0), (0, 1)])
    assert r["mp_replaced"].tolist()[:2] == [1, -1] and [e[0] for e in r["trace"] if e[0].startswith("skip")] == ["skipped_bad"]
    r = OR.fuse_apply(t, OR.LOOP_MATCHED, [4, 4], [0, 1, 2], [1, 2], [0, 0])
    # loop mode on keyframe 4, keypoint 0: Replace(1 -> 1) is the id return; then 1 -> 2
    assert r["mp_replaced"].tolist() == [-1, 2, -1, -1] and r["touched"].tolist() == [2] and r["n_fused"].tolist() == [1, 1]
    r = OR.fuse_apply(t, OR.FUSE, [0, 4], [0, 1, 2], [1, 3], [0, 0])
    # item 0: point 0 (keyframe 0, keypoint 0) into 1; item 1: 3 (one observation) meets 1 at keyframe 4: 3 -> 1, and the chain 0 -> 1 <- 3
    assert r["mp_replaced"].tolist() == [1, -1, -1, 1] and row(dict(t, **r), 1)[:3] == [(0, 0), (1, 0), (4, 0)] and r["kf_mappoint"][0, 1] == -1
    # a point that gains the keyframe earlier in the walk is skipped at its turn
    r = walk(t, OR.FUSE, 4, [(3, 2), (3, 0)])
    assert r["n_fused"].tolist() == [1] and [e[0] for e in r["trace"]] == ["added", "skipped_observes"]


def test_sim3_mode_runs_its_replacements_after_the_items_whole_list():
    obs = [[(0, 0)], [(4, 0)], [(1, 0)]]
    t = tiny(obs, [4] * 3)
    # entry 0: point 0 meets point 1 at keypoint 0 -> replace_point; entry 1: point 0 is added at the free keypoint 1 (no
    # IsInKeyFrame test in this mode's phase 0).  Phase 1: Replace(1 -> 0) sees that 0 observes keyframe 4 by now: erase
    r = walk(t, OR.FUSE_SIM3, 4, [(0, 0), (0, 1), (2, -1)])
    assert r["replace_point"].tolist() == [1, -1, -1] and r["n_fused"].tolist() == [2]
    assert r["kf_mappoint"][4].tolist() == [-1, 0, -1, -1] and row(dict(t, **r), 0)[:2] == [(0, 0), (4, 1)] and r["mp_replaced"][1] == 0
    assert r["touched"].tolist() == [0] and ("erased", 1, 0, 4) in r["trace"]
    # a bad point in the keyframe is not recorded
    r = walk(dict(t, mp_bad=np.array([0, 1, 0], np.uint8)), OR.FUSE_SIM3, 4, [(0, 0)])
    assert r["replace_point"].tolist() == [-1] and r["n_fused"].tolist() == [1] and r["mp_replaced"].tolist() == [-1] * 3


def test_loop_mode_replaces_a_bad_point_and_touches_what_it_adds():
    obs = [[(0, 0)], [(4, 0)], [(1, 0)]]
    t = tiny(obs, [4] * 3, bad=[1])
    r = walk(t, OR.LOOP_MATCHED, 4, [(0, 0), (2, 3), (-1, 2)])
    assert r["mp_replaced"][1] == 0 and r["kf_mappoint"][4].tolist() == [0, -1, -1, 2] and r["touched"].tolist() == [0, 2]
    assert row(dict(t, **r), 2)[:2] == [(1, 0), (4, 3)] and r["n_fused"].tolist() == [2]


@pytest.mark.parametrize("mode", OC.MODES)
def test_a_walk_stopped_at_its_first_a_middle_and_its_last_step_resumes_to_the_uninterrupted_result(mode):
    # three steps, each needing one free entry in its survivor's or its point's row
    obs = [[(0, 0)], [(1, 0)], [(2, 0)], [(4, 0)], [(4, 1)]]
    entries = [(0, 0), (1, 1), (2, 2)]                       # Replace with 3, Replace with 4, an add at the free keypoint 2
    want = walk(tiny(obs, [3] * 5), mode, 4, entries)
    assert want["status"] == OR.OK
    steps = sorted(set(e[1] for e in want["trace"] if e[0] in ("replaced", "added")))
    for stop in range(3):
        survivor = {e[1]: e[3] if e[0] == "replaced" else e[2] for e in want["trace"] if e[0] in ("replaced", "added")}[steps[stop]]
        room = [3] * 5
        room[survivor] = 1                                   # full at that step, not before
        t = tiny(obs, room)
        r = walk(t, mode, 4, entries)
        assert r["status"] == OR.OBS_OVERFLOW and r["progress"][3] == survivor
        t.update({k: r[k] for k in OR.UPDATED})
        off, kf, idx, st = OR.grow_observations(t["mp_obs_off"], t["mp_obs_kf"], t["mp_obs_idx"], 2, None, len(t["mp_obs_kf"]) + 10)
        t.update(mp_obs_off=off, mp_obs_kf=kf, mp_obs_idx=idx)
        r2 = walk(t, mode, 4, entries, **{k: r[k] for k in ("replace_point", "n_fused", "touched", "progress")})
        assert st == OR.OK and r2["status"] == OR.OK and r2["progress"].tolist() == [1, 0, 0, -1]
        a, b = OC.canonical(dict(t, **{k: r2[k] for k in OR.UPDATED})), OC.canonical(dict(tiny(obs, [3] * 5), **{k: want[k] for k in OR.UPDATED}))
        for k in OR.UPDATED + ("mp_obs_off",):
            assert np.array_equal(a[k], b[k]), (stop, k)
        for k in ("n_fused", "replace_point", "touched"):
            assert np.array_equal(r2[k], want[k]), (stop, k)


def test_the_new_keyframe_loop_and_the_grown_csr():
    t = tiny([[(0, 0)], [(1, 0), (4, 1)], [(2, 0)], [(3, 0)]], [2, 2, 1, 2], stereo={(4, 0)}, bad=[3])
    t["kf_mappoint"][4] = [0, 1, 2, 3]                       # Tracking's matches: 1 observes it already, 2's row is full, 3 is bad
    out, added, recent, status = OR.add_keyframe_observations(t, 4)
    assert added.tolist() == [0] and recent.tolist() == [1] and status.tolist() == [0, 0, OR.OBS_OVERFLOW, 0]
    assert out["mp_nobs"].tolist() == [3, 2, 1, 1] and out["mp_obs_kf"].tolist() == [0, 4, 1, 4, 2, 3, -1]
    off, kf, idx, st = OR.grow_observations(t["mp_obs_off"], out["mp_obs_kf"], out["mp_obs_idx"], 1, None, 20)
    assert off.tolist() == [0, 3, 6, 8, 10] and kf[:10].tolist() == [0, 4, -1, 1, 4, -1, 2, -1, 3, -1] and st == OR.OK
    off, kf, idx, st = OR.grow_observations(t["mp_obs_off"], out["mp_obs_kf"], out["mp_obs_idx"], 0, [2, 0, -1, 0], 7)
    assert off.tolist() == [0, 4, 6, 7, 8] and st == OR.OBS_OVERFLOW and kf.tolist() == [0, 4, -1, -1, 1, 4, 2]
