"""Shared generator for the observation-edit tests (tests/test_observe_*.py).  culling_cases.make_case is K = 24, kf_cap = 256,
M = 1500 with packed rows; the maps here need row slack, holes and planted walks, so they are built directly.

main()    K = 12, kf_cap = 64, M = 300: rows ascending in keyframe slot (asserted), a hole in some rows, `slack` free entries
          per row, and a Fuse list of N_ITEMS keyframes whose best_idx is planted at random over occupied and free
          keypoints.  The builder asserts on the restatement's trace that one walk holds at least 20 replacements in each
          direction, 20 adds, 5 entries skipped at their turn (bad by then, or the keyframe gained by then) and a chain
          A -> B, B -> C.
wide()    K = 320, kf_cap = 8: points of 70 and 300 observations replaced into points of 1, 65 and 260, the unions longer
          than a wavefront and than the workgroup, disjoint (interleaved) and overlapping.
dirty(c)  the same with slots, indices and offsets outside their tables written over some entries (what is live still
          ascends).
Computed once; treat as read-only (tables() copies)."""
import functools

import numpy as np

import observe_ref as OR

TABLES = ("kf_n", "kf_mappoint", "kf_uright", "mp_bad", "mp_nobs", "mp_found", "mp_visible", "mp_replaced", "mp_obs_off",
          "mp_obs_kf", "mp_obs_idx")
APPLY = ("item_kf", "mp_begin", "point", "best_idx")
K, KF_CAP, M = 12, 64, 300
N_ITEMS, PER_ITEM = 5, 90
MODES = (OR.FUSE, OR.FUSE_SIM3, OR.LOOP_MATCHED)


def build_tables(K, kf_cap, M, obs, slack, rng, holes=True):
    """obs[p]: ascending list of (keyframe, index).  A row is its entries, a -1 inside some rows, then slack free entries."""
    kf_n = np.full(K, kf_cap, np.int32)
    kf_mappoint = np.full((K, kf_cap), -1, np.int32)
    rows = []
    for p, o in enumerate(obs):
        assert [k for k, _ in o] == sorted(set(k for k, _ in o)), p   # the rows ascend; no keyframe twice
        for k, i in o:
            assert kf_mappoint[k, i] == -1
            kf_mappoint[k, i] = p
        row = list(o)
        if holes and len(row) >= 2 and rng.random() < 0.3:
            row.insert(int(rng.integers(1, len(row))), (-1, -1))          # an erased observation
        rows.append(row + [(-1, -1)] * slack)
    uright = np.where(rng.random((K, kf_cap)) < 0.5, rng.random((K, kf_cap)) * 600, -1).astype(np.float32)
    t = dict(kf_n=kf_n, kf_mappoint=kf_mappoint, kf_uright=uright, mp_bad=np.zeros(M, np.uint8),
             mp_nobs=np.array([sum(2 if uright[k, i] >= 0 else 1 for k, i in o) for o in obs], np.int32),
             mp_found=rng.integers(0, 40, M).astype(np.int32), mp_visible=rng.integers(40, 90, M).astype(np.int32),
             mp_replaced=np.full(M, -1, np.int32),
             mp_obs_off=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32),
             mp_obs_kf=np.array([k for r in rows for k, _ in r], np.int32), mp_obs_idx=np.array([i for r in rows for _, i in r], np.int32))
    return t


def make_main(seed=0, slack=K):
    rng = np.random.default_rng(seed)
    free = [list(rng.permutation(KF_CAP - 10)) for _ in range(K)]        # the top keypoints of every keyframe stay free
    obs = []
    for p in range(M):
        room = [k for k in range(K) if free[k]]
        n = min(int(rng.choice([0, 1, 1, 2, 2, 2, 3, 4])), len(room))
        obs.append([(int(k), int(free[k].pop())) for k in sorted(rng.choice(room, n, replace=False))])
    t = build_tables(K, KF_CAP, M, obs, slack, rng)
    for p in range(M):                                                   # a point without observations is bad, as after a cull
        if not obs[p]:
            t["mp_bad"][p] = 1
    item_kf = rng.choice(K, N_ITEMS, replace=False).astype(np.int32)
    point, best = [], []
    for kf in item_kf:
        cand = rng.choice(M, PER_ITEM, replace=False)
        for p in cand:
            point.append(int(p) if rng.random() > 0.03 else -1)
            best.append(int(rng.integers(0, KF_CAP)) if rng.random() < 0.45 else -1)
    return dict(t, item_kf=item_kf, mp_begin=(np.arange(N_ITEMS + 1) * PER_ITEM).astype(np.int32),
                point=np.array(point, np.int32), best_idx=np.array(best, np.int32))


def wide_sets():
    K = 320
    ev = lambda a, b: list(range(a, b, 2))                               # noqa: E731
    sets = dict(L70a=ev(0, 140), L70b=list(range(100, 170)), L70c=list(range(250, 320)), L300a=list(range(0, 300)),
                L300b=list(range(20, 320)), L300c=[k for k in range(K) if not 150 <= k < 170], S1a=[5], S1b=[200],
                S65a=ev(1, 131), S65b=list(range(90, 155)), S260a=list(range(30, 290)), S260b=list(range(60, 320)))
    pairs = (("L70a", "S65a", 0), ("L70b", "S1a", 100), ("L70c", "S260a", 300), ("L300a", "S1b", 0), ("L300b", "S65b", 20),
             ("L300c", "S260b", 0))                                      # loser, survivor, a keyframe only the loser observes
    return K, sets, pairs


def make_wide(seed=1):
    rng = np.random.default_rng(seed)
    K, sets, pairs = wide_sets()
    names = list(sets)
    nxt = [0] * K
    obs = []
    for n in names:
        o = []
        for k in sets[n]:
            o.append((k, nxt[k]))
            nxt[k] += 1
        obs.append(o)
    assert max(nxt) <= 8 and [len(sets[n]) for n in names] == [70, 70, 70, 300, 300, 300, 1, 1, 65, 65, 260, 260]
    t = build_tables(K, 8, len(names), obs, K, rng)
    item_kf, point, best = [], [], []
    for loser, surv, kf in pairs:
        assert kf in sets[loser] and kf not in sets[surv]
        item_kf.append(kf)
        point.append(names.index(surv))
        best.append(dict(obs[names.index(loser)])[kf])
    unions = [len(set(sets[a]) | set(sets[b])) for a, b, _ in pairs]
    overlaps = [len(set(sets[a]) & set(sets[b])) for a, b, _ in pairs]
    assert min(unions) < 256 < max(unions) and any(64 < u < 256 for u in unions) and 0 in overlaps and max(overlaps) > 64
    return dict(t, item_kf=np.array(item_kf, np.int32), mp_begin=np.arange(len(pairs) + 1).astype(np.int32),
                point=np.array(point, np.int32), best_idx=np.array(best, np.int32))


def dirty(c):
    """Entries outside their tables: the device skips them; the host entries refuse them."""
    c = {k: v.copy() for k, v in c.items()}
    M, K, cap = len(c["mp_bad"]), len(c["kf_n"]), c["kf_mappoint"].shape[1]
    live = np.flatnonzero(c["mp_obs_kf"] >= 0)
    c["mp_obs_kf"][live[[3, 40, 77]]] = K + 3, -2, 2 ** 30                 # no longer live: what is left still ascends
    c["mp_obs_idx"][live[[5, 60, 90]]] = cap + 1, -4, -(2 ** 31)
    c["kf_mappoint"][1, 3], c["kf_mappoint"][int(c["item_kf"][0]), 7], c["kf_mappoint"][int(c["item_kf"][1]), 9] = M + 5, M, -7
    c["point"][[2, 50, 120]] = M, -9, 2 ** 30
    c["best_idx"][[4, 51, 121, 200]] = cap, cap + 7, 2 ** 30, -3
    c["best_idx"][[7, 9]] = 7, 9                                         # reach the entries written above
    c["item_kf"] = np.concatenate([c["item_kf"], [K + 2, -1]]).astype(np.int32)
    c["mp_begin"] = np.concatenate([c["mp_begin"], [c["mp_begin"][-1], len(c["point"]) + 11]]).astype(np.int32)
    c["mp_obs_off"][M] += 7                                              # past the arrays
    c["kf_n"][2], c["kf_n"][3] = cap + 9, -1
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "wide":
        return make_wide()
    c = make_main()
    return dirty(c) if name == "dirty" else c


def tables(c):
    return {k: c[k].copy() for k in TABLES}


def apply_of(c):
    return {k: c[k] for k in APPLY}


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """The restatement's walk: computed once, shared, left unchanged."""
    c = case(name)
    return OR.fuse_apply(tables(c), mode, **apply_of(c))


def canonical(t):
    """The tables with the observation CSR compacted: what two walks on rows of different slack are compared on."""
    t = dict(t)
    off, kf, idx, _ = OR.grow_observations(t["mp_obs_off"], t["mp_obs_kf"], t["mp_obs_idx"], 0, None, len(t["mp_obs_kf"]))
    t["mp_obs_off"], t["mp_obs_kf"], t["mp_obs_idx"] = off, kf[:off[-1]], idx[:off[-1]]
    return t


def new_keyframe(seed=3):
    """The main map with keyframe CUR's observations taken out of most of its points' rows, as before ProcessNewKeyFrame: the
    points Tracking matched do not observe it yet; a few (the stereo points it created) do; one point's row is full."""
    c = make_main(seed, slack=1)
    t = tables(c)
    m = OR.Map(t)
    cur = int(np.argmax([(t["kf_mappoint"][k] >= 0).sum() for k in range(K)]))
    rng = np.random.default_rng(seed)
    kept = 0
    for i in range(KF_CAP):
        p = int(t["kf_mappoint"][cur, i])
        if p < 0:
            continue
        if rng.random() < 0.2:
            kept += 1
            continue
        e0, e1 = m.range[p]
        row = [(o, j) for o, j in m.observations(p) if o != cur]
        m.write_row(p, row)
        m.t["mp_nobs"][p] -= 2 if m.stereo(cur, i) else 1
    full = next(int(t["kf_mappoint"][cur, i]) for i in range(KF_CAP) if t["kf_mappoint"][cur, i] >= 0
                and not m.is_in_keyframe(int(t["kf_mappoint"][cur, i]), cur))
    e0, e1 = m.range[full]
    others = [k for k in range(K) if k != cur and not m.is_in_keyframe(full, k)]
    row = sorted(m.observations(full) + [(k, KF_CAP - 1 - j) for j, k in enumerate(others)])[:e1 - e0]
    m.write_row(full, row)                                               # no free entry (its extra entries have no kf_mappoint)
    assert len(m.observations(full)) == e1 - e0 and kept >= 3
    return m.t, cur, full


def _check():
    c = case("main")
    for mode in MODES:
        assert expected("main", mode)["status"] == OR.OK
    tr = expected("main", OR.FUSE)["trace"]
    pt = c["point"]
    rep = [e for e in tr if e[0] == "replaced"]
    into_kf = [e for e in rep if e[2] == pt[e[1]]]                       # the candidate is the loser
    into_point = [e for e in rep if e[3] == pt[e[1]]]
    assert len(into_kf) >= 20 and len(into_point) >= 20, (len(into_kf), len(into_point))
    assert sum(e[0] == "added" for e in tr) >= 20
    assert sum(e[0] in ("skipped_bad", "skipped_observes") for e in tr) >= 5 and any(e[0] == "skipped_observes" for e in tr)
    was_bad = set(np.flatnonzero(c["mp_bad"]).tolist())
    assert any(e[0] == "skipped_bad" and e[2] not in was_bad for e in tr)    # went bad earlier in the walk
    survivors = {}
    chain = False
    for e in rep:
        chain |= e[2] in survivors                                       # the loser survived an earlier Replace
        survivors[e[3]] = e[1]
    assert chain
    assert any(e[0] == "erased" for e in tr) and any(e[0] == "moved" for e in tr)
    for mode in MODES:
        w = expected("wide", mode)
        assert w["status"] == OR.OK and sum(e[0] == "replaced" for e in w["trace"]) == 6
    assert sorted(int(x) for x in expected("wide", OR.LOOP_MATCHED)["mp_replaced"][:6]) == [6, 7, 8, 9, 10, 11]


_check()
