"""Generated maps, frame batches and list batches for the map-creation tests (tests/test_creation_*.py).  Free map-point
slots hold what the entries' contract asks of the caller (mp_bad = 1, mp_nobs = 0, rows of -1) and recognisable values in
every other column, so that a column the constructor forgets shows."""
import numpy as np

COVIS = 10


def make_map(K=6, kf_cap=48, M=96, alloc=7, seed=0, rows=(2, 4), short_last_kf=True):
    """MAP_KEYS of creation.py.  Keyframe K - 1 has kf_n = kf_cap // 2 (with short_last_kf), the others kf_cap; keyframe 1 is bad."""
    rng = np.random.default_rng(seed)
    t = {}
    t["kf_id"] = (np.arange(K) * 3 + 2).astype(np.int32)
    t["kf_n"] = np.full(K, kf_cap, np.int32)
    if short_last_kf and K > 1:
        t["kf_n"][K - 1] = kf_cap // 2
    t["kf_mappoint"] = np.full((K, kf_cap), -1, np.int32)
    t["kf_uright"] = np.where(rng.random((K, kf_cap)) < 0.5, -1.0, rng.random((K, kf_cap)) * 600).astype(np.float32)
    t["kf_bad"] = np.zeros(K, np.uint8)
    if K > 2:
        t["kf_bad"][1] = 1
    t["kf_desc"] = rng.integers(0, 256, (K, kf_cap, 32), dtype=np.uint8)
    t["mp_bad"] = np.ones(M, np.uint8)
    t["mp_bad"][:alloc] = 0
    t["mp_xw"] = rng.normal(size=(M, 3)).astype(np.float32)
    t["mp_normal"] = rng.normal(size=(M, 3)).astype(np.float32)
    t["mp_max_min"] = (rng.random((M, 2)) + 1).astype(np.float32)
    t["mp_nobs"] = np.zeros(M, np.int32)
    t["mp_nobs"][:alloc] = 1
    t["mp_found"] = np.full(M, 77, np.int32)
    t["mp_visible"] = np.full(M, 78, np.int32)
    t["mp_replaced"] = np.full(M, 5, np.int32)
    t["mp_first_kf_id"] = np.full(M, 9999, np.int32)
    t["mp_ref_kf"] = np.full(M, -1, np.int32)
    t["mp_ref_kf"][:alloc] = 0
    t["mp_desc"] = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    lens = rng.integers(rows[0], rows[1] + 1, M)
    t["mp_obs_off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n_obs = int(t["mp_obs_off"][-1]) + 3                    # the arrays may be longer than the CSR
    t["mp_obs_kf"] = np.full(n_obs, -1, np.int32)
    t["mp_obs_idx"] = np.full(n_obs, -1, np.int32)
    for p in range(alloc):                                   # the points in use: one observation in keyframe 0
        t["mp_obs_kf"][t["mp_obs_off"][p]], t["mp_obs_idx"][t["mp_obs_off"][p]] = 0, kf_cap - 1 - p
        t["kf_mappoint"][0, kf_cap - 1 - p] = p
    return t


def make_lists(t, sizes, list_cap, two=False, by_keypoint=False, seed=1, values=True, drops=0, frames=None):
    """A list batch of len(sizes) items on map t; item i is on keyframe i % K (and (i + 1) % K with `two`, the two swapped for odd i).  No keypoint is listed twice.  drops: that many entries of every non-empty list get an index at or past kf_n or -1.
    frames: (F, kp_cap) for item_frame / frame_mappoint."""
    rng = np.random.default_rng(seed)
    K, kf_cap = t["kf_mappoint"].shape
    I = len(sizes)
    pools = [[i for i in rng.permutation(int(t["kf_n"][k])) if t["kf_mappoint"][k, i] < 0 and (not by_keypoint or i < list_cap)]
             for k in range(K)]
    ls = dict(kf1=np.array([i % K for i in range(I)], np.int32), n_list=np.array(sizes, np.int32),
              idx1=np.full((I, list_cap), -7, np.int32), xw=rng.normal(size=(I, list_cap, 3)).astype(np.float32))
    if two:
        ls["kf2"] = np.array([(i + 1) % K for i in range(I)], np.int32)
        ls["idx2"] = np.full((I, list_cap), -7, np.int32)
    if values:
        ls["normal"] = rng.normal(size=(I, list_cap, 3)).astype(np.float32)
        ls["max_distance"] = (rng.random((I, list_cap)) + 2).astype(np.float32)
        ls["min_distance"] = rng.random((I, list_cap)).astype(np.float32)
    for i in range(I):
        for j in range(sizes[i]):
            ls["idx1"][i, j] = pools[ls["kf1"][i]].pop()
            if two:
                ls["idx2"][i, j] = pools[ls["kf2"][i]].pop()
        if by_keypoint:
            ls["idx1"][i, :sizes[i]] = np.sort(ls["idx1"][i, :sizes[i]])
        for d in range(min(drops, sizes[i])):
            j = int(rng.integers(0, sizes[i]))
            which = "idx2" if two and d % 2 else "idx1"
            n = int(t["kf_n"][ls["kf2" if which == "idx2" else "kf1"][i]])
            ls[which][i, j] = -1 if d % 3 == 0 or n >= kf_cap else n   # (the host entries refuse an index at or past kf_cap)
    for i in range(1, I, 2 if two else I):                    # odd items: kf1 > kf2 where the slots allow, the row still ascends
        if two:
            ls["kf1"][i], ls["kf2"][i] = ls["kf2"][i], ls["kf1"][i]
            ls["idx1"][i], ls["idx2"][i] = ls["idx2"][i].copy(), ls["idx1"][i].copy()
    if frames is not None:
        F, kp_cap = frames
        ls["item_frame"] = np.array([i if i < F else -1 for i in range(I)], np.int32)   # a frame is one keyframe's
        ls["frame_mappoint"] = np.full((F, kp_cap), -3, np.int32)
    return ls


def n_valid(t, ls):
    """The entries a batch creates (tests size `alloc` and the rows with it)."""
    n = 0
    for i in range(len(ls["kf1"])):
        for j in range(int(ls["n_list"][i])):
            k1 = int(ls["kf1"][i])
            good = 0 <= ls["idx1"][i, j] < t["kf_n"][k1]
            if "kf2" in ls and ls["kf2"][i] >= 0:
                good = good and 0 <= ls["idx2"][i, j] < t["kf_n"][int(ls["kf2"][i])]
            n += bool(good)
    return n


def make_frames(F=3, kp_cap=40, seed=2):
    """FRAME_KEYS of creation.py; frame 1 is full, the others are not."""
    rng = np.random.default_rng(seed)
    fr = dict(frame_n=rng.integers(kp_cap // 3, kp_cap, F).astype(np.int32))
    if F > 1:
        fr["frame_n"][1] = kp_cap
    fr["frame_mappoint"] = rng.integers(-1, 50, (F, kp_cap)).astype(np.int32)
    fr["kp_un"] = rng.integers(0, 2 ** 30, (F, kp_cap, 7)).astype(np.int32)
    fr["kp_octave"] = rng.integers(0, 8, (F, kp_cap)).astype(np.int32)
    fr["kp_uright"] = np.where(rng.random((F, kp_cap)) < 0.5, -1.0, rng.random((F, kp_cap)) * 600).astype(np.float32)
    fr["kp_depth"] = np.where(fr["kp_uright"] < 0, -1.0, rng.random((F, kp_cap)) * 30).astype(np.float32)
    fr["kp_desc"] = rng.integers(0, 256, (F, kp_cap, 32), dtype=np.uint8)
    fr["pose"] = rng.normal(size=(F, 12)).astype(np.float32)
    fr["camera"] = (rng.random((F, 5)) * 500).astype(np.float32)
    return fr


def make_keyframes(K=5, kf_cap=44, conn_cap=6, seed=3):
    """KEYFRAME_KEYS of creation.py, every row full of recognisable values."""
    rng = np.random.default_rng(seed)
    i32 = lambda *s: rng.integers(100, 200, s).astype(np.int32)   # noqa: E731
    f32 = lambda *s: rng.normal(size=s).astype(np.float32)        # noqa: E731
    u8 = lambda *s: rng.integers(2, 9, s).astype(np.uint8)        # noqa: E731
    return dict(kf_id=i32(K), kf_n=i32(K), kf_mappoint=i32(K, kf_cap), kf_keypoint=i32(K, kf_cap, 7), kf_kp_octave=i32(K, kf_cap),
                kf_uright=f32(K, kf_cap), kf_depth=f32(K, kf_cap), kf_desc=rng.integers(0, 256, (K, kf_cap, 32), dtype=np.uint8),
                kf_pose=f32(K, 12), kf_camera=f32(K, 6), kf_bad=u8(K), kf_not_erase=u8(K), kf_to_be_erased=u8(K), kf_parent=i32(K),
                kf_first_connection=u8(K), conn_slot=i32(K, conn_cap), conn_weight=i32(K, conn_cap), n_conn=i32(K),
                ord_slot=i32(K, conn_cap), ord_weight=i32(K, conn_cap), n_ord=i32(K), kf_covis=i32(K, COVIS))


def bits(a):
    """What is compared: floats as their bits."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_same(got, want, keys=None):
    for k in keys or want:
        assert k in got, k
        assert np.array_equal(bits(got[k]), bits(want[k])), k
