"""Sequential numpy restatement of where the map grows, following the reference line by line, point by point:
KeyFrame::KeyFrame(const Frame&, ...) (src/KeyFrame.cc:51-64) and MapPoint::MapPoint(Xw, referenceKF, map)
(src/MapPoint.cc:44-56) with the calls after a construction (src/Tracking.cc:724-736, :981-997, :1104-1126;
src/LocalMapping.cc:562-575), on the slot tables of include/orbslam2_amd.h ("Map creation").  A MapPoint's id is its slot:
`alloc` plays nextId.  Shares no code with csrc/mk_create.h."""
import numpy as np

OK, OVERFLOW = 0, 1
COVIS = 10

PER_KEYPOINT = (("kf_mappoint", "frame_mappoint"), ("kf_keypoint", "kp_un"), ("kf_kp_octave", "kp_octave"), ("kf_uright", "kp_uright"),
                ("kf_depth", "kp_depth"), ("kf_desc", "kp_desc"))
MAP_UPDATED = ("kf_mappoint", "mp_bad", "mp_xw", "mp_normal", "mp_max_min", "mp_nobs", "mp_found", "mp_visible", "mp_replaced",
               "mp_first_kf_id", "mp_ref_kf", "mp_desc", "mp_obs_kf", "mp_obs_idx")


def insert_keyframes(frames, keyframes, item_frame, item_kf, item_id, item_baseline=None, skip_outside=True):
    """Returns updated copies of the tables `keyframes` holds."""
    kf = {k: np.array(v, copy=True) for k, v in keyframes.items() if v is not None}
    F = len(frames["frame_n"])
    K = len(next(iter(kf.values())))
    for it in range(len(item_frame)):
        f, k = int(item_frame[it]), int(item_kf[it])
        if not (0 <= f < F and 0 <= k < K):
            assert skip_outside
            continue
        N = int(frames["frame_n"][f])
        # :55-58 N(frame.N), keypointsUn, uright, depth, descriptorsL, mappoints_(frame.mappoints)
        for dst, src in PER_KEYPOINT:
            if dst in kf:
                kf[dst][k, :N] = frames[src][f, :N]
        if "kf_mappoint" in kf:
            kf["kf_mappoint"][k, N:] = -1                    # the slots a keyframe of N keypoints does not have
        state = dict(kf_n=N, kf_id=item_id[it],              # :62 id = nextId++ (the caller's counter)
                     kf_first_connection=1, kf_parent=-1, kf_not_erase=0, kf_to_be_erased=0, kf_bad=0,   # :59-60
                     n_conn=0, n_ord=0)                      # empty connectionTo_ / orderedConnectedKeyFrames_
        for name, v in state.items():
            if name in kf:
                kf[name][k] = v
        for name, v in (("conn_slot", -1), ("conn_weight", 0), ("ord_slot", -1), ("ord_weight", 0), ("kf_covis", -1)):
            if name in kf:
                kf[name][k, :] = v
        if "kf_pose" in kf:
            kf["kf_pose"][k] = frames["pose"][f]             # :63 SetPose(frame.pose)
        if "kf_camera" in kf:
            kf["kf_camera"][k, :5] = frames["camera"][f]     # :55 camera(frame.camera)
            kf["kf_camera"][k, 5] = item_baseline[it]
    return kf


class Map:
    def __init__(self, t):
        self.t = {k: np.array(v, copy=True) for k, v in t.items() if v is not None}
        t = self.t
        self.K, self.M, self.kf_cap = len(t["kf_n"]), len(t["mp_bad"]), t["kf_mappoint"].shape[1]
        self.n_obs = len(t["mp_obs_kf"])

    def row(self, p):
        e0 = min(max(int(self.t["mp_obs_off"][p]), 0), self.n_obs)
        return e0, min(max(int(self.t["mp_obs_off"][p + 1]), e0), self.n_obs)

    def n_keypoints(self, k):
        return min(max(int(self.t["kf_n"][k]), 0), self.kf_cap)

    # MapPoint::MapPoint(Xw, referenceKF, map), src/MapPoint.cc:44-56
    def construct(self, p, Xw, referenceKF):
        t = self.t
        t["mp_first_kf_id"][p] = t["kf_id"][referenceKF]     # firstKFid(referenceKF->id)
        t["mp_nobs"][p] = 0                                  # nobservations_(0)
        t["mp_ref_kf"][p] = referenceKF
        t["mp_visible"][p] = t["mp_found"][p] = 1
        t["mp_bad"][p] = 0
        t["mp_replaced"][p] = -1
        if "mp_max_min" in t:
            t["mp_max_min"][p] = 0                           # minDistance_(0), maxDistance_(0)
        t["mp_xw"][p] = Xw
        if "mp_normal" in t:
            t["mp_normal"][p] = 0                            # normal_ = Vec3D::zeros()
        e0, e1 = self.row(p)
        t["mp_obs_kf"][e0:e1] = t["mp_obs_idx"][e0:e1] = -1  # an empty observations_

    # MapPoint::AddObservation, src/MapPoint.cc:109-122; the map is ordered by keyframe slot
    def add_observation(self, p, keyframe, idx):
        t = self.t
        e0, e1 = self.row(p)
        obs = [(int(t["mp_obs_kf"][e]), int(t["mp_obs_idx"][e])) for e in range(e0, e1) if t["mp_obs_kf"][e] >= 0]
        if any(o == keyframe for o, _ in obs):
            return
        obs = sorted(obs + [(keyframe, idx)])
        assert len(obs) <= e1 - e0
        for j, (o, i) in enumerate(obs):
            t["mp_obs_kf"][e0 + j], t["mp_obs_idx"][e0 + j] = o, i
        t["mp_nobs"][p] += 2 if t["kf_uright"][keyframe, idx] >= 0 else 1

    # MapPoint::ComputeDistinctiveDescriptors, src/MapPoint.cc:256-320, for the one or two observations of a new point
    def compute_distinctive_descriptors(self, p):
        t = self.t
        if "mp_desc" not in t:
            return
        e0, e1 = self.row(p)
        descriptors = []
        for e in range(e0, e1):
            keyframe, idx = int(t["mp_obs_kf"][e]), int(t["mp_obs_idx"][e])
            if keyframe < 0:
                continue
            if not ("kf_bad" in t and t["kf_bad"][keyframe]):
                descriptors.append(t["kf_desc"][keyframe, idx])
        if not descriptors:
            return
        N = len(descriptors)
        assert N <= 2
        distances = [[0 if i == j else int(np.unpackbits(descriptors[i] ^ descriptors[j]).sum()) for j in range(N)] for i in range(N)]
        bestMedian, bestIdx = 2 ** 31 - 1, 0
        for i in range(N):
            median = sorted(distances[i])[(N - 1) // 2]
            if median < bestMedian:
                bestMedian, bestIdx = median, i
        t["mp_desc"][p] = descriptors[bestIdx]


def entry_valid(m, lists, by_keypoint, i, j):
    K, k1 = m.K, int(lists["kf1"][i])
    k2 = int(lists["kf2"][i]) if lists.get("kf2") is not None else -1
    if not 0 <= k1 < K or (k2 != -1 and not 0 <= k2 < K) or k1 == k2:
        return False
    i1 = int(lists["idx1"][i, j])
    if not 0 <= i1 < m.n_keypoints(k1) or (by_keypoint and i1 >= lists["idx1"].shape[1]):
        return False
    return k2 == -1 or 0 <= int(lists["idx2"][i, j]) < m.n_keypoints(k2)


def create_points(tables, lists, alloc, by_keypoint=False, recent=None, n_recent=0):
    """Returns (updated copies of MAP_UPDATED and frame_mappoint, out) as creation.CreatePoints does."""
    m = Map(tables)
    t = m.t
    I, list_cap = lists["idx1"].shape
    n_list = [min(max(int(n), 0), list_cap) for n in lists["n_list"]]
    entries = [(i, j) for i in range(I) for j in range(n_list[i]) if entry_valid(m, lists, by_keypoint, i, j)]
    given, alloc = alloc, min(max(int(alloc), 0), m.M)
    out = dict(alloc=np.array([given], np.int32), status=np.array([OK], np.int32), needed=np.array([alloc + len(entries), -1], np.int32),
               created=np.full((I, list_cap), -1, np.int32), n_created=np.zeros(I, np.int32))
    frame_mappoint = None if lists.get("frame_mappoint") is None else np.array(lists["frame_mappoint"], copy=True)
    if recent is not None:
        out["recent"], out["n_recent"] = np.array(recent, copy=True), np.array([n_recent], np.int32)
    # everything is checked before anything is written
    fits = alloc + len(entries) <= m.M
    short = -1
    if fits:
        for r, (i, j) in enumerate(entries):
            e0, e1 = m.row(alloc + r)
            two = lists.get("kf2") is not None and lists["kf2"][i] != -1
            if e1 - e0 < (2 if two else 1):
                short = alloc + r
                break
    out["needed"][1] = short
    if not fits or short >= 0 or (recent is not None and n_recent + len(entries) > len(recent)):
        out["status"][0] = OVERFLOW
        upd = {k: t[k] for k in MAP_UPDATED if k in t}
        if frame_mappoint is not None:
            upd["frame_mappoint"] = frame_mappoint
        return upd, out
    for i, j in entries:
        keyframe1, idx1 = int(lists["kf1"][i]), int(lists["idx1"][i, j])
        two = lists.get("kf2") is not None and lists["kf2"][i] != -1
        v = idx1 if by_keypoint else j
        p = alloc
        alloc += 1                                           # id = nextId++
        m.construct(p, lists["xw"][i, v], keyframe1)         # new MapPoint(Xw, keyframe1, map)
        m.add_observation(p, keyframe1, idx1)
        t["kf_mappoint"][keyframe1, idx1] = p                # keyframe1->AddMapPoint(mappoint, idx1)
        if two:
            keyframe2, idx2 = int(lists["kf2"][i]), int(lists["idx2"][i, j])
            m.add_observation(p, keyframe2, idx2)
            t["kf_mappoint"][keyframe2, idx2] = p
        m.compute_distinctive_descriptors(p)
        # UpdateNormalAndDepth: the values the producer computed, or the caller's next call
        if lists.get("normal") is not None and "mp_normal" in t:
            t["mp_normal"][p] = lists["normal"][i, v]
        if "mp_max_min" in t:
            if lists.get("max_distance") is not None:
                t["mp_max_min"][p, 0] = lists["max_distance"][i, v]
            if lists.get("min_distance") is not None:
                t["mp_max_min"][p, 1] = lists["min_distance"][i, v]
        if frame_mappoint is not None:                       # currFrame.mappoints[i] = newpoint
            f = int(lists["item_frame"][i])
            if 0 <= f < frame_mappoint.shape[0] and idx1 < frame_mappoint.shape[1]:
                frame_mappoint[f, idx1] = p
        out["created"][i, j] = p
        out["n_created"][i] += 1
        if recent is not None:                               # recentAddedMapPoints_.push_back(mappoint)
            out["recent"][int(out["n_recent"][0])] = p
            out["n_recent"][0] += 1
    out["alloc"][0] = alloc
    upd = {k: t[k] for k in MAP_UPDATED if k in t}
    if frame_mappoint is not None:
        upd["frame_mappoint"] = frame_mappoint
    return upd, out
