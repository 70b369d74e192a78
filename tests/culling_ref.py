"""Restatement of LocalMapping::MapPointCulling and KeyFrameCulling (src/LocalMapping.cc:335-369, 641-701) with
MapPoint::SetBadFlag and EraseObservation (src/MapPoint.cc:124-182), KeyFrame::SetBadFlag and EraseConnection
(src/KeyFrame.cc:379-489) on the slot tables of orb_slam2_refactored_amd/culling.py, line by line: slots for pointers, a
list of [keyframe, index] per point for observations_ (in the caller's CSR order, which stands in for pointer order), dicts
for connectionTo_.  Plain Python and numpy; what the device and csrc/mm_cull.h are compared with, exactly.

An erased observation stays in the CSR as keyframe -1 (compact_observations drops those).  Where the device does not trust
what it reads, this does the same: a slot, offset or index outside its table is skipped.  Departures from the reference, as
include/orbslam2_amd.h states them: a target that is already bad is skipped; a reference keyframe is replaced by the first
remaining observation in CSR order; the children are walked in ascending slot order."""
import numpy as np

import map_maintenance_ref as MR

F32 = np.float32
COVIS = MR.COVIS
POINT_UPDATED = ("mp_bad", "kf_mappoint", "mp_obs_kf")
KEYFRAME_UPDATED = ("kf_bad", "kf_to_be_erased", "kf_tcp", "kf_mappoint", "mp_bad", "mp_nobs", "mp_ref_kf", "mp_obs_kf",
                    "conn_slot", "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord", "kf_parent", "kf_covis")


class Map:
    def __init__(self, t):
        self.t = t = {k: np.array(v, copy=True) for k, v in t.items()}
        self.K, self.M, self.kf_cap = len(t["kf_n"]), len(t["mp_bad"]), t["kf_mappoint"].shape[1]
        n_obs = len(t["mp_obs_kf"])
        self.range = [(max(int(t["mp_obs_off"][p]), 0), min(int(t["mp_obs_off"][p + 1]), n_obs)) for p in range(self.M)]
        self.trace = []                  # what the cases assert on

    def observations(self, p):
        """(entry, keyframe, index) of the observations of p that are in the table, in CSR order."""
        e0, e1 = self.range[p]
        return [(e, int(self.t["mp_obs_kf"][e]), int(self.t["mp_obs_idx"][e])) for e in range(e0, e1)
                if 0 <= self.t["mp_obs_kf"][e] < self.K]

    # MapPoint::SetBadFlag
    def set_bad_flag(self, p):
        t = self.t
        t["mp_bad"][p] = 1                                   # bad_ = true
        e0, e1 = self.range[p]
        for e, o, idx in self.observations(p):
            if 0 <= idx < self.kf_cap:
                if t["kf_mappoint"][o, idx] != -1:
                    self.trace.append(("cleared", p, o))
                t["kf_mappoint"][o, idx] = -1                # keyframe->EraseMapPointMatch(observation.second)
        t["mp_obs_kf"][e0:e1] = -1                           # observations_.clear()

    # MapPoint::EraseObservation
    def erase_observation(self, p, k):
        t = self.t
        hit = [(e, idx) for e, o, idx in self.observations(p) if o == k]
        if not hit:                                          # if (observations_.count(keyframe))
            return
        e, idx = hit[0]
        stereo = 0 <= idx < self.kf_cap and t["kf_uright"][k, idx] >= 0
        t["mp_nobs"][p] -= 2 if stereo else 1
        t["mp_obs_kf"][e] = -1                               # observations_.erase(keyframe)
        if t["mp_ref_kf"][p] == k:
            left = self.observations(p)
            t["mp_ref_kf"][p] = left[0][1] if left else -1
        if t["mp_nobs"][p] <= 2:
            self.trace.append(("erased_bad", p, k))
            self.set_bad_flag(p)


def map_point_culling(tables, recent, cur_kf_id, monocular):
    """Returns (the updated copies of POINT_UPDATED, the list that is left, the branch each entry took)."""
    with np.errstate(all="ignore"):
        m = Map(tables)
        t = m.t
        min_observation = 2 if monocular else 3
        kept, branch = [], []
        for p in [int(x) for x in recent]:
            if p < 0 or p >= m.M:
                branch.append("outside")
                continue
            first_kf_id = int(t["mp_first_kf_id"][p])
            if t["mp_bad"][p]:
                branch.append("bad")
            elif F32(t["mp_found"][p]) / F32(t["mp_visible"][p]) < F32(0.25):
                m.set_bad_flag(p)
                branch.append("ratio")
            elif cur_kf_id - first_kf_id >= 2 and t["mp_nobs"][p] <= min_observation:
                m.set_bad_flag(p)
                branch.append("few")
            elif cur_kf_id - first_kf_id >= 3:
                branch.append("old")
            else:
                kept.append(p)
                branch.append("kept")
        return {k: t[k] for k in POINT_UPDATED}, np.array(kept, np.int32), branch


class Connections:
    def __init__(self, t, K):
        self.t, self.K = t, K
        self.cap = t["conn_slot"].shape[1]

    def conn(self, k):
        n = min(max(int(self.t["n_conn"][k]), 0), self.cap)
        return {int(s): int(w) for s, w in list(zip(self.t["conn_slot"][k, :n], self.t["conn_weight"][k, :n]))[::-1]}   # the first entry of a slot counts

    def ordered(self, k):
        n = min(max(int(self.t["n_ord"][k]), 0), self.cap)
        return [int(s) for s in self.t["ord_slot"][k, :n]]

    def write(self, k, conn):
        t = self.t
        rows = sorted(conn.items())
        order = sorted(((w, s) for s, w in conn.items()), reverse=True)   # UpdateBestCovisibles
        for name, row in (("conn_slot", [s for s, _ in rows]), ("conn_weight", [w for _, w in rows]),
                          ("ord_slot", [s for _, s in order]), ("ord_weight", [w for w, _ in order])):
            t[name][k] = -1 if name.endswith("slot") else 0
            t[name][k, :len(row)] = row
        t["n_conn"][k] = t["n_ord"][k] = len(rows)
        t["kf_covis"][k] = -1
        t["kf_covis"][k, :min(len(order), COVIS)] = [s for _, s in order[:COVIS]]


def pose_inverse(T):
    R, tr = T[:9].reshape(3, 3), T[9:]
    o = np.zeros(12, F32)
    o[:9] = R.T.reshape(-1)
    for i in range(3):
        s = F32(0)
        for k in range(3):
            s = F32(s + F32(F32(-R[k, i]) * tr[k]))
        o[9 + i] = s
    return o


def pose_mul(A, B):
    o = np.zeros(12, F32)
    for i in range(3):
        s = F32(0)
        for k in range(3):
            s = F32(s + F32(A[3 * i + k] * B[9 + k]))
        o[9 + i] = F32(s + A[9 + i])
        for j in range(3):
            s = F32(0)
            for k in range(3):
                s = F32(s + F32(A[3 * i + k] * B[3 * k + j]))
            o[3 * i + j] = s
    return o


def redundancy(m, k, monocular, th_depth):
    """(npoints, nredundant) of target k."""
    t = m.t
    npoints = nredundant = 0
    for i1 in range(min(max(int(t["kf_n"][k]), 0), m.kf_cap)):
        p = int(t["kf_mappoint"][k, i1])
        if p < 0 or p >= m.M or t["mp_bad"][p]:
            continue
        if not monocular:
            if t["kf_depth"][k, i1] > F32(th_depth) or t["kf_depth"][k, i1] < 0:
                continue
        npoints += 1
        if t["mp_nobs"][p] > 3:
            target_scale = int(t["kf_kp_octave"][k, i1])
            nobservations = 0
            for _, o, i2 in m.observations(p):
                if o == k or not 0 <= i2 < m.kf_cap:
                    continue
                if int(t["kf_kp_octave"][o, i2]) <= target_scale + 1:
                    nobservations += 1
                    if nobservations >= 3:
                        break
            if nobservations >= 3:
                nredundant += 1
    return npoints, nredundant


def set_bad_flag(m, G, k):
    """KeyFrame::SetBadFlag past the id and notErase_ tests."""
    t, K = m.t, m.K
    for v in G.conn(k):                                      # v.first->EraseConnection(this)
        if v < 0 or v >= K or v == k:
            continue
        c = G.conn(v)
        if k in c:
            del c[k]
            G.write(v, c)
    for i in range(min(max(int(t["kf_n"][k]), 0), m.kf_cap)):
        p = int(t["kf_mappoint"][k, i])
        if 0 <= p < m.M:
            m.erase_observation(p, k)
    G.write(k, {})                                           # connectionTo_.clear(); orderedConnectedKeyFrames_.clear()
    parent = int(t["kf_parent"][k])
    candidates = [parent] if 0 <= parent < K else []
    children = [c for c in range(K) if c != k and t["kf_parent"][c] == k and not t["kf_bad"][c]]
    while children:
        found, max_count, child_kf, parent_kf = False, -1, None, None
        for child in children:
            conn = G.conn(child)
            for connected in G.ordered(child):
                if connected < 0 or connected >= K:
                    continue
                for candidate in candidates:
                    if t["kf_id"][connected] == t["kf_id"][candidate]:
                        weight = conn.get(connected, 0)
                        if weight > max_count:
                            child_kf, parent_kf, max_count, found = child, connected, weight, True
        if not found:
            break
        t["kf_parent"][child_kf] = parent_kf
        m.trace.append(("adopted", child_kf, parent_kf, parent_kf in candidates[1:]))   # through a child adopted earlier?
        candidates.append(child_kf)
        children.remove(child_kf)
    for child in children:
        m.trace.append(("fell_back", child, parent))
        t["kf_parent"][child] = parent
    if 0 <= parent < K:
        t["kf_tcp"][k] = pose_mul(t["kf_pose"][k], pose_inverse(t["kf_pose"][parent]))
    t["kf_bad"][k] = 1


def keyframe_culling(tables, cur, monocular, th_depth):
    """Returns (the updated copies of KEYFRAME_UPDATED, culled (conn_cap entries, -1 padded), n_culled, the trace)."""
    m = Map(tables)
    t = m.t
    G = Connections(t, m.K)
    culled = np.full(G.cap, -1, np.int32)
    n = 0
    targets = G.ordered(cur) if 0 <= cur < m.K else []
    for k in targets:
        if k < 0 or k >= m.K or t["kf_id"][k] == 0 or t["kf_bad"][k]:
            continue
        npoints, nredundant = redundancy(m, k, monocular, th_depth)
        m.trace.append(("counted", k, npoints, nredundant))
        if nredundant > 0.9 * npoints:
            if t["kf_not_erase"][k]:
                t["kf_to_be_erased"][k] = 1
                m.trace.append(("held", k))
                continue
            set_bad_flag(m, G, k)
            culled[n] = k
            n += 1
    return {k: t[k] for k in KEYFRAME_UPDATED}, culled, n, m.trace


def compact_observations(mp_obs_off, mp_obs_kf, mp_obs_idx):
    """The CSR without the erased entries, the order within a point kept; the arrays keep their capacity."""
    n_obs, M = len(mp_obs_kf), len(mp_obs_off) - 1
    off, kf, idx = np.zeros(M + 1, np.int32), np.array(mp_obs_kf, copy=True), np.array(mp_obs_idx, copy=True)
    at = 0
    for p in range(M):
        off[p] = at
        for e in range(max(int(mp_obs_off[p]), 0), min(int(mp_obs_off[p + 1]), n_obs)):
            if mp_obs_kf[e] == -1:
                continue
            if at < n_obs:
                kf[at], idx[at] = mp_obs_kf[e], mp_obs_idx[e]
            at += 1
    off[M] = at
    return off, kf, idx


def live_children(kf_parent, kf_bad):
    """GetChildren() after EraseChild: the inverse of kf_parent with the bad keyframes left out as children."""
    K = len(kf_parent)
    lists = [[k for k in range(K) if kf_parent[k] == p and not kf_bad[k]] for p in range(K)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return off, np.array([k for x in lists for k in x], np.int32)
