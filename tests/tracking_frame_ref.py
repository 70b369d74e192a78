"""Sequential numpy restatement of Tracking's per-frame state as include/orbslam2_amd.h ("Tracking's per-frame state")
states it, read from src/Tracking.cc (DiscardOutliers :187-211, TrackWithMotionModel :220-255, NeedNewKeyFrame :490-511,
TrackLocalMap :664-680, CreateMapPoints :685-743, CreateMapPointsVO :745-786, GetReplaced :808-814, StereoInitialization
:980-997, the end of Update :1259-1313), src/Optimizer.cc:157-162 and :355-415, src/ORBmatcher.cc:1283-1311,
src/KeyFrame.cc:198-220, include/CameraPose.h.  One loop per reference loop, one frame at a time, float32 scalars in
the reference's operand order.  Every function works in place on a dict of frame tables `fr` (stride kp_cap) and a dict of
map tables `m`, as the library does; tests/test_tracking_frame_ref.py pins each gate with hand-built frames."""
import numpy as np

from newpoints_ref import Frame as LmFrame
from newpoints_ref import dot3 as lm_dot3

f32 = np.float32
MERGE, REPLACE = 0, 1
DISCARD, LOCAL_MAP = 0, 1
KEYFRAME, VO, INIT = 0, 1, 2
CLOSEST = 100


def ok(p, n):
    """A slot read from a table is not trusted: outside [0, n) it is null."""
    return 0 <= int(p) < int(n)


def n_of(fr, f):
    return min(max(int(fr["frame_n"][f]), 0), fr["frame_mappoint"].shape[1])


def matx_dot(a, b):
    """cv::Matx product element: s = 0; s += a(k) * b(k)."""
    s = f32(0)
    for k in range(3):
        s = f32(s + f32(f32(a[k]) * f32(b[k])))
    return s


def pose_product(A, B):
    """CameraPose::operator* on 12 floats (Rcw row-major, tcw): t = A.R * B.t + A.t, then R = A.R * B.R."""
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    RA, RB = A[:9].reshape(3, 3), B[:9].reshape(3, 3)
    t = [f32(matx_dot(RA[i], B[9:]) + A[9 + i]) for i in range(3)]
    R = [matx_dot(RA[i], RB[:, j]) for i in range(3) for j in range(3)]
    return np.array(R + t, f32)


def motion_of(L, Cp, baseline, monocular):
    """0, 1 = forward, 2 = backward (src/ORBmatcher.cc:1286-1288)."""
    L, Cp = np.asarray(L, f32), np.asarray(Cp, f32)
    R = Cp[:9].reshape(3, 3)
    inv = [matx_dot(-R[:, i], Cp[9:]) for i in range(3)]   # Invt() = (-R^T) * t
    z = f32(matx_dot(L[6:9], inv) + L[11])
    forward = bool(z > f32(baseline)) and not monocular
    backward = bool(-z > f32(baseline)) and not monocular
    return 1 if forward else (2 if backward else 0)


def project(P, cam, bd, Xw):
    """The tests of src/ORBmatcher.cc:1301-1311: (valid, u, v, ur)."""
    P, cam, bd, Xw = (np.asarray(a, f32) for a in (P, cam, bd, Xw))
    none = (0, f32(0), f32(0), f32(0))
    with np.errstate(all="ignore"):
        x = ((P[0] * Xw[0] + P[1] * Xw[1]) + P[2] * Xw[2]) + P[9]
        y = ((P[3] * Xw[0] + P[4] * Xw[1]) + P[5] * Xw[2]) + P[10]
        z = ((P[6] * Xw[0] + P[7] * Xw[1]) + P[8] * Xw[2]) + P[11]
        if z < f32(0):
            return none
        invZ = f32(1) / z
        u = invZ * cam[0] * x + cam[2]
        v = invZ * cam[1] * y + cam[3]
        ur = u - cam[4] / z
        if not (u >= bd[0] and u < bd[1] and v >= bd[2] and v < bd[3]):
            return none
    return (1, u, v, ur)


def unproject(P, cam, u, v, Z, vo=False):
    """CameraUnProjection::uvZToWorld, or Frame::UnprojectStereo (vo), with the frame's pose."""
    P = np.asarray(P, f32)
    T = np.concatenate([P[:9].reshape(3, 3), P[9:].reshape(3, 1)], 1).reshape(-1)
    fm = LmFrame(T, np.concatenate([np.asarray(cam, f32)[:5], [f32(0)]]))
    u, v, Z = f32(u), f32(v), f32(Z)
    with np.errstate(all="ignore"):
        if not vo:
            return fm.uvz_to_world(u, v, Z)
        c = np.array([f32(f32(f32(u - fm.cx) * Z) * fm.invfx), f32(f32(f32(v - fm.cy) * Z) * fm.invfy), Z], f32)
        return np.array([f32(lm_dot3(fm.Rwc[i], c) + fm.Ow[i]) for i in range(3)], f32)


# ---- 1
def apply_matches(fr, mode, kp_match, src, src_row=None, n_mappoints=None):
    M = n_mappoints
    for f in range(len(fr["frame_n"])):
        row = f if src_row is None else int(src_row[f])
        for i in range(n_of(fr, f)):
            k = int(kp_match[f, i])
            if not (ok(row, src.shape[0]) and ok(k, src.shape[1])):
                if mode == REPLACE:
                    fr["frame_mappoint"][f, i] = -1
                continue
            p = int(src[row, k])
            fr["frame_mappoint"][f, i] = p if ok(p, M) else -1


# ---- 2
def pose_edges(fr, m, inv_sigma2_table):
    """The gather of src/Optimizer.cc:355-411 as the arrays of a pose batch (rows past the last edge: zero)."""
    F, cap = fr["frame_mappoint"].shape
    M, L = len(m["mp_xw"]), len(inv_sigma2_table)
    e = dict(edge_begin=np.zeros(F + 1, np.int32), pose_R=fr["pose"][:, :9].astype(np.float64),
             pose_t=fr["pose"][:, 9:].astype(np.float64), cam=fr["camera"].astype(np.float64), xw=np.zeros((F * cap, 3)),
             obs=np.zeros((F * cap, 3)), inv_sigma2=np.zeros(F * cap), edge_kp=np.zeros(F * cap, np.int32))
    n = 0
    for f in range(F):
        for i in range(n_of(fr, f)):
            p = int(fr["frame_mappoint"][f, i])
            if not ok(p, M):
                continue
            fr["frame_outlier"][f, i] = 0
            e["xw"][n] = m["mp_xw"][p]
            e["obs"][n] = (fr["kp_xy"][f, i, 0], fr["kp_xy"][f, i, 1], fr["kp_uright"][f, i])
            e["inv_sigma2"][n] = inv_sigma2_table[min(max(int(fr["kp_octave"][f, i]), 0), L - 1)]
            e["edge_kp"][n] = i
            n += 1
        e["edge_begin"][f + 1] = n
    return e


# ---- 3
def finish_pose(fr, m, mode, edges, result, localization=False, stereo=False):
    F, cap = fr["frame_mappoint"].shape
    M = len(m["mp_nobs"])
    out = dict(n_inliers=np.zeros(F, np.int32), discarded=np.zeros((F, cap), np.int32), n_discarded=np.zeros(F, np.int32))
    for f in range(F):
        n = n_of(fr, f)
        e0, e1 = int(edges["edge_begin"][f]), int(edges["edge_begin"][f + 1])
        if e1 - e0 >= 3:   # :413-415
            for e in range(e0, e1):
                k = int(edges["edge_kp"][e])
                if ok(k, n):
                    fr["frame_outlier"][f, k] = 1 if result["outlier"][e] else 0
            fr["pose"][f, :9] = np.asarray(result["pose_R"][f], np.float64).reshape(-1).astype(f32)   # one rounding
            fr["pose"][f, 9:] = np.asarray(result["pose_t"][f], np.float64).astype(f32)
        c = 0
        for i in range(n):
            p = int(fr["frame_mappoint"][f, i])
            if not ok(p, M):
                continue
            if mode == DISCARD:
                if fr["frame_outlier"][f, i]:
                    fr["frame_mappoint"][f, i] = -1
                    fr["frame_outlier"][f, i] = 0
                    out["discarded"][f, out["n_discarded"][f]] = p
                    out["n_discarded"][f] += 1
                elif m["mp_nobs"][p] > 0:
                    c += 1
            else:
                if not fr["frame_outlier"][f, i]:
                    m["mp_found"][p] += 1
                    if localization or m["mp_nobs"][p] > 0:
                        c += 1
                elif stereo:
                    fr["frame_mappoint"][f, i] = -1
        out["n_inliers"][f] = c
    return out


# ---- 4
def motion_project(cur, last, m, velocity, baseline, monocular):
    F, capC = cur["frame_mappoint"].shape
    capL = last["frame_mappoint"].shape[1]
    M = len(m["mp_nobs"])
    o = dict(motion=np.zeros(F, np.int32), kp_begin=(np.arange(F + 1) * capC).astype(np.int32),
             mp_begin=(np.arange(F + 1) * capL).astype(np.int32), kp_claimed=np.ones((F, capC), np.uint8),
             mp_valid=np.zeros((F, capL), np.uint8), mp_proj=np.zeros((F, capL, 3), f32), mp_octave=np.zeros((F, capL), np.int32),
             mp_desc=np.zeros((F, capL, 32), np.uint8), mp_has_obs=np.zeros((F, capL), np.uint8), mp_angle=np.zeros((F, capL), f32))
    for f in range(F):
        nL = n_of(last, f)
        for i in range(nL):   # :808-814
            p = int(last["frame_mappoint"][f, i])
            if ok(p, M) and ok(m["mp_replaced"][p], M):
                last["frame_mappoint"][f, i] = m["mp_replaced"][p]
        cur["pose"][f] = pose_product(velocity[f], last["pose"][f])   # :225
        nC = n_of(cur, f)
        cur["frame_mappoint"][f, :nC] = -1   # :232
        o["kp_claimed"][f, :nC] = 0
        o["motion"][f] = motion_of(last["pose"][f], cur["pose"][f], baseline[f], monocular)
        for i in range(nL):
            o["mp_octave"][f, i] = last["kp_octave"][f, i]
            o["mp_angle"][f, i] = last["kp_angle"][f, i]
            p = int(last["frame_mappoint"][f, i])
            if not ok(p, M):
                continue
            o["mp_has_obs"][f, i] = 1 if m["mp_nobs"][p] > 0 else 0
            o["mp_desc"][f, i] = m["mp_desc"][p]
            if last["frame_outlier"][f, i]:
                continue
            valid, u, v, ur = project(cur["pose"][f], cur["camera"][f], cur["bounds"][f], m["mp_xw"][p])
            o["mp_valid"][f, i] = valid
            o["mp_proj"][f, i] = (u, v, ur)
    return o


def depth_valid(z):
    return bool(f32(z) > f32(0))


# ---- 5
def tracked_map_points(m, k, min_obs):
    """KeyFrame::TrackedMapPoints (src/KeyFrame.cc:198-220)."""
    if not ok(k, len(m["kf_n"])):
        return 0
    M, c = len(m["mp_nobs"]), 0
    for i in range(min(max(int(m["kf_n"][k]), 0), m["kf_mappoint"].shape[1])):
        p = int(m["kf_mappoint"][k, i])
        if not ok(p, M) or m["mp_bad"][p]:
            continue
        if min_obs > 0:
            if m["mp_nobs"][p] >= min_obs:
                c += 1
        else:
            c += 1
    return c


def end_frame(fr, m, th_depth, reference_kf, min_obs):
    F, cap = fr["frame_mappoint"].shape
    M = len(m["mp_nobs"])
    nobs = np.full((F, cap), -1, np.int32)
    counts = np.zeros((F, 3), np.int32)
    for f in range(F):
        n = n_of(fr, f)
        for i in range(n):   # :1259-1264
            p = int(fr["frame_mappoint"][f, i])
            nobs[f, i] = m["mp_nobs"][p] if ok(p, M) and not fr["frame_outlier"][f, i] else -1
        for i in range(n):   # :1273-1281
            p = int(fr["frame_mappoint"][f, i])
            if ok(p, M) and m["mp_nobs"][p] < 1:
                fr["frame_outlier"][f, i] = 0
                fr["frame_mappoint"][f, i] = -1
        if fr.get("kp_depth") is not None:
            for i in range(n):   # :502-510
                z = f32(fr["kp_depth"][f, i])
                if z > f32(0) and z < f32(th_depth):
                    tracked = ok(fr["frame_mappoint"][f, i], M) and not fr["frame_outlier"][f, i]
                    counts[f, 0 if tracked else 1] += 1
        counts[f, 2] = tracked_map_points(m, int(reference_kf[f]), int(min_obs[f]))
    return nobs, counts


# ---- 6
def drop_outliers(fr):
    for f in range(len(fr["frame_n"])):
        for i in range(n_of(fr, f)):
            if fr["frame_outlier"][f, i]:
                fr["frame_mappoint"][f, i] = -1


# ---- 7
def stereo_points(fr, m, mode, th_depth):
    F, cap = fr["frame_mappoint"].shape
    M = len(m["mp_nobs"])
    o = dict(created_kp=np.zeros((F, cap), np.int32), created_xw=np.zeros((F, cap, 3), f32), n_created=np.zeros(F, np.int32),
             n_processed=np.zeros(F, np.int32))
    th = f32(th_depth)
    for f in range(F):
        pairs = []
        for i in range(n_of(fr, f)):
            Z = f32(fr["kp_depth"][f, i])
            if Z > f32(0):
                pairs.append((Z, i))
        if mode != INIT:
            pairs.sort(key=lambda zi: (float(zi[0]), zi[1]))   # std::sort of distinct pairs
        npoints = 0
        for Z, i in pairs:
            p = int(fr["frame_mappoint"][f, i])
            create = False
            if mode == INIT or not ok(p, M):
                create = True
            elif m["mp_nobs"][p] < 1:
                create = True
                if mode == KEYFRAME:
                    fr["frame_mappoint"][f, i] = -1
            if create:
                j = o["n_created"][f]
                o["created_kp"][f, j] = i
                o["created_xw"][f, j] = unproject(fr["pose"][f], fr["camera"][f], fr["kp_xy"][f, i, 0], fr["kp_xy"][f, i, 1], Z,
                                                  vo=mode == VO)
                o["n_created"][f] += 1
            npoints += 1
            if mode != INIT and Z > th and npoints > CLOSEST:
                break
        o["n_processed"][f] = npoints
    return o
