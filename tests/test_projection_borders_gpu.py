"""The window clamp of FeaturesGrid::GetFeaturesInArea (Frame.cc:109-119) in each of the seven projection
searches: points projected 2 px inside each of the four image bounds, with a search radius larger than
that, so every window is clipped by its border, and one keypoint with the point's descriptor a few pixels
further in.  Batches of 3 frames (one without keypoints, one without points, the border frame; at most
200 keypoints and 100 points per frame) for the searches that take projections directly; one hand-built
keyframe (identity pose, 640 x 480) for those that project on the device.  Expected values from the
oracle and the Python restatements; every border point has to find its keypoint, through the device and
the host entry alike."""
import numpy as np
import pytest

import fuse_ref
import sim3_ref
from orb_slam2_refactored_amd import matcher as M
from orb_slam2_refactored_amd.synth import make_init_batch, make_proj_batch, make_reloc_batch
from test_fuse_ref import kat as fuse_kat
from test_sim3_ref import kat as sim3_kat, pt

pytestmark = pytest.mark.gpu

HOST_KEYS = ("scale_factors", "inv_sigma2")


def to_device(b):
    import torch
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) and k not in HOST_KEYS else v)
            for k, v in b.items()}


def on_device(fn, b, *sizes):
    import torch
    outs = fn(to_device(b))
    torch.cuda.synchronize()
    return [o.cpu().numpy()[:n] for o, n in zip(outs, sizes)]


def border_points(bd, inset=2.0, step=8.0):
    """(u, v) `inset` px inside the left, right, top and bottom bound, and the keypoint `step` px further in (far
    enough for Round() to keep it in the last cell: a keypoint within half a cell of maxx or maxy is off the grid)."""
    minx, maxx, miny, maxy = [float(v) for v in bd]
    cx, cy = 0.5 * (minx + maxx), 0.5 * (miny + maxy)
    pts = np.array([(minx + inset, cy), (maxx - inset, cy), (cx, miny + inset), (cx, maxy - inset)], np.float32)
    kps = np.array([(minx + inset + step, cy), (maxx - inset - step, cy), (cx, miny + inset + step), (cx, maxy - inset - step)], np.float32)
    return pts, kps


def proj_batch(th):
    """make_proj_batch with frame 2's first four keypoints and map points moved to the borders."""
    b = make_proj_batch(61, n_frames=3, n_kp=[0, 150, 200], n_mp=[60, 0, 100], th=th)
    k0, m0 = int(b["kp_begin"][2]), int(b["mp_begin"][2])
    pts, kps = border_points(b["bounds"][2])
    for i in range(4):
        b["kp_xy"][k0 + i] = kps[i]
        b["kp_octave"][k0 + i] = 0
        b["kp_uright"][k0 + i] = -1.0
        b["kp_claimed"][k0 + i] = 0
        b["kp_desc"][k0 + i] = 17 * (i + 1)
        b["mp_proj"][m0 + i] = (pts[i, 0], pts[i, 1], pts[i, 0] - 10)
        b["mp_level"][m0 + i] = 0
        b["mp_view_cos"][m0 + i] = 0.5   # radius 4 th
        b["mp_valid"][m0 + i] = 1
        b["mp_has_obs"][m0 + i] = 1
        b["mp_desc"][m0 + i] = 17 * (i + 1)
    return b, k0, m0


def test_search_by_projection_borders(oracle):
    b, k0, _ = proj_batch(th=5.0)   # radius 20 px
    exp, en = oracle.search_by_projection(b)
    assert list(exp[k0:k0 + 4]) == [0, 1, 2, 3] and en[0] == 0 and en[1] == 0
    K, F = int(b["kp_begin"][-1]), 3
    for got in (on_device(M.search_by_projection_device, b, K, F), M.SearchByProjection(b)):
        assert np.array_equal(got[0], exp) and np.array_equal(got[1], en)


def test_motion_projection_borders(oracle):
    b, k0, _ = proj_batch(th=15.0)   # radius 15 px at octave 0
    K, Mp = int(b["kp_begin"][-1]), int(b["mp_begin"][-1])
    rng = np.random.default_rng(3)
    m = dict(kp_begin=b["kp_begin"], kp_xy=b["kp_xy"], kp_octave=b["kp_octave"], kp_uright=b["kp_uright"],
             kp_desc=b["kp_desc"], kp_angle=rng.uniform(0, 360, K).astype(np.float32), kp_claimed=b["kp_claimed"],
             bounds=b["bounds"], mp_begin=b["mp_begin"], mp_valid=b["mp_valid"], mp_proj=b["mp_proj"],
             mp_octave=np.minimum(b["mp_level"], 7).astype(np.int32), mp_desc=b["mp_desc"], mp_has_obs=b["mp_has_obs"],
             mp_angle=rng.uniform(0, 360, Mp).astype(np.float32), motion=None, scale_factors=b["scale_factors"], th=15.0,
             check_orientation=False)
    exp, en = oracle.search_by_projection_motion(m)
    assert list(exp[k0:k0 + 4]) == [0, 1, 2, 3] and en[0] == 0 and en[1] == 0
    km, nm = on_device(M.search_by_projection_motion_device, m, K, 3)
    assert np.array_equal(km, exp) and np.array_equal(nm, en)


def test_init_borders(oracle):
    b = make_init_batch(62, n_pairs=3, n1=[60, 0, 100], n2=[0, 150, 200])
    b["window"], b["check_orientation"] = 20, False
    k0, q0 = int(b["kp_begin"][2]), int(b["q_begin"][2])
    pts, kps = border_points(b["bounds"][2], step=12.0)
    for i in range(4):
        b["kp_xy"][k0 + i] = kps[i]
        b["kp_octave"][k0 + i] = 0
        b["kp_desc"][k0 + i] = 17 * (i + 1)
        b["prev_matched"][q0 + i] = pts[i]
        b["q_octave"][q0 + i] = 0
        b["q_desc"][q0 + i] = 17 * (i + 1)
    exp, en, eprev = oracle.search_for_initialization(b)   # (b is not modified)
    assert list(exp[q0:q0 + 4]) == [0, 1, 2, 3] and en[0] == 0 and en[1] == 0
    Q = int(b["q_begin"][-1])
    d = dict(b, prev_matched=b["prev_matched"].copy())
    m12, n = on_device(M.search_for_initialization_device, d, Q, 3)
    assert np.array_equal(m12, exp) and np.array_equal(n, en)
    h = dict(b, prev_matched=b["prev_matched"].copy())
    hm, hn = M.SearchForInitialization(h)[:2]
    assert np.array_equal(hm, exp) and np.array_equal(hn, en)
    assert np.array_equal(h["prev_matched"], eprev)   # updated in place through the uploaded copy


# ---- the searches that project on the device: identity pose, fx = fy = 512, centre (320, 240), z = 1
BORDER_X = [(-0.625 + 2 / 512, 0.0, 1.0), (0.625 - 2 / 512, 0.0, 1.0), (0.0, -0.46875 + 2 / 512, 1.0), (0.0, 0.46875 - 2 / 512, 1.0)]
BORDER_KP = [(6, 240), (634, 240), (320, 6), (320, 474)]   # 4 px from (2, 240), (638, 240), (320, 2), (320, 478)


def test_fuse_and_sim3_projection_borders():
    # maxDistance_ = 1 < dist3D < 1.2: scale 0, radius th = 6; the normal along the ray
    b = fuse_kat([(X, X, 1.0) for X in BORDER_X], [(x, y, 0, -1, 0) for x, y in BORDER_KP], th=6.0, chi2=False)
    ei, ed, en = fuse_ref.fuse(b)
    assert list(ei) == [0, 1, 2, 3] and en[0] == 4
    for got in (on_device(M.fuse_device, b, 4, 4, 1), M.Fuse(b)):
        assert np.array_equal(got[0], ei) and np.array_equal(got[1], ed) and np.array_equal(got[2], en)
    b["kp_claimed"] = None
    em, en = fuse_ref.search_by_projection_sim3(b)
    assert list(em) == [0, 1, 2, 3] and en[0] == 4
    for got in (on_device(M.search_by_projection_sim3_device, b, 4, 1), M.SearchByProjectionSim3(b)):
        assert np.array_equal(got[0], em) and np.array_equal(got[1], en)


def test_search_by_sim3_borders():
    # keyframe 1 holds the four border points (its own keypoints far away), keyframe 2 the keypoints
    b = sim3_kat([(pt(X, 1.0), (320, 240, 0, 0xFF)) for X in BORDER_X], [(None, (x, y, 0, 0)) for x, y in BORDER_KP])
    exp = sim3_ref.search_by_sim3(b)
    assert list(exp[1]) == [0, 1, 2, 3]   # match1: each point found its keypoint through a clipped window
    for got in (on_device(M.search_by_sim3_device, b, 4, 4, 4, 1), M.SearchBySim3(b)):
        for g, e in zip(got, exp):
            assert np.array_equal(g, e)


def test_reloc_borders(oracle):
    b = make_reloc_batch(63, n_frames=3, n_kp=[0, 150, 200], n_mp=[60, 0, 100], th=10.0, check_orientation=False)
    k0, m0 = int(b["kp_begin"][2]), int(b["mp_begin"][2])
    P, C, bd = b["pose"][2].astype(np.float64), b["camera"][2].astype(np.float64), b["bounds"][2]
    R, t = P[:9].reshape(3, 3), P[9:]
    pts, kps = border_points(bd)
    z = 8.0
    for i in range(4):
        Xc = np.array([(pts[i, 0] - C[2]) / C[0] * z, (pts[i, 1] - C[3]) / C[1] * z, z])
        Xw = R.T @ (Xc - t)
        dist = float(np.linalg.norm(Xw + R.T @ t))
        b["mp_xw"][m0 + i] = Xw
        b["mp_max_min"][m0 + i] = (dist, dist / 3.0)   # predicted scale 0 or 1: radius 10 or 12 px
        b["mp_valid"][m0 + i] = 1
        b["mp_desc"][m0 + i] = 17 * (i + 1)
        b["kp_xy"][k0 + i] = kps[i]
        b["kp_octave"][k0 + i] = 0
        b["kp_claimed"][k0 + i] = 0
        b["kp_desc"][k0 + i] = 17 * (i + 1)
    exp, en = oracle.search_by_projection_reloc(b)
    assert list(exp[k0:k0 + 4]) == [0, 1, 2, 3] and en[0] == 0 and en[1] == 0
    K = int(b["kp_begin"][-1])
    for got in (on_device(M.search_by_projection_reloc_device, b, K, 3), M.SearchByProjectionReloc(b)):
        assert np.array_equal(got[0], exp) and np.array_equal(got[1], en)
