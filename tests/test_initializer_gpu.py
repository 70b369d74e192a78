"""Initializer::Initialize (src/Initializer.cc:45-122) on the device against tests/initializer_ref.py (pinned by
tests/test_initializer_ref.py).  One batch: 12 pairs with N in {0, 7, 8, 9, 63, 64, 65, 100, 128, 129, 150, 300}
matches among 1.3 N + 5 keypoints per frame, 0.3 px noise, 10-30 % gross outliers, scenes alternating plane, general
and pure rotation, plus a pair with 8193 keypoints in frame 1; max_iterations 1, 64, 65 and 200.  Identical: found,
model, best_h / best_f (where several hypotheses drew the same eight correspondences in another order they are one
model and tie up to rounding: the winner must then be of the same set), the masks, triangulated and the sorted
n_good.  Within the margins test_initializer_ref.py measures: every hyp_score, score_h / score_f, r21t21, p3d."""
import numpy as np
import pytest

import initializer_ref as R
from orb_slam2_refactored_amd.initializer import InitializerInitialize, initializer_initialize_device
from test_initializer_ref import GPU_N, gpu_batch, gpu_reference, margins

pytestmark = pytest.mark.gpu

_HOST = ("gt_r21t21",)
_FIELDS = ("found", "model", "r21t21", "p3d", "triangulated", "score_h", "score_f", "best_h", "best_f", "h21", "f21",
           "inlier_h", "inlier_f", "hyp_score", "n_good", "parallax")
_SLOTS = ("p3d", "triangulated", "inlier_h", "inlier_f")


def to_device(b):
    import torch
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) and k not in _HOST else v)
            for k, v in b.items()}


def _device(b, stream=None):
    import torch
    o = initializer_initialize_device(to_device(b), stream=stream)
    torch.cuda.synchronize()
    K1, F = int(b["kp1_begin"][-1]), len(b["kp1_begin"]) - 1
    return {k: o[k].cpu().numpy()[:K1 if k in _SLOTS else F] for k in _FIELDS}


def _same(a, c, what):
    for k in _FIELDS:
        assert a[k].tobytes() == c[k].tobytes(), (what, k)


def _check(b, got, exp, m, what):
    used = 0
    for p in range(len(GPU_N)):
        k0, k1 = int(b["kp1_begin"][p]), int(b["kp1_begin"][p + 1])
        for k in ("found", "model"):
            assert got[k][p] == exp[k][p], (what, p, k, got[k][p], exp[k][p])
        for mdl, k in enumerate(("best_h", "best_f")):
            if exp[k][p] < 0:
                assert got[k][p] == -1, (what, p, k)
            else:
                assert got[k][p] >= 0 and exp["set_id"][p][got[k][p]] == exp["set_id"][p][exp[k][p]], (what, p, k, got[k][p], exp[k][p])
        for k in ("inlier_h", "inlier_f", "triangulated"):
            assert np.array_equal(got[k][k0:k1], exp[k][k0:k1]), (what, p, k)
        assert sorted(got["n_good"][p].tolist()) == sorted(exp["n_good"][p].tolist()), (what, p, got["n_good"][p], exp["n_good"][p])
        g, e = got["hyp_score"][p].astype(np.float64), exp["hyp_score"][p].astype(np.float64)
        fin = np.isfinite(e)
        assert np.array_equal(np.isfinite(g), fin), (what, p, "finite scores")
        d = np.abs(g - e)[fin]
        used += int((d > 0).sum())
        print(what, "pair", p, "scores that differ from the restatement's:", int((d > 0).sum()), "of", int(fin.sum()),
              "largest / margin", float((d / m["score"][p][fin]).max()) if fin.any() else 0.0)
        assert (d <= m["score"][p][fin]).all(), (what, p, "hyp_score outside the margin")
        for mdl, k in enumerate(("score_h", "score_f")):
            best = exp["best_h" if mdl == 0 else "best_f"][p]
            tol = m["score"][p, mdl, best] if best >= 0 else 0.0
            assert abs(float(got[k][p]) - float(exp[k][p])) <= tol, (what, p, k)
        if exp["found"][p] == 1:
            dr = R.pose_distance(exp["r21t21"][p], got["r21t21"][p])
            tri = exp["triangulated"][k0:k1].astype(bool)
            dp = R.point_distance(exp["p3d"][k0:k1][tri], got["p3d"][k0:k1][tri])
            print(what, "pair", p, "pose distance (rot, t)", dr, "p3d", dp, "margins", m["rot"], m["t"], m["p3d"])
            assert dr[0] <= m["rot"] and dr[1] <= m["t"] and dp <= m["p3d"], (what, p, dr, dp)
        else:
            assert not got["r21t21"][p].any() and not got["p3d"][k0:k1].any() and not got["triangulated"][k0:k1].any(), (what, p)
    return used


@pytest.mark.parametrize("max_iterations", [1, 64, 65, 200])
def test_initialize_vs_reference(max_iterations):
    b, exp, m = gpu_batch(max_iterations), gpu_reference(max_iterations), margins(max_iterations)
    dev, host = _device(b), InitializerInitialize(b)
    _check(b, dev, exp, m, f"T={max_iterations}")
    _same(dev, host, "host entry against device entry")


def test_repeatable_and_on_a_side_stream():
    import torch
    b = gpu_batch(200)
    a = _device(b)
    _same(a, _device(b), "run to run")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = _device(b, stream=st)
    _same(a, c, "side stream")


def test_over_limit_pair():
    from orb_slam2_refactored_amd._lib import OrbError
    b = gpu_batch(200, True)
    got = _device(b)
    p = len(GPU_N)
    k0, k1 = int(b["kp1_begin"][p]), int(b["kp1_begin"][p + 1])
    assert k1 - k0 == 8193 and got["found"][p] == -1
    for k in _FIELDS:
        if k in ("best_h", "best_f"):
            assert got[k][p] == -1, k
        elif k != "found":
            assert not np.asarray(got[k][k0:k1] if k in _SLOTS else got[k][p]).any(), k
    _check(b, got, gpu_reference(200, None, True), margins(200, True), "neighbours of the oversized pair")
    with pytest.raises(OrbError, match="ORBM_PROJ_MAX_KP"):
        InitializerInitialize(b)


def test_search_for_initialization_feeds_the_initializer_on_the_device():
    """Tracking.cc:1050-1075 without a host round trip: search_for_initialization_device's matches12 tensor goes straight
    into initializer_initialize_device; equal to the chain through the two host entries."""
    import torch
    from orb_slam2_refactored_amd.initializer import make_draws
    from orb_slam2_refactored_amd.matcher import SearchForInitialization, search_for_initialization_device
    from orb_slam2_refactored_amd.synth import make_init_batch
    sb = make_init_batch(3, n_pairs=2, n1=[900, 1200], n2=[1000, 1100])
    F = 2
    # frame 1 positions: prev_matched is F1's keypointsUn on entry
    kp1_xy = sb["prev_matched"].copy()
    extra = dict(kp1_begin=sb["q_begin"], kp2_begin=sb["kp_begin"], kp1_xy=kp1_xy, kp2_xy=sb["kp_xy"],
                 camera=np.tile(np.array([700, 700, 640, 360], np.float32), (F, 1)), draws=make_draws(F, 200, 5), max_iterations=200)
    hb = dict(sb, prev_matched=sb["prev_matched"].copy())
    m12, _ = SearchForInitialization(hb)
    assert (m12 >= 0).sum() > 100
    ho = InitializerInitialize(dict(extra, matches12=m12))
    db = to_device(dict(sb, prev_matched=sb["prev_matched"].copy()))
    dm12, _ = search_for_initialization_device(db)
    do = initializer_initialize_device(dict(to_device(extra), matches12=dm12))
    torch.cuda.synchronize()
    K1 = int(sb["q_begin"][-1])
    for k in _FIELDS:
        assert do[k].cpu().numpy()[:K1 if k in _SLOTS else F].tobytes() == ho[k].tobytes(), k
    assert (ho["best_h"] >= 0).all() and (ho["best_f"] >= 0).all()
