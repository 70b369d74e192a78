"""SearchByProjection(const KeyFrame*, const Sim3& Scw, points, matched, th) (src/ORBmatcher.cc:518-612,
LoopClosing::ComputeSim3) on the device against tests/fuse_ref.py: kp_match and n_matches exactly equal
through the device and the host entries at th 10, with half the points competing for another point's
keypoint (claims made during the call decide), entry claims on 10 % of the keypoints and empty items."""
import numpy as np
import pytest

import fuse_ref
from orb_slam2_refactored_amd.matcher import SearchByProjectionSim3, search_by_projection_sim3_device
from orb_slam2_refactored_amd.synth import make_fuse_batch
from test_fuse_gpu import to_device

pytestmark = pytest.mark.gpu


def _batch(seed, **kw):
    return make_fuse_batch(seed, n_items=5, n_kp=[800, 500, 0, 300, 64], n_mp=[500, 400, 50, 0, 40], th=10.0,
                           chi2_gate=False, dup_frac=0.5, **kw)


def _check(b):
    import torch
    exp, en = fuse_ref.search_by_projection_sim3(b)
    km, nm = search_by_projection_sim3_device(to_device(b))
    torch.cuda.synchronize()
    K, F = int(b["kp_begin"][-1]), len(b["kp_begin"]) - 1
    assert np.array_equal(km.cpu().numpy()[:K], exp)
    assert np.array_equal(nm.cpu().numpy()[:F], en)
    hm, hn = SearchByProjectionSim3(b)
    assert np.array_equal(hm, exp) and np.array_equal(hn, en)
    return exp, en


def test_sim3_vs_reference():
    b = _batch(5, claimed_frac=0.1)
    exp, en = _check(b)
    assert en[0] > 20 and en[1] > 20 and en[2] == 0 and en[3] == 0
    # the claims made during the call matter: without them more than one point takes the same keypoint
    bi, _bd, _nf = fuse_ref.fuse(b)   # the same search with no claims at all
    mb = b["mp_begin"]
    taken = [bi[mb[i]:mb[i + 1]] for i in range(2)]
    assert any(len(t[t >= 0]) > len(set(t[t >= 0])) for t in taken)
    assert not b["kp_claimed"][exp >= 0].any()   # an entry claim is never matched (:588)


def test_sim3_without_entry_claims():
    b = _batch(6)
    b["kp_claimed"] = None
    _check(b)


def test_sim3_over_limit_item():
    """A keyframe above the device keypoint limit gets n_matches = -1 and kp_match = -1 on every keypoint
    (initialised, never garbage); the item within the limit is unaffected."""
    import torch
    from test_projection_gpu import one_frame
    b = make_fuse_batch(9, n_items=2, n_kp=[8193, 300], n_mp=[40, 200], th=10.0, chi2_gate=False, dup_frac=0.5,
                        claimed_frac=0.1)
    km, nm = search_by_projection_sim3_device(to_device(b), kp_match=torch.full((8493,), 12345, dtype=torch.int32,
                                                                                device="cuda"))
    torch.cuda.synchronize()
    km, nm = km.cpu().numpy(), nm.cpu().numpy()
    assert nm[0] == -1 and (km[:8193] == -1).all()
    exp, en = fuse_ref.search_by_projection_sim3(one_frame(b, 1))
    assert en[0] > 0 and nm[1] == en[0] and np.array_equal(km[8193:8493], exp)
