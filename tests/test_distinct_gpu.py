"""MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:285-319) on the device against tests/sim3_ref.py
(pinned by tests/test_sim3_ref.py): best and best_median exactly equal through the device and the host
entries.  The row counts sit on both sides of every size at which the kernels change (16 / 17: the 16-lane
group and the wavefront; 64 / 65: the wavefront and the workgroup; 1024 / 1025: the cap)."""
import numpy as np
import pytest

import sim3_ref
from orb_slam2_refactored_amd._lib import OrbError
from orb_slam2_refactored_amd.matcher import ComputeDistinctiveDescriptors, compute_distinctive_descriptors_device
from orb_slam2_refactored_amd.synth import make_observation_sets
from test_sim3_ref import distinct_cases, gpu_observation_sets

pytestmark = pytest.mark.gpu
SENT = 0xA5


def _device(desc, begin, stream=None):
    """Sentinel-filled outputs through the device entry."""
    import torch
    P = len(begin) - 1
    d = torch.from_numpy(np.ascontiguousarray(desc)).cuda()
    out = torch.full((max(P, 1), 32), SENT, dtype=torch.uint8, device="cuda")
    best = torch.full((max(P, 1),), 12345, dtype=torch.int32, device="cuda")
    med = torch.full((max(P, 1),), 12345, dtype=torch.int32, device="cuda")
    compute_distinctive_descriptors_device(d, torch.from_numpy(begin).cuda(), best, med, out, stream=stream)
    torch.cuda.synchronize()
    return best.cpu().numpy()[:P], med.cpu().numpy()[:P], out.cpu().numpy()[:P]


def _check_rows(desc, begin, best, out):
    for p, bi in enumerate(best):
        want = desc[begin[p] + bi] if bi >= 0 else np.full(32, SENT, np.uint8)   # an unwritten row keeps the sentinel
        assert np.array_equal(out[p], want), p


def test_distinctive_descriptors_vs_reference():
    o = gpu_observation_sets()
    desc, begin = o["desc"], o["begin"]
    eb, em = sim3_ref.distinctive_descriptors(desc, begin)
    gb, gm, go = _device(desc, begin)
    assert np.array_equal(gb, eb) and np.array_equal(gm, em)
    _check_rows(desc, begin, eb, go)
    assert eb[0] == -1 and (go[0] == SENT).all()
    hb, hm, ho = ComputeDistinctiveDescriptors(desc, begin, out_desc=np.full((len(eb), 32), SENT, np.uint8))
    assert np.array_equal(hb, eb) and np.array_equal(hm, em)
    _check_rows(desc, begin, eb, ho)


def test_distinctive_descriptors_by_hand():
    for i, (desc, begin, best, med) in enumerate(distinct_cases()):
        gb, gm, go = _device(desc, begin)
        assert gb.tolist() == best and gm.tolist() == med, i
        _check_rows(desc, begin, best, go)
        hb, hm, _ = ComputeDistinctiveDescriptors(desc, begin)
        assert hb.tolist() == best and hm.tolist() == med, i


def test_distinctive_descriptors_many_small_points():
    """More points than one workgroup of any of the three kernels holds, with empty ones among them."""
    import torch
    rng = np.random.default_rng(3)
    o = make_observation_sets(9, 300, rng.integers(0, 20, 300))
    eb, em = sim3_ref.distinctive_descriptors(o["desc"], o["begin"])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        gb, gm, go = _device(o["desc"], o["begin"], stream=st)
    assert np.array_equal(gb, eb) and np.array_equal(gm, em)
    _check_rows(o["desc"], o["begin"], eb, go)


def test_distinctive_descriptors_over_limit_point():
    o = make_observation_sets(11, 3, [5, 1025, 20])
    eb, em = sim3_ref.distinctive_descriptors(o["desc"], o["begin"])
    gb, gm, go = _device(o["desc"], o["begin"])
    assert gb[1] == -1 and (go[1] == SENT).all()
    assert gb[0] == eb[0] and gb[2] == eb[2] and gm[0] == em[0] and gm[2] == em[2]
    _check_rows(o["desc"], o["begin"], [eb[0], -1, eb[2]], go)
    with pytest.raises(OrbError, match="ORBM_DISTINCT_MAX_OBS"):
        ComputeDistinctiveDescriptors(o["desc"], o["begin"])
