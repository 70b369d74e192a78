"""ORBmatcher::Fuse (src/ORBmatcher.cc:868-980 and :982-1088) on the device against tests/fuse_ref.py
(pinned by tests/test_fuse_ref.py): best_idx, best_dist and n_fused exactly equal through the device and
the host entries, for the LocalMapping (th 3) and LoopClosing (th 4) calls, with and without the chi2
gates.  The item sizes put fewer candidates than lanes in a 16-lane group, an item below one 256-thread
block and an empty item on either side in every batch."""
import numpy as np
import pytest

import fuse_ref
from orb_slam2_refactored_amd._lib import OrbError
from orb_slam2_refactored_amd.matcher import Fuse, fuse_device
from orb_slam2_refactored_amd.synth import make_fuse_batch
from test_fuse_ref import GPU_N_KP, GPU_N_MP, gpu_batch

pytestmark = pytest.mark.gpu



def to_device(b):
    import torch
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda()
                if isinstance(v, np.ndarray) and k not in ("scale_factors", "inv_sigma2") else v) for k, v in b.items()}


def _device(b, **out):
    import torch
    bi, bd, nf = fuse_device(to_device(b), **out)
    torch.cuda.synchronize()
    M, F = int(b["mp_begin"][-1]), len(b["mp_begin"]) - 1
    return bi.cpu().numpy()[:M], bd.cpu().numpy()[:M], nf.cpu().numpy()[:F]


@pytest.mark.parametrize("th", [3.0, 4.0])
@pytest.mark.parametrize("chi2", [True, False])
def test_fuse_vs_reference(th, chi2):
    b = gpu_batch(th, chi2)
    ei, ed, en = fuse_ref.fuse(b)
    assert en[:4].min() > 0
    gi, gd, gn = _device(b)
    assert np.array_equal(gi, ei)
    assert np.array_equal(gd, ed)
    assert np.array_equal(gn, en)
    hi, hd, hn = Fuse(b)
    assert np.array_equal(hi, ei) and np.array_equal(hd, ed) and np.array_equal(hn, en)


def test_fuse_repeatable():
    b = make_fuse_batch(31, n_items=6, n_kp=GPU_N_KP, n_mp=GPU_N_MP, th=3.0, chi2_gate=True)
    first, second = _device(b), _device(b)
    for x, y in zip(first, second):
        assert np.array_equal(x, y)


def test_fuse_over_limit_item():
    import torch
    b = make_fuse_batch(88, n_items=2, n_kp=[9000, 500], n_mp=[100, 100], th=3.0, chi2_gate=True)
    sent = lambda n: torch.full((n,), 12345, dtype=torch.int32, device="cuda")   # noqa: E731
    gi, gd, gn = _device(b, best_idx=sent(200), best_dist=sent(200), n_fused=sent(2))
    assert gn[0] == -1 and (gi[:100] == -1).all() and (gd[:100] == 256).all()
    with pytest.raises(OrbError, match="ORBM_PROJ_MAX_KP"):   # the host entry refuses the batch, as the others do
        Fuse(b)
    # the item within the limit is unaffected
    ei, ed, en = fuse_ref.fuse(dict(b, kp_begin=np.array([0, 500], np.int32), mp_begin=np.array([0, 100], np.int32),
                               **{k: b[k][9000:] for k in ("kp_xy", "kp_octave", "kp_uright", "kp_desc")},
                               **{k: b[k][100:] for k in ("mp_valid", "mp_xw", "mp_max_min", "mp_normal", "mp_desc")},
                               **{k: b[k][1:] for k in ("bounds", "pose", "camera")}))
    assert np.array_equal(gi[100:], ei) and np.array_equal(gd[100:], ed) and gn[1] == en[0]


def test_fuse_boundary_cases():
    """The hand-built boundary cases of tests/test_fuse_ref.py (z = 0, u = maxx, dot = 0.5 dist, the chi2
    thresholds, uright = 0, the scan-order tie), on the device."""
    from test_fuse_ref import CENTRE, Z, kat
    f32 = np.float32
    near = lambda x, to: float(np.nextafter(f32(x), f32(to)))   # noqa: E731
    mono, stereo = [(319, 240, 0, -1, 0)], [(319, 240, 0, 310, 0)]
    tie = ((5.0 * 4.0 / 512.0, 0.0, 4.0), Z, float(np.sqrt(16 + (20.0 / 512) ** 2)))
    edge = [((1.0, 0.0, 0.0), Z, 4.0), ((0.0, 0.0, -0.0), Z, 4.0), ((0.0, 0.0, -2.0 ** -20), Z, 4.0),
            ((-0.625, 0.0, 1.0), (-0.625, 0.0, 1.0), 1.0), ((0.625, 0.0, 1.0), (0.625, 0.0, 1.0), 1.0),
            ((0.0, 0.0, 4.0), (0.8, 0.0, 0.5), 4.0), ((0.0, 0.0, 4.0), (0.8, 0.0, near(0.5, 0)), 4.0)]
    cases = [kat(edge, [(320, 240, 0, -1, 0), (1, 240, 0, -1, 0), (638, 240, 0, -1, 0)]),
             kat([CENTRE], mono, inv_sigma2=[5.99] * 8), kat([CENTRE], mono, inv_sigma2=[near(5.99, np.inf)] * 8),
             kat([CENTRE], stereo, inv_sigma2=[7.8] * 8), kat([CENTRE], stereo, inv_sigma2=[near(7.8, 0)] * 8),
             kat([CENTRE], mono, inv_sigma2=[100.0] * 8, chi2=False),
             kat([CENTRE], [(320, 240, 0, 0.0, 0)]), kat([tie], [(326, 240, 0, -1, 0), (324, 240, 0, -1, 0)]),
             kat([CENTRE], [(320, 240, 1, -1, 0), (321, 240, 0, -1, 0x0F)])]
    for i, b in enumerate(cases):
        exp = fuse_ref.fuse(b)
        for got in (_device(b), Fuse(b)):
            for g, e in zip(got, exp):
                assert np.array_equal(g, e), i
