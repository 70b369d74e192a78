"""ComputeStereoMatches on the GPU against the oracle on the branch-targeted scenes of tests/stereo_cases.py (what each scene
reaches is asserted on CPU, tests/test_stereo_ref.py): the host entry on every scene, the C entry with strided levels, the
batch entry with unequal counts and decoys behind them, and the argument checks.  uright and depth as int32 bit patterns."""
import ctypes as C

import numpy as np
import pytest

import stereo_cases as SC
from orb_slam2_refactored_amd import ComputeStereoMatches, ORBextractor, synth_image
from orb_slam2_refactored_amd._lib import KP_DTYPE, OrbError, StereoView, check, lib, ptr
from orb_slam2_refactored_amd.matcher import stereo_matches_batch_device

pytestmark = pytest.mark.gpu
SCENES = SC.all_scenes()
# stereo_filter_kernel: 2 static ints + cap ints of dynamic LDS within 48 KiB (csrc/orbs.hip, ST_MAX_CAP)
MAX_CAP = (48 * 1024 - 8) // 4


def same_bits(got, exp):
    return np.array_equal(got.view(np.int32), exp.view(np.int32))


@pytest.mark.parametrize("case,scene", SCENES, ids=[s.name for _, s in SCENES])
def test_host_entry_bit_exact_on_every_scene(oracle, case, scene):
    eu, ed = oracle.compute_stereo_matches(*scene.args())
    gu, gd = ComputeStereoMatches(*scene.args())
    assert same_bits(gu, eu), (gu, eu)
    assert same_bits(gd, ed), (gd, ed)


def _strided_view(kps, desc, levels, pad, fill):
    """StereoView over levels that are column slices of wider arrays (level_step > level_cols), what is outside the slice
    filled with `fill`."""
    wide = [np.full((im.shape[0], im.shape[1] + pad + 5), fill, np.uint8) for im in levels]
    views = []
    for w, im in zip(wide, levels):
        w[:, pad:pad + im.shape[1]] = im
        views.append(w[:, pad:pad + im.shape[1]])
    ptrs = (C.c_void_p * len(views))(*[v.ctypes.data for v in views])
    rows = np.array([v.shape[0] for v in views], np.int32)
    cols = np.array([v.shape[1] for v in views], np.int32)
    step = np.array([v.strides[0] for v in views], np.int32)
    assert np.all(step > cols)
    sv = StereoView(len(kps), kps.ctypes.data, desc.ctypes.data, len(views), C.cast(ptrs, C.c_void_p), rows.ctypes.data,
                    cols.ctypes.data, step.ctypes.data)
    return sv, views, (wide, ptrs, rows, cols, step)


@pytest.mark.parametrize("case", ["border", "dx_and_parabola"])
def test_c_entry_with_level_step_above_level_cols(oracle, case):
    s = SC.all_cases()[case][0]
    vl, levels_l, keep_l = _strided_view(s.kl, s.dl, s.pl, 3, 255)
    vr, levels_r, keep_r = _strided_view(s.kr, s.dr, s.pr, 7, 0)
    gu, gd = np.full(len(s.kl), -2, np.float32), np.full(len(s.kl), -2, np.float32)
    check(lib().orbm_compute_stereo_matches(C.byref(vl), C.byref(vr), ptr(SC.SCALE), ptr(SC.INV_SCALE), C.c_float(s.bf),
                                            C.c_float(s.baseline), ptr(gu), ptr(gd)), "orbm_compute_stereo_matches")
    eu, ed = oracle.compute_stereo_matches(s.kl, s.dl, levels_l, s.kr, s.dr, levels_r, SC.SCALE, SC.INV_SCALE, s.bf, s.baseline)
    assert (ed > 0).sum() >= 3
    assert same_bits(gu, eu) and same_bits(gd, ed)


def test_rows_above_the_row_table_are_refused():
    s = SC.Scene("rows_4097", 0, 4097, 64)
    i, _ = s.pair(50, 8.25, 30)
    s.finish()
    with pytest.raises(OrbError, match="rows must be 1..4096"):
        ComputeStereoMatches(*s.args())


def test_cap_limit_is_an_argument_error_before_any_launch(oracle):
    """More keypoints than stereo_filter_kernel's LDS holds: refused by launch_stereo's argument check (no launch issued);
    exactly the limit runs."""
    s = SC.all_cases()["disparity"][0]
    for n, side in ((MAX_CAP + 1, "left"), (MAX_CAP + 1, "right")):
        k = np.zeros(n, KP_DTYPE)
        k["x"], k["y"] = 60, 30.5                           # a row nobody lists; the other side stays as it is
        d = np.zeros((n, 32), np.uint8)
        a = (k, d, s.pl, s.kr, s.dr, s.pr) if side == "left" else (s.kl, s.dl, s.pl, k, 255 - d, s.pr)
        with pytest.raises(OrbError, match="more than 12286 keypoints per frame"):
            ComputeStereoMatches(*a, SC.SCALE, SC.INV_SCALE, s.bf, s.baseline)
    # at the limit: the scene's keypoints first, the rest on a row without candidates
    k = np.zeros(MAX_CAP, KP_DTYPE)
    k["x"], k["y"] = 60, 30.5
    d = np.zeros((MAX_CAP, 32), np.uint8)
    k[:len(s.kl)], d[:len(s.kl)] = s.kl, s.dl
    a = (k, d, s.pl, s.kr, s.dr, s.pr, SC.SCALE, SC.INV_SCALE, s.bf, s.baseline)
    eu, ed = oracle.compute_stereo_matches(*a)
    gu, gd = ComputeStereoMatches(*a)
    assert (ed > 0).sum() == 3 and same_bits(gu, eu) and same_bits(gd, ed)


F_B, K_B, SHIFT_B = 3, 24, 20


def batch_data(oracle, cap):
    """F = 3 frame pairs of 640 x 480, the right image the left one moved 20 columns (at level 0) plus noise; keypoints and
    descriptors hand-made, octave 0, `cap` slots a frame.  K real pairs (right x = uL - 20 + 2: the minimum at dx = -2,
    descriptor distance 10).  Left slots cycle through the real left keypoints.  Right slots K and up are decoys: copies
    of the even pairs' right keypoints 4 columns further (the true position leaves the search range) with distance 2, so a
    decoy read from behind a count beats the real keypoint and changes the result."""
    F, K, S = F_B, K_B, SHIFT_B
    Ls = np.stack([synth_image(40 + f, 640, 480) for f in range(F)])
    rng = np.random.default_rng(9)
    Rs = np.concatenate([Ls[:, :, S:], np.repeat(Ls[:, :, -1:], S, axis=2)], axis=2)
    # one grey level of noise: SADs above 0, or the median is 0 and the filter drops every match
    Rs = np.clip(Rs.astype(np.int16) + rng.integers(0, 2, Rs.shape), 0, 255).astype(np.uint8)
    kl, kr = np.zeros((F, cap), KP_DTYPE), np.zeros((F, cap), KP_DTYPE)
    dl, dr = np.zeros((F, cap, 32), np.uint8), np.zeros((F, cap, 32), np.uint8)
    for f in range(F):
        base = rng.integers(0, 256, (K, 32), dtype=np.uint8)
        for i in range(cap):
            q = i % K
            kl[f, i] = (100 + 60 * (q % 8), 100 + 120 * (q // 8), 31, 0, 1, 0, -1)
            dl[f, i] = base[q]
            if i >= K:
                q = 2 * (i % (K // 2))
            kr[f, i] = (100 + 60 * (q % 8) - S + (2 if i < K else 6), 100 + 120 * (q // 8), 31, 0, 1, 0, -1)
            dr[f, i] = SC.flip(base[q], 10 if i < K else 2, 0 if i < K else 50)
    p = oracle.params(500)
    t = oracle.scale_tables(p)
    pyr = [(oracle.pyramid(p, Ls[f]), oracle.pyramid(p, Rs[f])) for f in range(F)]

    def expect(f, nl, nr):
        return oracle.compute_stereo_matches(kl[f, :nl], dl[f, :nl], pyr[f][0], kr[f, :nr], dr[f, :nr], pyr[f][1], t["scale"],
                                             t["inv_scale"], SC.BF, SC.BASELINE)
    return dict(Ls=Ls, Rs=Rs, kl=kl, kr=kr, dl=dl, dr=dr, expect=expect)


@pytest.fixture(scope="module")
def batch(oracle):
    """batch_data on the device: both image stacks extracted for their pyramids, then the hand-made keypoint, descriptor
    and count tensors in place of the extractors' own."""
    import torch
    tl, tr = (torch.from_numpy(batch_data(oracle, 1)[k]).cuda() for k in ("Ls", "Rs"))
    exl, exr = ORBextractor(ORBextractor.Parameters(500)), ORBextractor(ORBextractor.Parameters(500))
    outl, outr = exl.extract_batch_device(tl), exr.extract_batch_device(tr)
    torch.cuda.synchronize()
    cap = outl[0].shape[1]
    assert cap > 2 * K_B
    b = batch_data(oracle, cap)

    def run(cl, cr):
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(F_B, cap, -1)).cuda()
        ol = (dev(b["kl"], np.int32), dev(b["dl"], np.uint8), torch.tensor(cl, dtype=torch.int32).cuda())
        orr = (dev(b["kr"], np.int32), dev(b["dr"], np.uint8), torch.tensor(cr, dtype=torch.int32).cuda())
        out = (torch.full((F_B, cap), -7, dtype=torch.float32).cuda(), torch.full((F_B, cap), -7, dtype=torch.float32).cuda())
        stereo_matches_batch_device(exl, exr, ol, orr, SC.BF, SC.BASELINE, out=out)
        torch.cuda.synchronize()
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return dict(F=F_B, K=K_B, cap=cap, run=run, expect=b["expect"], keep=(tl, tr, outl, outr))


def _batch_check(b, cl, cr):
    gu, gd = b["run"](cl, cr)
    for f in range(b["F"]):
        eu, ed = b["expect"](f, cl[f], cr[f])
        assert same_bits(gu[f, :cl[f]], eu), f      # slots past the left count are not compared
        assert same_bits(gd[f, :cl[f]], ed), f


def test_batch_entry_counts_zero_k_cap(batch):
    K, cap = batch["K"], batch["cap"]
    # the decoys matter: with them in reach the K real pairs come out differently
    eu, ed = batch["expect"](1, K, 0)
    assert np.all(eu == -1) and np.all(ed == -1)
    assert not same_bits(batch["expect"](1, K, K)[0], batch["expect"](1, K, cap)[0])
    assert (batch["expect"](2, cap, cap)[1] > 0).sum() >= K // 4
    _batch_check(batch, [0, K, cap], [K, 0, cap])


def test_batch_entry_counts_below_cap_on_both_sides(batch):
    K, cap = batch["K"], batch["cap"]
    assert (batch["expect"](0, K, K)[1] > 0).sum() >= K // 2
    _batch_check(batch, [K, K // 2, 1], [K, cap, K // 2])
