"""C3 end to end on the device (BASELINE.json configs[2]): stereo 1242x375 pairs are
extracted in one batch (L and R frames), then SearchForTriangulation (ORBmatcher.cc:768-866) runs as
one batched launch on the extractor's HBM slots.  Parity: the oracle's restatement on the same
keypoints / descriptors (extraction itself is compared with the oracle too), exact match12 and
match counts.  Also the DBoW2-FeatureVector mode fed by orbv_transform_batch_device, and
uright / has_mappoint / onlyStereo masks."""
import numpy as np
import pytest

from orb_slam2_refactored_amd import ORBextractor
from orb_slam2_refactored_amd.matcher import search_for_triangulation_batch_device
from orb_slam2_refactored_amd.synth import KITTI, stereo_pair, stereo_tri_geometry

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["mm", "mm_split2", "scan"])
def tri_path(request, monkeypatch):
    """Both all-pairs kernels: the matrix-core event path (default; also with kf2 cut into two column
    parts merged through match12 keys) and the per-lane segmented scan."""
    monkeypatch.setenv("ORBM_TRI_MM", "0" if request.param == "scan" else "1")
    monkeypatch.setenv("ORBM_TRI_SPLIT", "2" if request.param == "mm_split2" else "1")
    return request.param


def _oracle_pair(O, kps1, d1, n1, kps2, d2, n2, F12, ep2, scale, sigma2, ur1=None, ur2=None, mp1=None, mp2=None,
                 fv1=None, fv2=None, only_stereo=False):
    keep = O._Keep()
    k1 = kps1[:n1].view(np.float32)
    k2 = kps2[:n2].view(np.float32)

    def frame(k, kk, d, n, ur, mp, fv):
        xy = np.ascontiguousarray(kk[:, :2])
        oc = np.ascontiguousarray(k[:n, 5]).astype(np.int32)
        ur = np.full(n, -1, np.float32) if ur is None else ur[:n]
        mp = np.zeros(n, np.uint8) if mp is None else mp[:n]
        if fv is None:
            fv = (np.array([0], np.uint32), np.array([0, n], np.int32), np.arange(n, dtype=np.int32))
        return O.tri_frame(keep, xy, oc, ur, mp, d[:n], *fv)

    f1 = frame(kps1, k1, d1, n1, ur1, mp1, fv1)
    f2 = frame(kps2, k2, d2, n2, ur2, mp2, fv2)
    return O.search_for_triangulation(f1, f2, F12, ep2, scale, sigma2, only_stereo)


def _c3_batch(pairs, seed0):
    import torch
    Ls, Rs = zip(*[stereo_pair(seed0 + i)[:2] for i in range(pairs)])
    frames = torch.from_numpy(np.stack(list(Ls) + list(Rs))).cuda()
    ex = ORBextractor(ORBextractor.Parameters(2000))
    kps, desc, cnt = ex.extract_batch_device(frames)
    return ex, frames, kps, desc, cnt


def test_c3_extracted_pairs(oracle, tri_path):
    """The C3 workload as written: extract L+R, single-node FeatureVector, uright = -1, no MapPoints,
    F12 / ep2 of the rectified rig (ep2 = (-inf, NaN): the epipole gate falls as in the reference)."""
    import torch
    P = 4
    ex, frames, kps, desc, cnt = _c3_batch(P, 9100)
    F12, ep2 = stereo_tri_geometry()
    assert np.isneginf(ep2[0]) and np.isnan(ep2[1])
    Ft = torch.from_numpy(np.tile(F12, (P, 1))).cuda()
    Et = torch.from_numpy(np.tile(ep2, (P, 1))).cuda()
    f1 = torch.arange(P, dtype=torch.int32, device="cuda")
    f2 = f1 + P
    scale, sigma2 = ex.GetScaleFactors(), ex.GetScaleSigmaSquares()
    m12, nm = search_for_triangulation_batch_device(kps, desc, cnt, kps, desc, cnt, Ft, Et, scale, sigma2,
                                                    frame1=f1, frame2=f2)
    torch.cuda.synchronize()
    K, D, N = kps.cpu().numpy(), desc.cpu().numpy(), cnt.cpu().numpy()
    M, NM = m12.cpu().numpy(), nm.cpu().numpy()
    # extraction of pair 0 against the oracle (the full extractor parity lives in test_extractor_gpu)
    okp, od, _ = oracle.extract(oracle.params(2000), frames[0].cpu().numpy())
    assert len(okp) == N[0] and np.array_equal(od, D[0, :N[0]])
    total = 0
    for p in range(P):
        exp, n = _oracle_pair(oracle, K[p], D[p], N[p], K[P + p], D[P + p], N[P + p], F12, ep2, scale, sigma2)
        assert np.array_equal(M[p, :N[p]], exp), p
        assert NM[p] == n
        total += n
    assert total > 400 * P   # stereo correspondences on the same rows


def test_c3_masks_and_only_stereo(oracle, tri_path):
    """uright (stereo keypoints skip the epipole gate; onlyStereo drops mono queries / candidates)
    and has_mappoint masks on both keyframes, with a finite epipole."""
    import torch
    P = 3
    ex, frames, kps, desc, cnt = _c3_batch(P, 9200)
    cap = kps.shape[1]
    rng = np.random.default_rng(5)
    ur = np.where(rng.random((2 * P, cap)) < 0.4, rng.uniform(0, 1241, (2 * P, cap)), -1).astype(np.float32)
    mp = (rng.random((2 * P, cap)) < 0.15).astype(np.uint8)
    F12, _ = stereo_tri_geometry()
    ep2 = np.array([650.0, 190.0], np.float32)   # finite epipole inside the image
    Ft = torch.from_numpy(np.tile(F12, (P, 1))).cuda()
    Et = torch.from_numpy(np.tile(ep2, (P, 1))).cuda()
    f1 = torch.arange(P, dtype=torch.int32, device="cuda")
    scale, sigma2 = ex.GetScaleFactors(), ex.GetScaleSigmaSquares()
    K, D, N = kps.cpu().numpy(), desc.cpu().numpy(), cnt.cpu().numpy()
    for only in (False, True):
        m12, nm = search_for_triangulation_batch_device(
            kps, desc, cnt, kps, desc, cnt, Ft, Et, scale, sigma2, frame1=f1, frame2=f1 + P,
            uright1=torch.from_numpy(ur).cuda(), uright2=torch.from_numpy(ur).cuda(),
            has_mappoint1=torch.from_numpy(mp).cuda(), has_mappoint2=torch.from_numpy(mp).cuda(), only_stereo=only)
        torch.cuda.synchronize()
        M, NM = m12.cpu().numpy(), nm.cpu().numpy()
        for p in range(P):
            q = P + p
            exp, n = _oracle_pair(oracle, K[p], D[p], N[p], K[q], D[q], N[q], F12, ep2, scale, sigma2,
                                  ur1=ur[p], ur2=ur[q], mp1=mp[p], mp2=mp[q], only_stereo=only)
            assert np.array_equal(M[p, :N[p]], exp), (only, p)
            assert NM[p] == n and n > 0


def test_c3_query_block_edges(oracle, tri_path):
    """255 / 256 / 257 queries (one query block of the all-pairs kernels, exactly and one over) against
    300 / 289 / 257 candidates: the keyframes' counts cut down to the first keypoints of extracted frames."""
    import torch
    P = 3
    ex, frames, kps, desc, cnt = _c3_batch(P, 9300)
    N = cnt.cpu().numpy().copy()
    assert N.min() >= 300
    N[:P] = [255, 256, 257]
    N[P:] = [300, 289, 257]
    ct = torch.from_numpy(N).cuda()
    F12, _ = stereo_tri_geometry()
    ep2 = np.array([650.0, 190.0], np.float32)
    Ft = torch.from_numpy(np.tile(F12, (P, 1))).cuda()
    Et = torch.from_numpy(np.tile(ep2, (P, 1))).cuda()
    f1 = torch.arange(P, dtype=torch.int32, device="cuda")
    scale, sigma2 = ex.GetScaleFactors(), ex.GetScaleSigmaSquares()
    m12, nm = search_for_triangulation_batch_device(kps, desc, ct, kps, desc, ct, Ft, Et, scale, sigma2,
                                                    frame1=f1, frame2=f1 + P)
    torch.cuda.synchronize()
    K, D = kps.cpu().numpy(), desc.cpu().numpy()
    M, NM = m12.cpu().numpy(), nm.cpu().numpy()
    for p in range(P):
        q = P + p
        exp, n = _oracle_pair(oracle, K[p], D[p], N[p], K[q], D[q], N[q], F12, ep2, scale, sigma2)
        assert np.array_equal(M[p, :N[p]], exp), p
        assert NM[p] == n


def test_c3_event_overflow(oracle, tri_path):
    """Repeated descriptors: kf2 holds copies of four kf1 descriptors (and near copies), so those rows
    see a candidate with d <= TH_LOW at every column and the matrix path's per-lane event lists
    overflow (exact rescan of the marked rows); every other row keeps its events."""
    import torch
    P = 2
    ex, frames, kps, desc, cnt = _c3_batch(P, 9400)
    N = cnt.cpu().numpy()
    D = desc.cpu().numpy().copy()
    rng = np.random.default_rng(11)
    for p in range(P):
        q = P + p
        n2 = N[q]
        src = D[p, np.arange(n2) % 4]
        flip = (rng.random((n2, 32)) < 0.02) * (1 << rng.integers(0, 8, (n2, 32)))
        D[q, :n2] = np.where(rng.random((n2, 1)) < 0.5, src ^ flip.astype(np.uint8), D[q, :n2])
    dt = torch.from_numpy(D).cuda()
    F12, ep2 = stereo_tri_geometry()
    ep2 = np.array([650.0, 190.0], np.float32)
    Ft = torch.from_numpy(np.tile(F12, (P, 1))).cuda()
    Et = torch.from_numpy(np.tile(ep2, (P, 1))).cuda()
    f1 = torch.arange(P, dtype=torch.int32, device="cuda")
    scale, sigma2 = ex.GetScaleFactors(), ex.GetScaleSigmaSquares()
    m12, nm = search_for_triangulation_batch_device(kps, dt, cnt, kps, dt, cnt, Ft, Et, scale, sigma2,
                                                    frame1=f1, frame2=f1 + P)
    torch.cuda.synchronize()
    K = kps.cpu().numpy()
    M, NM = m12.cpu().numpy(), nm.cpu().numpy()
    for p in range(P):
        q = P + p
        exp, n = _oracle_pair(oracle, K[p], D[p], N[p], K[q], D[q], N[q], F12, ep2, scale, sigma2)
        assert np.array_equal(M[p, :N[p]], exp), p
        assert NM[p] == n and n > 0


def test_c3_empty_keyframes(tri_path):
    """A pair whose kf2 has no keypoints (every query -1, no matches) next to one whose kf1 has none."""
    import torch
    P = 2
    ex, frames, kps, desc, cnt = _c3_batch(P, 9500)
    c = cnt.clone()
    c[P] = 0      # kf2 of pair 0
    c[1] = 0      # kf1 of pair 1
    F12, ep2 = stereo_tri_geometry()
    Ft = torch.from_numpy(np.tile(F12, (P, 1))).cuda()
    Et = torch.from_numpy(np.tile(ep2, (P, 1))).cuda()
    f1 = torch.arange(P, dtype=torch.int32, device="cuda")
    scale, sigma2 = ex.GetScaleFactors(), ex.GetScaleSigmaSquares()
    cap = kps.shape[1]
    out = (torch.full((P, cap), 7, dtype=torch.int32, device="cuda"), torch.full((P,), 7, dtype=torch.int32, device="cuda"))
    m12, nm = search_for_triangulation_batch_device(kps, desc, c, kps, desc, c, Ft, Et, scale, sigma2,
                                                    frame1=f1, frame2=f1 + P, out=out)
    torch.cuda.synchronize()
    n0 = int(cnt[0])
    assert (m12[0, :n0] == -1).all() and int(nm[0]) == 0 and int(nm[1]) == 0


def test_c3_feature_vectors(oracle):
    """FeatureVector mode: DBoW2 transform on the device (levelsup 2) feeds the node join."""
    import torch
    from orb_slam2_refactored_amd.synth import make_vocabulary
    from orb_slam2_refactored_amd.vocabulary import ORBVocabulary
    P = 3
    ex, frames, kps, desc, cnt = _c3_batch(P, 9300)
    voc = make_vocabulary(21, L=4, k=6)
    g = ORBVocabulary.from_arrays(voc["k"], voc["L"], voc["scoring"], voc["weighting"], voc["parent"],
                                  voc["is_leaf"], voc["desc"], voc["weight"])
    bow = g.transform_batch_device(desc, cnt, levelsup=2)
    fv = (bow["fv_node"], bow["fv_off"], bow["fv_idx"], bow["n_nodes"])
    F12, ep2 = stereo_tri_geometry()
    Ft = torch.from_numpy(np.tile(F12, (P, 1))).cuda()
    Et = torch.from_numpy(np.tile(ep2, (P, 1))).cuda()
    f1 = torch.arange(P, dtype=torch.int32, device="cuda")
    scale, sigma2 = ex.GetScaleFactors(), ex.GetScaleSigmaSquares()
    m12, nm = search_for_triangulation_batch_device(kps, desc, cnt, kps, desc, cnt, Ft, Et, scale, sigma2,
                                                    frame1=f1, frame2=f1 + P, fv1=fv, fv2=fv)
    torch.cuda.synchronize()
    K, D, N = kps.cpu().numpy(), desc.cpu().numpy(), cnt.cpu().numpy()
    M, NM = m12.cpu().numpy(), nm.cpu().numpy()
    node, off, idx, nn = (t.cpu().numpy() for t in fv)

    def host_fv(f):
        k = nn[f]
        o = off[f, :k + 1]
        return node[f, :k].astype(np.uint32), o, idx[f, :o[-1]]

    for p in range(P):
        q = P + p
        assert nn[p] > 1
        exp, n = _oracle_pair(oracle, K[p], D[p], N[p], K[q], D[q], N[q], F12, ep2, scale, sigma2,
                              fv1=host_fv(p), fv2=host_fv(q))
        assert np.array_equal(M[p, :N[p]], exp), p
        assert NM[p] == n and n > 0


def test_tri_batch_rejects_bad_args():
    import torch
    from orb_slam2_refactored_amd._lib import OrbError
    k = torch.zeros((1, 8, 7), dtype=torch.int32, device="cuda")
    d = torch.zeros((1, 8, 32), dtype=torch.uint8, device="cuda")
    c = torch.zeros(1, dtype=torch.int32, device="cuda")
    F = torch.zeros((1, 9), dtype=torch.float32, device="cuda")
    e = torch.zeros((1, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(OrbError):
        search_for_triangulation_batch_device(k, d, c, k, d, c, F, e, np.ones(40, np.float32), np.ones(40, np.float32))
    with pytest.raises(ValueError):
        search_for_triangulation_batch_device(k, d[:, :4], c, k, d, c, F, e, np.ones(8, np.float32),
                                              np.ones(8, np.float32))
