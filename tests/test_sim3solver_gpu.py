"""Sim3Solver::iterate (src/Sim3Solver.cc:206-365) on the device against tests/sim3solver_ref.py (pinned by
tests/test_sim3solver_ref.py): found, iterations, terminate, inlier, match12 and n_inliers exactly equal, every
hypothesis's count inside the restatement's bounds [lo, hi] at margin M, max_inliers exact on success and inside
[max lo, max hi] on termination, s12 within TOL = 16 x the restatement's own spread under one-ulp jitter of M;
through the device and the host entries, with fix_scale 0 and 1 and max_iterations 1, 64, 65 and 300."""
import numpy as np
import pytest

import sim3_ref
import sim3solver_ref as R
from orb_slam2_refactored_amd.matcher import SearchBySim3, search_by_sim3_device
from orb_slam2_refactored_amd.optimizer import OptimizeSim3, optimize_sim3_device
from orb_slam2_refactored_amd.sim3solver import Sim3SolverIterate, sim3solver_iterate_device
from orb_slam2_refactored_amd.synth import make_sim3_batch, make_sim3solver_batch
from test_sim3solver_ref import GPU_CORR, M, TOL, gpu_batch, gpu_reference

pytestmark = pytest.mark.gpu

_HOST_KEYS = ("level_sigma2", "inv_level_sigma2", "scale_factors", "gt_s12", "outlier", "n_corr")
_FIELDS = ("s12", "inlier", "match12", "found", "n_inliers", "iterations", "max_inliers", "terminate", "hyp_inliers")


def to_device(b):
    import torch
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) and k not in _HOST_KEYS else v)
            for k, v in b.items()}


def _device(b, stream=None, out=None):
    import torch
    o = sim3solver_iterate_device(to_device(b), out=out, stream=stream)
    torch.cuda.synchronize()
    K1, F = int(b["kp1_begin"][-1]), len(b["kp1_begin"]) - 1
    return {k: o[k].cpu().numpy()[:K1 if k in ("inlier", "match12") else F] for k in _FIELDS}


def _same(a, c, what):
    for k in _FIELDS:
        assert a[k].tobytes() == c[k].tobytes(), (what, k)


def _check(b, got, exp, what, pairs=None):
    F = len(b["kp1_begin"]) - 1
    mn = int(b["min_inliers"])
    for p in (range(F) if pairs is None else pairs):
        assert R.stop_is_decided(exp, b, p), (what, p, "the restatement's own stop decision is not settled")
        k0, k1 = int(b["kp1_begin"][p]), int(b["kp1_begin"][p + 1])
        for k in ("found", "iterations", "terminate", "n_inliers"):
            assert got[k][p] == exp[k][p], (what, p, k, got[k][p], exp[k][p])
        for k in ("inlier", "match12"):
            assert np.array_equal(got[k][k0:k1], exp[k][k0:k1]), (what, p, k)
        h, ev = got["hyp_inliers"][p], exp["hyp_inliers"][p] >= 0
        assert np.array_equal(h >= 0, ev), (what, p, "evaluated range")
        off = int((h[ev] != exp["n"][p][ev]).sum())
        print(what, "pair", p, "hypotheses", int(ev.sum()), "counts that differ from the restatement's", off)
        assert (h[ev] >= exp["lo"][p][ev]).all() and (h[ev] <= exp["hi"][p][ev]).all(), (what, p, "hyp_inliers outside [lo, hi]")
        if exp["found"][p] == 1:
            assert got["max_inliers"][p] == exp["max_inliers"][p] and got["n_inliers"][p] > mn
            d = R.spread(exp["s12"][p], got["s12"][p])
            print(what, "pair", p, "s12 distance to the restatement (rot, t, s):", d)
            assert (d <= np.array(TOL)).all(), (what, p, d, TOL)
            if b["fix_scale"]:
                assert got["s12"][p][12].tobytes() == np.float32(1).tobytes()
        else:
            lo = max([0] + exp["lo"][p][ev].tolist()), max([0] + exp["hi"][p][ev].tolist())
            assert lo[0] <= got["max_inliers"][p] <= lo[1], (what, p, got["max_inliers"][p], lo)
            assert not got["s12"][p].any() and not got["inlier"][k0:k1].any() and (got["match12"][k0:k1] == -1).all()


@pytest.mark.parametrize("fix_scale", [0, 1])
@pytest.mark.parametrize("max_iterations", [1, 64, 65, 300])
def test_iterate_vs_reference(fix_scale, max_iterations):
    b, exp = gpu_batch(fix_scale, max_iterations, 300), gpu_reference(fix_scale, max_iterations, 300)
    dev, host = _device(b), Sim3SolverIterate(b)
    _check(b, dev, exp, "device")
    _same(dev, host, "host entry against device entry")
    if max_iterations == 300:
        assert (exp["found"][4:] == 1).all() and tuple(exp["terminate"][:3]) == (1, 1, 1)


def test_iterate_repeatable_and_on_a_side_stream():
    import torch
    b = gpu_batch(0)
    a = _device(b)
    _same(a, _device(b), "run to run")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = _device(b, stream=st)
    _same(a, c, "side stream")


def _chunk_batch():
    # few inliers: the first success comes late, after several chunks, and one pair never succeeds
    return make_sim3solver_batch(31, n_corr=[25, 60, 150, 150], outlier_frac=[0.3, 0.5, 0.6, 0.9], maxk=300)


def test_chunks_of_five_equal_one_call():
    """maxk = 5 with the state carried against maxk = 300: exact, no tolerance."""
    import torch
    b = _chunk_batch()
    F = 4
    one = _device(b)
    exp = R.iterate(b)
    assert np.array_equal(one["found"], exp["found"]) and (one["iterations"] > 5).any() and (one["found"] == 0).any()
    d = to_device(dict(b, maxk=5))
    out = None
    first = {}
    for _ in range(60):
        out = sim3solver_iterate_device(d, out=out)
        torch.cuda.synchronize()
        found = out["found"].cpu().numpy()
        for p in range(F):
            if p not in first and (found[p] == 1 or out["terminate"][p].item() == 1):
                k0, k1 = int(b["kp1_begin"][p]), int(b["kp1_begin"][p + 1])
                first[p] = {k: (out[k][k0:k1] if k in ("inlier", "match12") else out[k][p]).cpu().numpy().copy()
                            for k in _FIELDS if k != "hyp_inliers"}
        for p in first:   # a finished pair is parked: the caller stops iterating it
            out["iterations"][p] = 10 ** 6
        if len(first) == F:
            break
    assert len(first) == F
    for p in range(F):
        k0, k1 = int(b["kp1_begin"][p]), int(b["kp1_begin"][p + 1])
        for k, v in first[p].items():
            w = one[k][k0:k1] if k in ("inlier", "match12") else one[k][p]
            assert np.asarray(v).tobytes() == np.asarray(w).tobytes(), (p, k, v, w)


def test_resume_after_a_success():
    b = make_sim3solver_batch(12, n_corr=[80, 150], outlier_frac=[0.3, 0.2], maxk=300)
    first = _device(b)
    assert (first["found"] == 1).all()
    b2 = dict(b, iterations=first["iterations"], max_inliers=first["max_inliers"])
    exp = R.iterate(b2, margin=M)
    got = _device(b2)
    _check(b2, got, exp, "resumed")
    _same(got, Sim3SolverIterate(b2), "resumed, host entry")


def test_over_limit_pair():
    """A keyframe with more than ORBM_PROJ_MAX_KP slots: found = -1 from the device entry, its neighbours as the
    restatement has them; the host entry refuses the batch."""
    from orb_slam2_refactored_amd._lib import OrbError
    b = make_sim3solver_batch(5, n_corr=[60, 8200, 40], outlier_frac=[0.2, 0.0, 0.1], extras=0)
    got = _device(b)
    k0, k1 = int(b["kp1_begin"][1]), int(b["kp1_begin"][2])
    assert got["found"][1] == -1 and got["terminate"][1] == 1 and got["iterations"][1] == 0 and got["n_inliers"][1] == 0
    assert not got["inlier"][k0:k1].any() and (got["match12"][k0:k1] == -1).all() and (got["hyp_inliers"][1] == -1).all()
    exp = R.iterate(b, margin=M, pairs=[0, 2])
    assert (exp["found"][[0, 2]] == 1).all()
    _check(b, got, exp, "neighbours", pairs=[0, 2])
    with pytest.raises(OrbError, match="ORBM_PROJ_MAX_KP"):
        Sim3SolverIterate(b)


def test_solver_feeds_search_by_sim3_and_optimize_sim3_on_the_device():
    """LoopClosing.cc:115-139 without a host round trip: the solver's s12 and match12 go through torch ops on the
    device (the merge of LoopClosing.cc:133-137) into search_by_sim3_device and optimize_sim3_device; equal to the
    same chain staged through the three host entries."""
    import torch
    sb = make_sim3_batch(45, n_pairs=2, n_kp1=[400, 700], n_kp2=[500, 600], th=7.5)
    F, K1 = 2, int(sb["kp1_begin"][-1])
    # the BoW matches the solver starts from: SearchBySim3's own agreement under the generator's S12, a third dropped
    seed12 = sim3_ref.search_by_sim3(sb)[0].copy()
    seed12[::3] = -1
    sig = (np.asarray(sb["scale_factors"], np.float64) ** 2).astype(np.float32)
    isig = (1.0 / np.asarray(sb["scale_factors"], np.float64) ** 2).astype(np.float32)
    from orb_slam2_refactored_amd.sim3solver import make_draws
    extra = dict(level_sigma2=sig, draws=make_draws(F, 300, 9), min_inliers=20, max_iterations=300, maxk=300, probability=0.99,
                 fix_scale=0)
    has1, has2 = sb["mp1_valid"].copy(), sb["mp2_valid"].copy()   # "has a good map point", before any matching

    # staged through the host entries
    hs = Sim3SolverIterate(dict(sb, match12=seed12, **extra))
    assert (hs["found"] == 1).all()
    v1 = has1 & (hs["match12"] < 0)                    # :1130: not yet matched
    taken = np.zeros(len(has2), np.uint8)
    for p in range(F):
        k1, k1e, k2 = int(sb["kp1_begin"][p]), int(sb["kp1_begin"][p + 1]), int(sb["kp2_begin"][p])
        m = hs["match12"][k1:k1e]
        taken[k2 + m[m >= 0]] = 1
    v2 = has2 & (1 - taken)
    h12 = SearchBySim3(dict(sb, s12=hs["s12"], mp1_valid=v1, mp2_valid=v2))[0]
    hm = np.where(hs["match12"] >= 0, hs["match12"], h12).astype(np.int32)
    ho = OptimizeSim3(dict(sb, s12=hs["s12"], match12=hm, mp1_valid=has1, mp2_valid=has2, inv_level_sigma2=isig, max_chi2=10.0,
                           fix_scale=0))

    # the same on the device, torch ops between the calls
    d = to_device(dict(sb, match12=seed12, **extra))
    ds = sim3solver_iterate_device(d)
    m12 = ds["match12"][:K1]
    dv1 = d["mp1_valid"] * (m12 < 0).to(torch.uint8)
    kb2 = d["kp2_begin"].long()
    pair_of = torch.bucketize(torch.arange(K1, device="cuda"), d["kp1_begin"].long()[1:], right=True)
    dtaken = torch.zeros_like(d["mp2_valid"])
    sel = m12 >= 0
    dtaken[(kb2[pair_of] + m12.long())[sel]] = 1
    dv2 = d["mp2_valid"] * (1 - dtaken)
    s12 = ds["s12"].contiguous()
    g12 = search_by_sim3_device(dict(d, s12=s12, mp1_valid=dv1.contiguous(), mp2_valid=dv2.contiguous()))[0]
    dm = torch.where(sel, m12, g12[:K1]).contiguous()
    do = optimize_sim3_device(dict(d, s12=s12, match12=dm, inv_level_sigma2=isig, max_chi2=10.0, fix_scale=0))
    torch.cuda.synchronize()
    assert np.array_equal(dm.cpu().numpy(), hm) and (hm != hs["match12"]).any()
    for k in ("s12", "match12", "n_inliers", "iterations"):
        assert do[k].cpu().numpy()[:len(ho[k])].tobytes() == ho[k].tobytes(), k
    assert (ho["n_inliers"] >= 20).all()
