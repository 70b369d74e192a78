"""PnPsolver on the device against tests/pnpsolver_ref.py (pinned by tests/test_pnpsolver_ref.py, which also checks on
the CPU that every candidate of these batches has a decided stop and holds MARGIN and TOL)."""
import functools
import math

import numpy as np
import pytest
import torch

import pnpsolver_ref as ref
from orb_slam2_refactored_amd import optimizer
from orb_slam2_refactored_amd._lib import OrbError
from orb_slam2_refactored_amd.pnpsolver import PnPsolverIterate, make_draws, pnpsolver_iterate_device
from test_pnpsolver_ref import MARGIN, CARRIED_P, GPU_CASES, GPU_N, N_DRAWS, TOL, carried_case, carried_reference, gpu_batch, gpu_reference

pytestmark = pytest.mark.gpu

_ARR = ("kp_begin", "kp_xy", "kp_octave", "camera", "mp_valid", "mp_xw", "draws")
_STATE = ("iterations", "best_inliers", "best_mask", "best_tcw")
_OUT = ("tcw", "inlier", "found", "n_inliers", "terminate", "hyp_inliers") + _STATE


def to_device(b):
    d = dict(b)
    for k in _ARR + _STATE:
        if b.get(k) is not None:
            d[k] = torch.as_tensor(np.ascontiguousarray(b[k])).cuda()
    return d


def run_device(b, out=None, stream=None):
    o = pnpsolver_iterate_device(to_device(b), out, stream)
    torch.cuda.synchronize()
    F, K = len(b["kp_begin"]) - 1, int(b["kp_begin"][-1])
    r = {k: o[k].cpu().numpy() for k in _OUT}
    for k in ("inlier", "best_mask"):
        r[k] = r[k][:K]
    r["best_tcw"] = r["best_tcw"][:12 * F].reshape(F, 12)
    return r, o


@functools.lru_cache(maxsize=None)
def device_result(case):
    return run_device(gpu_batch(**GPU_CASES[case]))[0]


def same_bytes(a, b):
    for k in _OUT:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.parametrize("case", list(GPU_CASES))
def test_device_equals_the_restatement(case):
    r, d = gpu_reference(case), device_result(case)
    for k in ("found", "iterations", "terminate", "n_inliers", "inlier"):
        assert (d[k] == r[k]).all(), (k, d[k][:len(GPU_N)], r[k][:len(GPU_N)])
    ev = r["hyp_inliers"] >= 0
    assert ((d["hyp_inliers"] >= 0) == ev).all()   # the evaluated range
    # (a hypothesis the reference stopped before keeps its count in n but is -1 in hyp_inliers)
    assert (d["hyp_inliers"][ev] >= r["lo"][ev]).all() and (d["hyp_inliers"][ev] <= r["hi"][ev]).all()
    print(f"\n{case}: {int((d['hyp_inliers'][ev] != r['n'][ev]).sum())} of {int(ev.sum())} hypothesis counts differ from n[k]")
    for p in range(len(GPU_N)):
        if r["found"][p] > 0:
            assert d["best_inliers"][p] == r["best_inliers"][p]
            s = ref.spread(d["tcw"][p], r["tcw"][p])
            assert s[0] <= TOL[0] and s[1] <= TOL[1], (p, s)
        else:
            assert (d["tcw"][p] == 0).all()
            e = np.nonzero(ev[p])[0]
            mi = r["min_inliers_adj"][p]
            los = [int(r["lo"][p, k]) for k in e if r["lo"][p, k] >= mi] + [0]
            his = [int(r["hi"][p, k]) for k in e if r["hi"][p, k] >= mi] + [0]
            assert max(los) <= d["best_inliers"][p] <= max(his)
    assert (d["best_mask"].reshape(-1) <= 1).all()


def test_host_entry_run_to_run_and_side_stream_are_byte_equal():
    b = gpu_batch()
    d = device_result("reloc")
    same_bytes(d, PnPsolverIterate(b))
    same_bytes(d, run_device(b)[0])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        r2 = run_device(b, stream=st)[0]
    same_bytes(d, r2)


def against_restatement(d, r):
    """The exact outputs, every visible count inside [lo, hi], the state and the pose of a result d against r."""
    for k in ("found", "iterations", "terminate", "n_inliers", "inlier", "best_inliers", "best_mask"):
        assert (d[k].reshape(-1) == r[k].reshape(-1)).all(), k
    ev = r["hyp_inliers"] >= 0
    assert ((d["hyp_inliers"] >= 0) == ev).all()
    assert (d["hyp_inliers"][ev] >= r["lo"][ev]).all() and (d["hyp_inliers"][ev] <= r["hi"][ev]).all()
    for p in np.nonzero(r["found"] > 0)[0]:
        s = ref.spread(d["tcw"][p], r["tcw"][p])
        assert s[0] <= TOL[0] and s[1] <= TOL[1], (p, s)


def cand_bytes(r, b, p, hyp=slice(None)):
    k0, k1 = int(b["kp_begin"][p]), int(b["kp_begin"][p + 1])
    return b"".join(np.ascontiguousarray(x).tobytes() for x in (
        r["tcw"][p], r["inlier"][k0:k1], r["found"][p], r["n_inliers"][p], r["terminate"][p], r["iterations"][p],
        r["best_inliers"][p], r["best_mask"][k0:k1], r["best_tcw"][p], r["hyp_inliers"][p, hyp]))


def park(r):
    """The state of a result, through the host, as fresh device tensors."""
    return {k: torch.as_tensor(np.array(r[k])).reshape(-1).cuda() for k in _STATE}


def test_state_carry_one_call_equals_a_pair_of_calls():
    """max_iterations = 300, epsilon = 0.1 in one call against the same work in two: a first call with
    max_iterations = 64 (cap 64: hypotheses [0, 64)), its state parked, then a call with max_iterations = 300, which
    the OR rule sends over [64, 300).  Exact, byte for byte."""
    b = gpu_batch(**GPU_CASES["eps01_it300"])
    one = device_result("eps01_it300")
    cap = gpu_reference("eps01_it300")["cap"]
    first = device_result("eps01_it64")
    second, _ = run_device(b, out=park(first))
    split = 0
    for p in range(len(GPU_N)):
        if first["found"][p] == 1 or cap[p] <= 64:   # the first call is already the whole of the one call
            if cap[p] <= 64 or first["found"][p] == 1:
                assert cand_bytes(first, b, p) == cand_bytes(one, b, p), p
            continue
        split += 1
        assert cand_bytes(second, b, p, slice(64, None)) == cand_bytes(one, b, p, slice(64, None)), p
        assert (first["hyp_inliers"][p, :64] == one["hyp_inliers"][p, :64]).all() and (second["hyp_inliers"][p, :64] == -1).all()
    assert split >= 4   # the candidates whose events come after hypothesis 64, or never


def test_an_exhausted_solver_runs_maxk_more_from_its_state():
    b = gpu_batch(**GPU_CASES["eps01_it300"])
    one = device_result("eps01_it300")
    ex = np.nonzero((one["terminate"] == 1) & (one["iterations"] > 0))[0]
    assert len(ex) >= 2 and (one["iterations"][ex] == 300).any()
    more, _ = run_device(b, out=park(one))
    r = ref.iterate(dict(b, **{k: one[k] for k in _STATE}), margin=MARGIN)
    against_restatement(more, r)
    for p in ex:
        if one["found"][p] != 1:
            assert (np.nonzero(more["hyp_inliers"][p] >= 0)[0] == np.arange(one["iterations"][p], one["iterations"][p] + 5)).all()


def test_a_failed_refine_of_the_carried_best_then_a_record_that_succeeds():
    b, r = carried_case(), carried_reference()
    d, _ = run_device(b)
    against_restatement(d, r)
    assert d["found"][CARRIED_P] == 1 and d["iterations"][CARRIED_P] > 64 and len(r["refines"][CARRIED_P]) >= 2
    same_bytes(d, PnPsolverIterate(b))


def test_resume_after_a_success_succeeds_at_its_first_event():
    b = gpu_batch()
    d = device_result("reloc")
    nxt, _ = run_device(b, out={k: torch.as_tensor(np.ascontiguousarray(d[k])).cuda() for k in _STATE})
    for p in np.nonzero(d["found"] == 1)[0]:
        ev = np.nonzero(nxt["hyp_inliers"][p] >= 0)[0]
        if nxt["found"][p] == 1:   # the first event: nothing before it reached minInliers
            mi = ref.ransac_parameters(GPU_N[p])[0]
            assert (nxt["hyp_inliers"][p, ev[:-1]] < mi).all()
            assert nxt["iterations"][p] == ev[-1] + 1
    assert (nxt["found"][d["found"] == 1] >= 1).all()


def test_refused_candidates_leave_their_state_and_their_neighbours_alone():
    b = gpu_batch()
    big = 8193
    kb = np.concatenate([b["kp_begin"], [b["kp_begin"][-1] + big]]).astype(np.int32)
    rng = np.random.default_rng(0)
    bb = dict(b, kp_begin=kb, kp_xy=np.concatenate([b["kp_xy"], rng.uniform(0, 300, (big, 2)).astype(np.float32)]),
              kp_octave=np.concatenate([b["kp_octave"], np.zeros(big, np.int32)]), camera=np.concatenate([b["camera"], b["camera"][:1]]),
              mp_valid=np.concatenate([b["mp_valid"], np.ones(big, np.uint8)]),
              mp_xw=np.concatenate([b["mp_xw"], rng.uniform(1, 9, (big, 3)).astype(np.float32)]),
              draws=make_draws(len(GPU_N) + 1, N_DRAWS, 11), iterations=np.r_[np.zeros(len(GPU_N), np.int32), 7],
              best_inliers=np.r_[np.zeros(len(GPU_N), np.int32), 3])
    bb["draws"][:len(GPU_N)] = b["draws"]
    d, _ = run_device(bb)
    assert d["found"][-1] == -1 and d["terminate"][-1] == 1 and d["iterations"][-1] == 7 and d["best_inliers"][-1] == 3
    assert (d["tcw"][-1] == 0).all() and (d["inlier"][kb[-2]:] == 0).all()
    base = device_result("reloc")
    for k in ("found", "iterations", "n_inliers", "terminate", "tcw"):
        assert (d[k][:-1] == base[k]).all(), k
    with pytest.raises(OrbError, match="ORBM_PROJ_MAX_KP"):
        PnPsolverIterate(bb)
    # a draw table too short for an exhausted solver's maxk more
    short = dict(b, th2=1e-9, draws=np.ascontiguousarray(b["draws"][:, :36]))   # no event: every solver runs its cap
    s1, o = run_device(short)
    s2, _ = run_device(dict(short, maxk=5), out={k: o[k].clone() for k in _STATE})
    ex = s1["iterations"] + 5 > 36   # cap 35: five more would read draws[36 .. 40)
    assert (s2["found"][~ex] >= 0).all()
    assert ex.any() and (s2["found"][ex] == -1).all() and (s2["iterations"][ex] == s1["iterations"][ex]).all()
    assert (s2["best_inliers"][ex] == s1["best_inliers"][ex]).all()
    with pytest.raises(OrbError, match="n_draws"):
        PnPsolverIterate(dict(short, **{k: s1[k] for k in _STATE}))


def _pose_batch(xp, tcw, inlier, found, b, frame_of):
    """Tracking.cc:362-380 in array ops (xp: numpy or torch): the frame's map points are the solver's inliers, the
    pose its tcw (the identity where nothing was returned: such a frame has no edge)."""
    F = tcw.shape[0]
    sel = xp.nonzero(inlier != 0)
    sel = sel[0] if xp is np else sel[:, 0]
    counts = xp.bincount(frame_of[sel], minlength=F)
    zero = xp.zeros(1, dtype=counts.dtype) if xp is np else xp.zeros(1, dtype=counts.dtype, device=counts.device)
    begin = xp.cumsum(xp.concatenate([zero, counts]) if xp is np else xp.cat([zero, counts]), 0)
    eye = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    if xp is np:
        pose = np.where((found > 0)[:, None], tcw, np.array(eye, np.float32)).astype(np.float64)
        one = -np.ones((len(sel), 1))
        return dict(edge_begin=begin.astype(np.int32), pose_R=np.ascontiguousarray(pose[:, :9]), pose_t=np.ascontiguousarray(pose[:, 9:]),
                    cam=np.concatenate([b["camera"].astype(np.float64), np.zeros((F, 1))], 1), xw=b["mp_xw"][sel].astype(np.float64),
                    obs=np.concatenate([b["kp_xy"][sel].astype(np.float64), one], 1),
                    inv_sigma2=1.0 / b["level_sigma2"].astype(np.float64)[b["kp_octave"][sel]])
    pose = xp.where((found > 0)[:, None], tcw, xp.tensor(eye, dtype=xp.float32, device=tcw.device)).double()
    one = -xp.ones((sel.numel(), 1), dtype=xp.float64, device=tcw.device)
    sig = xp.as_tensor(b["level_sigma2"].astype(np.float64)).cuda()
    return dict(edge_begin=begin.int().contiguous(), pose_R=pose[:, :9].contiguous(), pose_t=pose[:, 9:].contiguous(),
                cam=xp.cat([b["camera_t"].double(), xp.zeros((F, 1), dtype=xp.float64, device=tcw.device)], 1).contiguous(),
                xw=b["mp_xw_t"][sel].double().contiguous(), obs=xp.cat([b["kp_xy_t"][sel].double(), one], 1).contiguous(),
                inv_sigma2=(1.0 / sig[b["kp_octave_t"][sel].long()]).contiguous())


def _reloc_batch(xp, b, ro, sel, pose_R, pose_t, n_good, outlier, found):
    """Tracking.cc:383-403 in array ops: the frame keeps the map points PoseOptimization left as inliers
    (kp_claimed), the candidate keyframe's points that are not among them are searched (mp_valid), and only where
    a pose was found and fewer than 50 inliers remain."""
    K, F = ro["K"], ro["F"]
    if xp is np:
        claimed = np.zeros(K, np.uint8)
        claimed[sel] = 1 - outlier
        go = (found > 0) & (n_good < 50)
        valid = (ro["kf_valid"] != 0) & (claimed == 0) & go[ro["frame_of"]]
        pose = np.concatenate([pose_R, pose_t], 1).astype(np.float32)
        return dict(ro["host"], kp_claimed=claimed, mp_valid=valid.astype(np.uint8), pose=np.ascontiguousarray(pose))
    claimed = xp.zeros(K, dtype=xp.uint8, device=sel.device)
    claimed[sel] = 1 - outlier
    go = (found > 0) & (n_good < 50)
    valid = (ro["kf_valid_t"] != 0) & (claimed == 0) & go[ro["frame_of_t"]]
    pose = xp.cat([pose_R, pose_t], 1).float().contiguous()
    return dict(ro["dev"], kp_claimed=claimed, mp_valid=valid.to(xp.uint8), pose=pose)


def test_chain_into_pose_optimization_and_the_projection_search_equals_the_host_chain():
    """Tracking.cc:336-430: SearchByBoW found 70 % of the correspondences; the solver's pose and inliers go through
    torch ops only into pose_optimization_device, and where fewer than 50 inliers remain the candidate keyframe's
    other points go into search_by_projection_reloc_device (th 10, ORBdist 100).  The same chain staged through the
    three host entries gives the same bytes."""
    from orb_slam2_refactored_amd.matcher import SearchByProjectionReloc, search_by_projection_reloc_device
    b = gpu_batch()
    F, K = len(GPU_N), int(b["kp_begin"][-1])
    rng = np.random.default_rng(5)
    kf_valid = b["mp_valid"].copy()                       # the keyframe's map points, one per slot
    b["mp_valid"] = (kf_valid * (rng.random(K) < 0.7)).astype(np.uint8)   # those SearchByBoW matched
    frame_of = np.repeat(np.arange(F), np.diff(b["kp_begin"]))
    desc = rng.integers(0, 256, (K, 32), dtype=np.uint8)  # a point's descriptor is its keypoint's
    angle = rng.uniform(0, 360, K).astype(np.float32)
    # maxDistance such that PredictScale gives the keypoint's own octave from the true camera centre
    Rg, tg = b["gt_tcw"][:, :9].reshape(F, 3, 3).astype(np.float64), b["gt_tcw"][:, 9:].astype(np.float64)
    centre = -np.einsum("fji,fj->fi", Rg, tg)
    dist = np.linalg.norm(b["mp_xw"] - centre[frame_of], axis=1)
    max_min = np.stack([dist * 1.2 ** (b["kp_octave"] - 0.5), np.full(K, 0.01)], 1).astype(np.float32)
    host = dict(kp_begin=b["kp_begin"], kp_xy=b["kp_xy"], kp_octave=b["kp_octave"], kp_desc=desc, kp_angle=angle,
                bounds=np.tile(np.array([0, 1241, 0, 376], np.float32), (F, 1)), camera=b["camera"], mp_begin=b["kp_begin"],
                mp_xw=b["mp_xw"], mp_max_min=max_min, mp_desc=desc, mp_angle=angle,
                scale_factors=(1.2 ** np.arange(8)).astype(np.float32), log_scale_factor=math.log(1.2), th=10.0, orb_dist=100,
                check_orientation=1)
    dev = {k: (torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) and k != "scale_factors" else v) for k, v in host.items()}
    ro = dict(K=K, F=F, host=host, dev=dev, kf_valid=kf_valid, frame_of=frame_of, kf_valid_t=torch.as_tensor(kf_valid).cuda(),
              frame_of_t=torch.as_tensor(frame_of).cuda())
    # the device chain
    d = to_device(b)
    o = pnpsolver_iterate_device(d)
    bt = dict(b, camera_t=d["camera"], mp_xw_t=d["mp_xw"], kp_xy_t=d["kp_xy"], kp_octave_t=d["kp_octave"])
    pd = _pose_batch(torch, o["tcw"][:F], o["inlier"][:K], o["found"][:F], bt, ro["frame_of_t"])
    rd = optimizer.pose_optimization_device(pd)
    E = int(pd["edge_begin"][-1])
    sel_d = torch.nonzero(o["inlier"][:K] != 0)[:, 0]
    qd = _reloc_batch(torch, b, ro, sel_d, rd["pose_R"], rd["pose_t"], rd["n_inliers"], rd["outlier"][:E], o["found"][:F])
    km_d, nm_d = search_by_projection_reloc_device(qd)
    torch.cuda.synchronize()
    # the host chain
    h = PnPsolverIterate(b)
    ph = _pose_batch(np, h["tcw"], h["inlier"], h["found"], b, frame_of)
    rh = optimizer.PoseOptimization(ph)
    qh = _reloc_batch(np, b, ro, np.nonzero(h["inlier"])[0], rh["pose_R"], rh["pose_t"], rh["n_inliers"], rh["outlier"], h["found"])
    km_h, nm_h = SearchByProjectionReloc(qh)
    assert E == int(ph["edge_begin"][-1]) and E > 100
    for k in ("pose_R", "pose_t", "n_inliers"):
        assert rd[k].cpu().numpy().tobytes() == rh[k].tobytes(), k
    assert rd["outlier"].cpu().numpy()[:E].tobytes() == rh["outlier"].tobytes()
    assert km_d.cpu().numpy()[:K].tobytes() == km_h.tobytes() and nm_d.cpu().numpy()[:F].tobytes() == nm_h.tobytes()
    went = (h["found"] > 0) & (rh["n_inliers"] < 50)
    assert went.sum() >= 3 and nm_h[went].sum() >= 10 and (nm_h[~went] == 0).all()   # the search found the points BoW had not
    assert (qh["kp_claimed"][km_h >= 0] == 0).all()


def test_the_device_wrapper_names_the_field_it_refuses():
    d = to_device(gpu_batch())
    for key, bad in (("kp_xy", d["kp_xy"].double()), ("kp_octave", d["kp_octave"].long()), ("mp_valid", d["mp_valid"].int()),
                     ("draws", d["draws"].long()), ("camera", d["camera"].t().contiguous().t()), ("mp_xw", d["mp_xw"].cpu()),
                     ("kp_begin", d["kp_begin"].long())):
        with pytest.raises(ValueError, match=f"pnpsolver_iterate_device: {key} must be"):
            pnpsolver_iterate_device(dict(d, **{key: bad}))
    with pytest.raises(ValueError, match="kp_octave has"):
        pnpsolver_iterate_device(dict(d, kp_octave=d["kp_octave"][:-1].contiguous()))
    K, F = d["mp_xw"].shape[0], len(GPU_N)
    for key, bad, msg in (("tcw", torch.zeros((F, 12), dtype=torch.float64).cuda(), r"out\['tcw'\] must be"),
                          ("inlier", torch.zeros(K - 1, dtype=torch.uint8).cuda(), "inlier has"),
                          ("best_mask", torch.zeros(K, dtype=torch.uint8), r"out\['best_mask'\] must be"),
                          ("hyp_inliers", torch.zeros((F, N_DRAWS - 1), dtype=torch.int32).cuda(), "hyp_inliers has")):
        with pytest.raises(ValueError, match=msg):
            pnpsolver_iterate_device(d, out={key: bad})
