"""The oracle on the rows of tests/pose_cases.py: its trace witnesses the branch each row claims, and on the
trials that make up a witness every accept / reject and relative-improvement decision is far from rounding,
which is what makes the device comparison (tests/test_pose_cases_gpu.py) a test of that branch.  Also: the
per-trial trace changes no result."""
import numpy as np
import pytest

from oracle_api import PO_END_REASONS, PO_QUAT_BRANCHES
from orb_slam2_refactored_amd.synth import make_pose_batch
from pose_cases import (BEHIND, BY_ID, CASE_IDS, CASES, EDGE_COUNTS, QUAT_TARGETS, build_case, oracle_result, planted,
                        swap_cameras)

# A fixed-order fp64 sum over <= 1100 edges differs between two orders by about n * eps = 2.4e-13 relative:
# four and seven orders below these (the margins of tests/test_ba_early_end_oracle.py).
MARGIN_TRIAL = 1e-9   # |cur - tmp| >= MARGIN_TRIAL * cur
MARGIN_NBAD = 1e-6    # |(ini - cur) * 1e3 - ini| >= MARGIN_NBAD * ini wherever the nbad test is reached
MARGIN_CLASS = 1e-9   # |chi2 - th| >= MARGIN_CLASS * th for every edge in every round
TOL = 1e-6            # the device's pose tolerance (tests/test_pose_gpu.py)


def reasons(o, f):
    r = o["rounds"]
    return tuple(PO_END_REASONS[x] for x in r["reason"][r["frame"] == f])


def check_margins(trials):
    assert len(trials) > 0
    for r in trials:
        assert abs(r["cur"] - r["tmp"]) >= MARGIN_TRIAL * r["cur"], (r["round"], r["it"], r["q"])
    for r in trials[trials["nbad_tested"] == 1]:
        assert abs((r["ini"] - r["cur_end"]) * 1e3 - r["ini"]) >= MARGIN_NBAD * r["ini"], (r["round"], r["it"])


def pose_distance(a, b):
    return max(np.abs(a["pose_R"] - b["pose_R"]).max(), np.abs(a["pose_t"] - b["pose_t"]).max())


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_row(oracle, case):
    """What holds for every row: the table's literals, the trace consistent with the counts it explains, and
    every classification far from its threshold."""
    b, o = build_case(case), oracle_result(oracle, case)
    eb = b["edge_begin"]
    E = np.diff(eb)
    assert ((E >= 12) & (E <= 1100)).all()
    tr, rd = o["trials"], o["rounds"]
    assert len(o["frames"]) == len(E) and len(rd) == 4 * len(E)
    for f in range(len(E)):
        r = rd[rd["frame"] == f]
        assert r["round"].tolist() == [0, 1, 2, 3]
        for k in range(4):
            t = tr[(tr["frame"] == f) & (tr["round"] == k)]
            assert int(t["iter_end"].sum()) == r["iterations"][k]
            assert (r["n_active"][k] == 0) == (PO_END_REASONS[r["reason"][k]] == "none") == (len(t) == 0)
        assert r["n_active"][0] == E[f]
        assert np.array_equal(r["n_active"][1:], E[f] - r["n_outliers"][:3])
        assert r["n_outliers"][3] == E[f] - o["n_inliers"][f] == o["outlier"][eb[f]:eb[f + 1]].sum()
        if case.iterations is not None and case.iterations[f] is not None:
            for k in range(4):
                if case.iterations[f][k] is not None:
                    assert r["iterations"][k] == case.iterations[f][k], (f, k)
                    assert PO_END_REASONS[r["reason"][k]] == case.reasons[f][k], (f, k)
    assert (rd["min_margin"] >= MARGIN_CLASS).all()


def test_cams_witness(oracle):
    b, o = build_case(BY_ID["cams"]), oracle_result(oracle, BY_ID["cams"])
    cam = b["cam"]
    assert len(cam) >= 4
    for f in range(len(cam)):
        for g in range(len(cam)):
            if f != g:
                ratio = np.maximum(cam[f] / cam[g], cam[g] / cam[f])
                assert (ratio >= 1.3 - 1e-6).all()
    assert np.array_equal(cam, cam.astype(np.float32).astype(np.float64))
    other = oracle.pose_optimization(swap_cameras(b))
    assert (other["n_inliers"] != o["n_inliers"]).all()
    assert (o["n_inliers"] > 45).all() and (other["n_inliers"] < 20).all()


def test_quat_witness(oracle):
    res = {name: oracle_result(oracle, BY_ID[name]) for name in QUAT_TARGETS}
    for name, (_, (branch, flipped)) in QUAT_TARGETS.items():
        fr = res[name]["frames"]
        assert len(fr) == 1
        assert PO_QUAT_BRANCHES[fr["branch"][0]] == branch and fr["flipped"][0] == flipped, name
    first = res["quat-t"]
    assert 40 < first["n_inliers"][0] < 60
    for name, o in res.items():   # one problem in five world frames
        assert np.array_equal(o["n_inliers"], first["n_inliers"]), name
        assert np.array_equal(o["outlier"], first["outlier"]), name
        assert np.abs(o["pose_t"] - first["pose_t"]).max() < 1e-4, name   # t = Xc - R X is frame-independent


def test_budget_witness(oracle):
    b, o = build_case(BY_ID["budget"]), oracle_result(oracle, BY_ID["budget"])
    assert "budget" in reasons(o, 0)
    tr = o["trials"]
    check_margins(tr)   # every trial of the row: all four rounds use the whole budget
    assert (tr["ok"] == 1).all()
    for other_budget in (9, 11):
        w = oracle.pose_optimization(b, trace=True, max_iters=other_budget)
        assert w["rounds"]["iterations"].tolist() == [other_budget] * 4
        assert pose_distance(w, o) >= 100 * TOL, other_budget


@pytest.mark.parametrize("name", ["solve-fail-mono", "solve-fail-stereo"])
def test_solve_fail_witness(oracle, name):
    """What the trace shows: round 0 is ten iterations of one rejected trial each.  H holds NaN, so does
    lambda (g2o's std::max keeps a NaN diagonal), the solve fails (ok 0), x = 0, cur = inf, tmp = DBL_MAX,
    scale = 0 * NaN = NaN, rho = NaN: neither accepted nor `rho < 0`, so each iteration ends after one trial;
    (inf - inf) * 1e3 < inf is false, so nbad stays 0 and the budget runs out.  The pose stays put, edge 0 is
    flagged (chi2 = inf), and rounds 1 to 3 run without it and never fail."""
    b, o = build_case(BY_ID[name]), oracle_result(oracle, BY_ID[name])
    tr = o["trials"]
    t0 = tr[tr["round"] == 0]
    assert len(t0) == 10 and t0["it"].tolist() == list(range(10)) and (t0["q"] == 0).all()
    assert (t0["ok"] == 0).all() and (t0["accepted"] == 0).all() and (t0["iter_end"] == 1).all()
    assert np.isnan(t0["rho"]).all() and np.isinf(t0["cur"]).all() and (t0["tmp"] == np.finfo(np.float64).max).all()
    assert (t0["nbad_tested"] == 1).all() and (t0["nbad"] == 0).all()
    rd = o["rounds"]
    assert rd["n_outliers"][0] >= 1 and o["outlier"][0] == 1
    assert rd["n_active"][1] == 40 - rd["n_outliers"][0] >= 35
    later = tr[tr["round"] > 0]
    assert len(later) > 0 and (later["ok"] == 1).all() and np.isfinite(later["rho"]).all()
    assert np.isfinite(o["pose_R"]).all() and np.isfinite(o["pose_t"]).all()
    # round 0 classified at the untouched prediction (R = I, t = 0)
    import pose_ref
    fr = pose_ref.Frame(b["xw"], b["obs"], b["inv_sigma2"], b["cam"][0])
    with np.errstate(all="ignore"):
        fr.compute_error(np.arange(40), (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)))
        assert int((fr.chi2(np.arange(40)) > fr.th).sum()) == rd["n_outliers"][0]


def test_solve_fail_nan_witness(oracle):
    """The stereo edge with x > 0: its disparity residual is inf - inf, chi2 is NaN, `chi2 > th` is false, the
    edge is never flagged and poisons all four rounds: 40 failed solves, the pose is the prediction, and the
    edge counts as an inlier."""
    b, o = build_case(BY_ID["solve-fail-nan"]), oracle_result(oracle, BY_ID["solve-fail-nan"])
    tr = o["trials"]
    assert len(tr) == 40 and (tr["ok"] == 0).all() and np.isnan(tr["cur"]).all() and np.isnan(tr["rho"]).all()
    assert o["outlier"][0] == 0 and (o["rounds"]["n_readmitted"] == 0).all()
    assert np.array_equal(o["pose_R"], b["pose_R"]) and np.array_equal(o["pose_t"], b["pose_t"])


def test_behind_witness(oracle):
    b, o = build_case(BY_ID["behind"]), oracle_result(oracle, BY_ID["behind"])
    Xc = b["xw"] @ b["pose_R"][0].reshape(3, 3).T + b["pose_t"][0]
    assert sorted(np.flatnonzero(Xc[:, 2] < 0)) == list(BEHIND)
    assert ((Xc[list(BEHIND), 2] < -3.5) & (Xc[list(BEHIND), 2] > -7.5)).all()
    tr = o["trials"]
    assert (tr["ok"] == 1).all() and np.isfinite(tr["cur"]).all() and np.isfinite(tr["tmp"]).all()
    assert np.isfinite(o["rounds"]["min_margin"]).all()
    assert o["outlier"][list(BEHIND)].all() and o["n_inliers"][0] >= 50
    check_margins(tr[(tr["round"] == 0) & (tr["it"] < 3)])   # the behind edges are active there


def test_exact_fit_witness(oracle):
    b, o = build_case(BY_ID["exact-fit"]), oracle_result(oracle, BY_ID["exact-fit"])
    st = b["obs"][:, 2] >= 0
    assert st.any() and (~st).any()
    tr = o["trials"]
    assert len(tr) == 4 and tr["round"].tolist() == [0, 1, 2, 3]
    for r in tr:
        assert r["cur"] == 0.0 and r["tmp"] == 0.0 and r["rho"] == 0.0 and r["ok"] == 1 and not r["accepted"]
    assert reasons(o, 0) == ("rho0",) * 4
    assert np.array_equal(o["pose_R"], b["pose_R"]) and np.array_equal(o["pose_t"], b["pose_t"])
    assert o["n_inliers"][0] == 24 and not o["outlier"].any()


@pytest.mark.parametrize("n", [2, 1])
def test_few_active_witness(oracle, n):
    o = oracle_result(oracle, BY_ID[f"active-{n}"])
    rd, tr = o["rounds"], o["trials"]
    few = rd["round"][rd["n_active"] == n]
    assert len(few) > 0 and (tr["ok"] == 1).all()
    assert o["n_inliers"][0] == n
    check_margins(tr[np.isin(tr["round"], few)])


def test_none_witness(oracle):
    o = oracle_result(oracle, BY_ID["all-out-then-none"])
    assert reasons(o, 1)[1:] == ("none",) * 3
    rd = o["rounds"]
    assert (rd["n_active"][(rd["frame"] == 1) & (rd["round"] > 0)] == 0).all() and o["n_inliers"][1] == 0
    tr = o["trials"]
    check_margins(tr[(tr["frame"] == 1) & (tr["round"] == 0) & (tr["it"] < 3)])


def test_edges_witness(oracle):
    b, o = build_case(BY_ID["edges"]), oracle_result(oracle, BY_ID["edges"])
    eb = b["edge_begin"]
    assert tuple(np.diff(eb)) == EDGE_COUNTS
    for f, E in enumerate(EDGE_COUNTS):
        p, nb = planted(E)
        flags = o["outlier"][eb[f]:eb[f + 1]]
        assert flags[p].all(), (E, p)
        assert not flags[nb].any(), (E, nb)
    assert planted(255) == ([0, 254], [1, 253]) and planted(1025)[0] == [0, 254, 255, 256, 1022, 1023, 1024]


@pytest.mark.parametrize("kw", [
    dict(seed=1, n_frames=8, n_edges=[0, 1, 2, 3, 9, 10, 11, 257]),
    dict(seed=0, n_frames=16, n_edges=600),
], ids=["ragged", "16x600"])
def test_trace_changes_nothing(oracle, kw):
    b = make_pose_batch(**kw)
    a = oracle.pose_optimization(b)
    t = oracle.pose_optimization(b, trace=True)
    for k in a:
        assert np.array_equal(a[k], t[k]), k
    ran = int((np.diff(b["edge_begin"]) >= 3).sum())
    assert len(t["frames"]) == ran and len(t["trials"]) >= 3 * ran
    assert t["rounds"]["iterations"].max() <= 10 and t["trials"]["q"].max() <= 9
