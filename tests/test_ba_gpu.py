"""GPU LocalBundleAdjustment vs the oracle's g2o restatement: poses within 1e-4 RMSE, identical
outlier set and LM iteration counts (BASELINE.json north star)."""
from pathlib import Path

import numpy as np
import pytest

from ba_cases import CASE_IDS, EARLY_END_CASES, REFED_CASES, build_case, oracle_result
from orb_slam2_refactored_amd.optimizer import LocalBundleAdjustment
from orb_slam2_refactored_amd.synth import make_ba_problem

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
TOL = 1e-4   # pose RMSE tolerance (north star)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


def compare(g, o):
    assert rmse(g["pose_t"], o["pose_t"]) < TOL
    assert rmse(g["pose_R"], o["pose_R"]) < TOL
    assert rmse(g["points"], o["points"]) < 10 * TOL
    assert np.array_equal(g["edge_outlier"], o["edge_outlier"])
    assert tuple(g["iterations"]) == tuple(o["iterations"])


@pytest.mark.parametrize("seed,kf,pts,fixed", [(0, 20, 3000, 2), (1, 20, 3000, 2), (2, 12, 1500, 0), (3, 5, 200, 1)])
def test_local_ba_matches_oracle(oracle, seed, kf, pts, fixed):
    pr = make_ba_problem(seed, n_kf=kf, n_pts=pts, n_fixed=fixed)
    g = LocalBundleAdjustment(pr)
    o = oracle.local_ba(pr)
    compare(g, o)
    assert g["chi2"][1] < g["chi2"][0]


def test_local_ba_per_edge_cameras(oracle):
    """Edges with different cameras (a second calibration on every third keyframe) take the per-edge camera
    upload; one shared camera (every other test) is uploaded once (cam_step 0).  Both match the oracle."""
    pr = make_ba_problem(7, n_kf=10, n_pts=900, n_fixed=1)
    cam = pr["edge_cam"].copy()
    sel = (pr["edge_pose"] % 3) == 1
    cam[sel, 0] *= 1.01   # fx
    cam[sel, 2] += 2.0    # cx
    pr = dict(pr, edge_cam=cam)
    compare(LocalBundleAdjustment(pr), oracle.local_ba(pr))


@pytest.mark.parametrize("env", [("ORBBA_STRUCT", "host"), ("ORBBA_STRUCT", "sorted")])
def test_local_ba_struct_forms_identical(env, monkeypatch):
    """The structure built on the device (default: host counts + ba_struct_*_kernel lists) gives the
    same arrays as the host builds, so the whole call is bit-identical to ORBBA_STRUCT=host / sorted
    (tests/test_ba_struct_native.py checks the arrays on the CPU)."""
    pr = make_ba_problem(8, n_kf=20, n_pts=3000, n_fixed=2)
    a = LocalBundleAdjustment(pr)
    monkeypatch.setenv(*env)
    b = LocalBundleAdjustment(pr)
    for k in ("pose_t", "pose_R", "points", "edge_outlier", "iterations", "chi2"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_local_ba_unsorted_edges(oracle):
    """Edges not grouped by point (the device build's precondition) take the host build: same result as
    the oracle on the shuffled problem."""
    pr = make_ba_problem(9, n_kf=10, n_pts=800, n_fixed=1)
    perm = np.random.default_rng(9).permutation(len(pr["edge_point"]))
    pr = {k: (np.asarray(v)[perm] if k.startswith("edge_") else v) for k, v in pr.items()}
    compare(LocalBundleAdjustment(pr), oracle.local_ba(pr))


def test_local_ba_repeated_observation(oracle):
    """A point observed twice by the same free keyframe (two edges with the same (point, pose)) breaks
    the device structure build's precondition: the call takes the host build (generic path with
    nested pair loops) and still matches the oracle."""
    pr = make_ba_problem(10, n_kf=8, n_pts=600, n_fixed=1)
    ep, ek = np.asarray(pr["edge_point"]), np.asarray(pr["edge_pose"])
    fixed = np.asarray(pr["pose_fixed"]).astype(bool)
    dup = [e for e in range(0, len(ep), 37) if not fixed[ek[e]]][:10]
    order = np.sort(np.concatenate([np.arange(len(ep)), np.asarray(dup)]))   # duplicates next to their originals
    pr = {k: (np.asarray(v)[order] if k.startswith("edge_") else v) for k, v in pr.items()}
    compare(LocalBundleAdjustment(pr), oracle.local_ba(pr))


def test_local_ba_golden():
    z = np.load(GOLDEN / "local_ba_small.npz")
    pr = {k: z[k] for k in z.files if not k.startswith("out_")}
    g = LocalBundleAdjustment(pr)
    assert rmse(g["pose_t"], z["out_pose_t"]) < TOL
    assert np.array_equal(g["edge_outlier"], z["out_outlier"])
    assert tuple(g["iterations"]) == tuple(z["out_iterations"])


def test_local_ba_stop_flag(oracle):
    pr = make_ba_problem(4, n_kf=6, n_pts=300, n_fixed=1)
    g = LocalBundleAdjustment(pr, stop_flag=1)
    assert not g["ran"]   # Optimizer.cc:633-634: nothing optimised, nothing to write back
    assert tuple(g["iterations"]) == (0, 0)
    assert not g["edge_outlier"].any()
    assert rmse(g["points"], pr["points"]) == 0


def test_local_ba_deterministic():
    pr = make_ba_problem(6, n_kf=10, n_pts=800, n_fixed=1)
    a = LocalBundleAdjustment(pr)
    b = LocalBundleAdjustment(pr)
    assert np.array_equal(a["pose_t"], b["pose_t"]) and np.array_equal(a["points"], b["points"])


@pytest.mark.parametrize("seed,kf,pts,yaw", [(10, 24, 3000, 0.5), (11, 40, 5000, 0.5), (12, 64, 6000, 0.1),
                                              (13, 96, 8000, 0.05)])
def test_local_ba_large_window(oracle, seed, kf, pts, yaw):
    """More than 21 free keyframes (D = 6 x free > 128): the reduced system is factored in HBM by
    ba_solve_global_kernel; same outliers / iteration counts as the oracle's dense LDL^T."""
    pr = make_ba_problem(seed, n_kf=kf, n_pts=pts, n_fixed=2, yaw_per_kf=yaw)
    assert int((pr["pose_fixed"] == 0).sum()) > 21
    g = LocalBundleAdjustment(pr)
    o = oracle.local_ba(pr)
    compare(g, o)
    assert g["ran"] and g["chi2"][1] < g["chi2"][0]


@pytest.mark.parametrize("after", [1, 2, 3, 5, 8, 13])
def test_local_ba_stop_between_trials(oracle, after, monkeypatch):
    """The force-stop flag takes effect at the next trial boundary, as g2o's terminate() polls
    (levenberg.cpp:149, sparse_optimizer.cpp:376): the flag is raised right after `after` LM trials
    (test hook on both sides), and iteration counts / outliers / poses must equal the oracle's."""
    pr = make_ba_problem(20 + after, n_kf=12, n_pts=1500, n_fixed=1)
    monkeypatch.setenv("ORBBA_DEBUG_STOP_AFTER_TRIALS", str(after))
    g = LocalBundleAdjustment(pr)
    o = oracle.local_ba(pr, stop_after=after)
    compare(g, o)
    full = oracle.local_ba(pr)
    assert sum(g["iterations"]) <= sum(full["iterations"])
    if after < 5:
        assert g["iterations"][1] == 0   # stopped inside optimize(5): doMore is false


def test_local_ba_stop_flag_async():
    """A flag raised by another thread while the call runs ends it early without error."""
    import ctypes
    import threading
    import time
    pr = make_ba_problem(30, n_kf=40, n_pts=5000, n_fixed=2)
    full = LocalBundleAdjustment(pr)
    flag = ctypes.c_int32(0)
    t = threading.Timer(0.002, lambda: setattr(flag, "value", 1))
    t0 = time.perf_counter()
    t.start()
    g = LocalBundleAdjustment(pr, stop_flag=flag)
    t.join()
    assert g["ran"]
    assert sum(g["iterations"]) <= sum(full["iterations"])
    assert time.perf_counter() - t0 < 5


def test_local_ba_all_outliers_then_normal(oracle):
    """Every edge an outlier after optimize(5): the second optimize() has no level-0 edge, which the
    device learns on its own (no host copy of the levels) and ends at once with 0 iterations, as the
    oracle's g2o restatement; the next call on the same context runs normally."""
    pr = make_ba_problem(7, n_kf=6, n_pts=300, n_fixed=1)
    rng = np.random.default_rng(7)
    obs = np.array(pr["edge_obs"], np.float64)
    obs[:, :2] += rng.uniform(1000, 3000, (len(obs), 2)) * rng.choice([-1, 1], (len(obs), 2))
    pr["edge_obs"] = obs
    g = LocalBundleAdjustment(pr)
    o = oracle.local_ba(pr)
    assert g["edge_outlier"].all() and o["edge_outlier"].all()
    assert tuple(g["iterations"]) == tuple(o["iterations"]) and g["iterations"][1] == 0
    pr2 = make_ba_problem(3, n_kf=5, n_pts=200, n_fixed=1)
    compare(LocalBundleAdjustment(pr2), oracle.local_ba(pr2))


# Problems whose loops run differently: heavy outlier fractions (more rejected LM trials, so retries
# after the host's guess of the last step) and problems started at their ground truth.  Round 6
# enqueues each loop's end (the outlier classification, the second loop's ctl_start, the final gather)
# behind the step the host expects to be the last, guarded on `done`; a retry after that guess takes the
# host-driven path (ORBBA_DEBUG_TIMING=1 prints the hits and misses).  Every case must match the oracle.
# These generators always run the full (5, 10) iterations.  Loops that end before their budget (the nbad
# stop, rho == 0), where the host's guess of the last step is late rather than early, are
# tests/ba_cases.py's EARLY_END_CASES: re-fed windows, low-noise windows, the exact-fit problem and its
# one-bad-observation variant, whose decisions tests/test_ba_early_end_oracle.py shows to be far from
# rounding on the oracle (test_local_ba_early_end_* below).
_LOOP_END_CASES = [(20, 20, 3000, 2, 0.15, False), (21, 20, 3000, 2, 0.30, False), (22, 12, 1500, 0, 0.25, False),
                   (23, 8, 600, 1, 0.20, False), (24, 20, 3000, 2, 0.03, True), (25, 6, 300, 0, 0.10, True),
                   (26, 12, 1500, 1, 0.30, True), (27, 5, 120, 1, 0.0, True)]


def _loop_end_problem(seed, kf, pts, fixed, outl, at_gt):
    pr = make_ba_problem(seed, n_kf=kf, n_pts=pts, n_fixed=fixed, outlier_frac=outl)
    if at_gt:   # start at the ground truth: only the measurement noise is left to fit
        pr = dict(pr, pose_R=pr["gt_R"].copy(), pose_t=pr["gt_t"].copy(), points=pr["gt_points"].copy())
    return pr


@pytest.mark.parametrize("seed,kf,pts,fixed,outl,at_gt", _LOOP_END_CASES)
def test_local_ba_loop_end_variants(oracle, seed, kf, pts, fixed, outl, at_gt):
    pr = _loop_end_problem(seed, kf, pts, fixed, outl, at_gt)
    g = LocalBundleAdjustment(pr)
    o = oracle.local_ba(pr)
    compare(g, o)


@pytest.mark.parametrize("case", [_LOOP_END_CASES[0], _LOOP_END_CASES[1], _LOOP_END_CASES[3], _LOOP_END_CASES[5]])
def test_local_ba_loop_end_guess_misses(oracle, case, monkeypatch):
    """The loop ends enqueued one step too early (ORBBA_DEBUG_SPEC_EARLY): each loop's first guarded
    classification / ctl_start / gather does nothing, the host holds back further first-loop steps until
    the steps before them have reported, then goes on and enqueues the loop end again.  Same results."""
    monkeypatch.setenv("ORBBA_DEBUG_SPEC_EARLY", "1")
    pr = _loop_end_problem(*case)
    g = LocalBundleAdjustment(pr)
    o = oracle.local_ba(pr)
    compare(g, o)
    monkeypatch.delenv("ORBBA_DEBUG_SPEC_EARLY")
    g2 = LocalBundleAdjustment(pr)
    for k in ("pose_R", "pose_t", "points", "edge_outlier", "edge_chi2"):
        assert np.array_equal(g[k], g2[k]), k



# chi2 (the loops' final robust chi2, the C-ABI's chi2[2]) against the oracle's, relative.  Measured on the
# MI355X over test_local_ba_matches_oracle's four problems: largest |gpu - oracle| / oracle = CHI2_MEASURED
# (seed 3's second loop; the first loops agree to 1e-14); the tolerance is 100 x that, capped at 1e-6.  (The
# early-end cases themselves came out at 2e-10 and below.)
CHI2_MEASURED = 3.93e-8
CHI2_RTOL = min(100 * CHI2_MEASURED, 1e-6)   # = 1e-6
_RESULT_KEYS = ("pose_R", "pose_t", "pose_q", "points", "edge_outlier", "edge_chi2", "iterations", "chi2", "ran")


def _identical(a, b):
    for k in _RESULT_KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def _check_early_end(case, pr, g, o):
    compare(g, o)
    assert tuple(g["iterations"]) == case.iterations
    assert g["iterations"][0] < 5 or g["iterations"][1] < 10
    assert g["ran"]
    if case.kind == "exact":
        assert tuple(g["chi2"]) == (0.0, 0.0)
        for k in ("pose_R", "pose_t", "points"):
            assert np.array_equal(g[k], pr[k]), k
    else:
        for lp in (0, 1):
            rel = abs(g["chi2"][lp] - o["chi2"][lp]) / o["chi2"][lp]
            print(f"{case.id}: loop {lp} chi2 gpu {g['chi2'][lp]!r} oracle {o['chi2'][lp]!r} rel {rel:.3e}")
            assert rel <= CHI2_RTOL, (lp, rel)


@pytest.mark.parametrize("case", EARLY_END_CASES, ids=CASE_IDS)
def test_local_ba_early_end_matches_oracle(oracle, case):
    """Loops that end before their budget (nbad >= 3 after 3 .. 8 iterations, rho == 0 after one): the same
    iteration counts as the oracle, which are the table's literals, the same outliers, poses and chi2."""
    pr = build_case(oracle, case)
    _check_early_end(case, pr, LocalBundleAdjustment(pr), oracle_result(oracle, case))


@pytest.mark.parametrize("case", REFED_CASES, ids=[c.id for c in REFED_CASES])
def test_local_ba_early_end_guess_misses(oracle, case, monkeypatch):
    """An early end makes the host's guess of the last step late; ORBBA_DEBUG_SPEC_EARLY makes it early as
    well (test_local_ba_loop_end_guess_misses does that for full-length loops).  Bit-identical results."""
    pr = build_case(oracle, case)
    a = LocalBundleAdjustment(pr)
    monkeypatch.setenv("ORBBA_DEBUG_SPEC_EARLY", "1")
    b = LocalBundleAdjustment(pr)
    _check_early_end(case, pr, b, oracle_result(oracle, case))
    _identical(a, b)


@pytest.mark.parametrize("cid", ["refeed-8kf", "refeed-large", "lownoise-5kf", "exact-fit", "one-bad-133"])
def test_local_ba_early_end_context_reuse(oracle, cid):
    """The thread's context after an early end (nbad / q / done, the snapshot ring, steps enqueued past the
    end): a plain problem on it runs its full (5, 10) and matches the oracle, and the early-end case then
    repeats its first run bit for bit."""
    case = EARLY_END_CASES[CASE_IDS.index(cid)]
    pr = build_case(oracle, case)
    a = LocalBundleAdjustment(pr)
    _check_early_end(case, pr, a, oracle_result(oracle, case))
    plain = make_ba_problem(3, n_kf=5, n_pts=200, n_fixed=1)
    g = LocalBundleAdjustment(plain)
    compare(g, oracle.local_ba(plain))
    assert tuple(g["iterations"]) == (5, 10)
    _identical(a, LocalBundleAdjustment(pr))


def test_local_ba_early_end_struct_host(oracle, monkeypatch):
    """ORBBA_STRUCT=host on a re-fed case: bit-identical to the default structure build."""
    case = EARLY_END_CASES[CASE_IDS.index("refeed-large")]
    pr = build_case(oracle, case)
    a = LocalBundleAdjustment(pr)
    monkeypatch.setenv("ORBBA_STRUCT", "host")
    b = LocalBundleAdjustment(pr)
    _check_early_end(case, pr, b, oracle_result(oracle, case))
    _identical(a, b)


@pytest.mark.parametrize("offset", [-1, 0, 1])
def test_local_ba_stop_flag_meets_early_end(oracle, offset, monkeypatch):
    """The stop flag raised one trial before, at and one trial after the trial T that ends the second loop
    by nbad (T from the oracle's trace): each equals the oracle with the same stop_after."""
    case = EARLY_END_CASES[CASE_IDS.index("refeed-8kf")]
    pr = build_case(oracle, case)
    full = oracle_result(oracle, case)
    T = len(full["trace"])
    assert full["end_reason"][1] == "nbad" and T == 11
    monkeypatch.setenv("ORBBA_DEBUG_STOP_AFTER_TRIALS", str(T + offset))
    g = LocalBundleAdjustment(pr)
    o = oracle.local_ba(pr, stop_after=T + offset)
    compare(g, o)
    assert g["ran"]
    assert tuple(g["iterations"]) == ((5, 5) if offset < 0 else (5, 6))
    for lp in (0, 1):
        assert abs(g["chi2"][lp] - o["chi2"][lp]) <= CHI2_RTOL * o["chi2"][lp]
