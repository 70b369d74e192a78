"""Pins tests/optsim3_ref.py, the restatement of Optimizer::OptimizeSim3 that tests/test_optsim3_gpu.py holds
the device to: g2o's Sim3 algebra against matrix algebra, answers that do not depend on the restatement
(noise-free data lands on the ground truth), the schedule's thresholds (9 / 10 correspondences, 9 survivors),
fix_scale, and the GPU batch: its margins and the spread of the reference's own result under one-ulp jitter
of every error evaluation, from which the GPU tolerance is derived.  CPU only."""
import functools

import numpy as np
import pytest

import optsim3_ref as R
from orb_slam2_refactored_amd.synth import make_optsim3_batch

_ARRAYS1 = ("kp1_xy", "kp1_octave", "mp1_valid", "mp1_xw", "match12", "outlier")
_ARRAYS2 = ("kp2_xy", "kp2_octave", "mp2_valid", "mp2_xw")
_PER_PAIR = ("pose1", "camera1", "pose2", "camera2", "s12", "gt_s12", "n_corr")


def concat_batches(bs):
    """One batch from single-pair batches (same pyramid, max_chi2 and fix_scale)."""
    out = dict(bs[0])
    for k in _ARRAYS1 + _ARRAYS2 + _PER_PAIR:
        out[k] = np.concatenate([b[k] for b in bs])
    for s in "12":
        out[f"kp{s}_begin"] = np.concatenate([[0], np.cumsum([b[f"kp{s}_begin"][-1] for b in bs])]).astype(np.int32)
    return out


# ---------------------------------------------------------------- the GPU batch
# (count, gross outliers) per pair: below / at / above the 10-correspondence thresholds, one lane short of, at
# and past one and two wavefronts, either side of the 128 correspondences the kernel stages in LDS, a typical
# candidate, and 600 so that a lane holds several edges and the tail past the staged ones is rebuilt per pass.
GPU_PAIRS = ((0, 0), (9, 0), (10, 0), (12, 3), (14, 2), (63, 6), (64, 6), (65, 6), (127, 12), (128, 12), (129, 12),
             (150, 15), (300, 30), (600, 60))
MAX_CHI2 = 10.0
JITTER_SEEDS = tuple(range(1, 9))
# Generator seed of every pair, per fix_scale, found by a search for seeds that keep the margins below (a
# seed that fails them is replaced here, not tolerated): test_gpu_batch_margins_and_spread asserts them.
GPU_SEEDS = {0: (1000, 1050, 1101, 1150, 1200, 1253, 1300, 1352, 1408, 1451, 1505, 1551, 1601, 1650),
             1: (2000, 2050, 2101, 2150, 2201, 2250, 2300, 2350, 2400, 2450, 2501, 2553, 2600, 2653)}
# Largest distance between the reference's s12_g2o and its own result under jitter, over the batch (both
# fix_scale values) and JITTER_SEEDS: (rotation angle [rad], |dt| / |t|, |ds| / s), measured by
# test_gpu_batch_margins_and_spread, which asserts that it is not exceeded.  The jitter models +-1 ulp per
# error evaluation; the device's sin / cos / exp / divide and its summation order add a few ulp more, and the
# amplification (by 1 / (2 delta) = 5e8 into the Jacobian) is linear: the device gets 16 x.
SPREAD = (1.6e-8, 4.1e-6, 5.8e-6)   # measured: 1.60e-8, 4.08e-6, 5.72e-6
# With fix_scale the 6-DoF problem converges inside the first optimize(5): from its fourth iteration on every
# trial's rho is rounding noise of order 1e-9 around 0, for every generator seed, so no seed can keep rho
# 1e-3 away from 0 there.  The fix_scale batch keeps the two other margins, of which "nothing discrete moves
# under any of the jitter seeds" is the one the rho margin stands for.
RHO_MARGIN = {0: True, 1: False}
TOL = tuple(16 * s for s in SPREAD)


@functools.lru_cache(maxsize=None)
def gpu_batch(fix_scale):
    return concat_batches([make_optsim3_batch(seed, n_corr=[n], n_outliers=[o], max_chi2=MAX_CHI2, fix_scale=bool(fix_scale))
                           for seed, (n, o) in zip(GPU_SEEDS[int(fix_scale)], GPU_PAIRS)])


@functools.lru_cache(maxsize=None)
def gpu_reference(fix_scale):
    """The restatement's result for gpu_batch(fix_scale), computed once and shared."""
    return R.optimize_sim3(gpu_batch(fix_scale))


def pair_margins(b, p, base, jittered, rho_margin=True):
    """What makes pair p of batch b a fair comparison: the discrete results do not move under jitter, no
    chi2 at either classification within 1 % of max_chi2, no trial's rho within 1e-3 of 0.  Returns (list of
    failures, spread [3])."""
    bad = []
    k0, k1 = int(b["kp1_begin"][p]), int(b["kp1_begin"][p + 1])
    spread = np.zeros(3)
    for j in jittered:
        if not (np.array_equal(j["match12"][k0:k1], base["match12"][k0:k1]) and j["n_inliers"][p] == base["n_inliers"][p]
                and np.array_equal(j["iterations"][p], base["iterations"][p])):
            bad.append("discrete results move under jitter")
            break
        spread = np.maximum(spread, R.spread(base["s12_g2o"][p], j["s12_g2o"][p]))
    for r in [base] + list(jittered):
        t = r["trace"][p]
        for chis in t["chi2"]:
            c = np.asarray(chis, np.float64)
            c = c[np.isfinite(c)]
            if c.size and np.abs(c / b["max_chi2"] - 1).min() < 0.01:
                bad.append("a chi2 within 1 % of max_chi2")
        if rho_margin and t["rho"] and np.abs(t["rho"]).min() < 1e-3:
            bad.append("a rho within 1e-3 of 0")
    return bad, spread


def test_gpu_batch_margins_and_spread():
    worst = np.zeros(3)
    for fs in (0, 1):
        b, base = gpu_batch(fs), gpu_reference(fs)
        assert tuple(b["n_corr"]) == tuple(n for n, _ in GPU_PAIRS)
        jittered = [R.optimize_sim3(b, jitter_seed=s) for s in JITTER_SEEDS]
        for p in range(len(GPU_PAIRS)):
            bad, spread = pair_margins(b, p, base, jittered, rho_margin=RHO_MARGIN[fs])
            assert not bad, (fs, p, GPU_SEEDS[fs][p], bad)
            worst = np.maximum(worst, spread)
        # the schedule's branches are all in the batch
        n, it = base["n_inliers"], base["iterations"]
        assert n[0] == 0 and tuple(it[0]) == (0, 0)
        assert n[1] == 0 and it[1][0] > 0 and it[1][1] == 0
        assert n[2] == 10 and it[2][1] > 0
        assert n[3] == 0 and it[3][1] == 0            # 12 - 3 = 9 survivors
        assert n[4] == 12 and it[4][1] > 0            # 14 - 2 = 12
        assert (n[5:] >= 10).all()
    print("spread (rotation rad, dt / |t|, ds / s):", worst)
    assert (worst <= np.array(TOL) / 16).all(), worst


# ---------------------------------------------------------------- g2o::Sim3 against matrix algebra
def _generator(u):
    G = np.zeros((4, 4))
    w = u[:3]
    G[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + u[6] * np.eye(3)
    G[:3, 3] = u[3:6]
    return G


@pytest.mark.parametrize("omega,sigma,tol_R,tol_t", [
    # |sigma| < eps, theta < eps: R = I + Omega + Omega^2 is off by Omega^2 / 2 = 5e-13; C = 1 stands for
    # (s - 1) / sigma = 1 + sigma / 2, so t is off by sigma / 2 = 5e-8 relative
    (1e-6, 1e-7, 1e-11, 6e-8),
    (0.3, 1e-7, 1e-13, 6e-8),      # |sigma| < eps, theta >= eps: R exact, the same C
    # |sigma| >= eps, theta < eps: A and B are their theta -> 0 limits; measured 8e-11, bounded here by theta
    # itself over 1000
    (1e-6, 0.2, 1e-11, 1e-9),
    (0.4, -0.3, 1e-13, 1e-13),     # the general branch
])
def test_sim3_exp_against_expm(omega, sigma, tol_R, tol_t):
    from scipy.linalg import expm
    rng = np.random.default_rng(3)
    w = rng.normal(size=3)
    u = np.concatenate([omega * w / np.linalg.norm(w), rng.normal(size=3), [sigma]])
    M = expm(_generator(u))
    S = R.sim3_exp([float(v) for v in u])
    got = R.sim3_matrix(S)
    assert np.abs(got[:3, :3] - M[:3, :3]).max() <= tol_R   # s R
    assert np.abs(got[:3, 3] - M[:3, 3]).max() <= tol_t * np.linalg.norm(M[:3, 3])


def test_sim3_inverse_and_product_against_matrices():
    rng = np.random.default_rng(4)
    A = R.sim3_exp([float(v) for v in rng.normal(0, 0.5, 7)])
    B = R.sim3_exp([float(v) for v in rng.normal(0, 0.5, 7)])
    MA, MB = R.sim3_matrix(A), R.sim3_matrix(B)
    assert np.abs(R.sim3_matrix(R.sim3_mul(A, B)) - MA @ MB).max() < 1e-14
    assert np.abs(R.sim3_matrix(R.sim3_inverse(A)) - np.linalg.inv(MA)).max() < 1e-14
    x = rng.normal(size=3)
    assert np.abs(np.array(R.sim3_map(A, [float(v) for v in x])) - (MA @ np.append(x, 1))[:3]).max() < 1e-14


# ---------------------------------------------------------------- hand-built cases (run again on the device)
def hand_cases():
    """(name, batch) of the schedule's cases; tests/test_optsim3_gpu.py runs them on the device."""
    return [("noise_free", make_optsim3_batch(20, n_corr=[40], noise=False)),
            ("fix_scale", make_optsim3_batch(23, n_corr=[40], n_outliers=[4], fix_scale=True)),
            ("nine", make_optsim3_batch(20, n_corr=[9])),
            ("ten", make_optsim3_batch(23, n_corr=[10], noise=False)),
            ("twelve_minus_three", make_optsim3_batch(20, n_corr=[12], n_outliers=[3])),
            ("fourteen_minus_two", make_optsim3_batch(34, n_corr=[14], n_outliers=[2]))]


def jitter_study(b):
    """(reference result, failures of the jitter and chi2 margins over every pair, spread [3] of s12_g2o over
    JITTER_SEEDS): a hand-built case is compared on the device within 16 x its own spread."""
    base = R.optimize_sim3(b)
    jittered = [R.optimize_sim3(b, jitter_seed=s) for s in JITTER_SEEDS]
    bad, spread = [], np.zeros(3)
    for p in range(len(b["kp1_begin"]) - 1):
        f, sp = pair_margins(b, p, base, jittered, rho_margin=False)
        bad += f
        spread = np.maximum(spread, sp)
    return base, bad, spread


def test_hand_cases_keep_their_discrete_results_under_jitter():
    for name, b in hand_cases():
        _, bad, _ = jitter_study(b)
        assert not bad, (name, bad)


def _case(name):
    return dict(hand_cases())[name]


def test_noise_free_lands_on_ground_truth():
    b = _case("noise_free")
    r = R.optimize_sim3(b)
    assert r["n_inliers"][0] == 40 and (r["match12"] == b["match12"]).all()
    # inputs are rounded to float32 (6e-8 relative): the optimum sits that far from the generator's truth
    d = R.spread(r["s12_g2o"][0], R.g2o_row(R.to_g2o(b["gt_s12"][0])))
    d0 = R.spread(R.g2o_row(R.to_g2o(b["s12"][0])), R.g2o_row(R.to_g2o(b["gt_s12"][0])))
    assert d0[0] > 1e-3 and (d < [1e-6, 1e-4, 1e-5]).all(), (d0, d)


def test_fix_scale_zero_column_and_scale_bits():
    b = _case("fix_scale")
    g = R.Pair(b, 0)
    g.err = g.errors_at(g.est)
    J = g.jacobians()
    for e in range(2):
        for r in range(2):
            assert (J[e][r][6] == 0).all() and np.abs(J[e][r][0]).max() > 0
    r = R.optimize_sim3(b)
    assert r["n_inliers"][0] >= 10
    assert r["s12"][0][12].tobytes() == np.float32(b["s12"][0][12]).tobytes()
    assert r["s12_g2o"][0][7] == float(np.float32(b["s12"][0][12]))


def test_nine_correspondences_return_zero():
    b = _case("nine")
    r = R.optimize_sim3(b)
    assert r["n_inliers"][0] == 0 and r["iterations"][0][0] > 0 and r["iterations"][0][1] == 0
    assert r["s12"].tobytes() == b["s12"].tobytes()


def test_ten_clean_correspondences_are_optimised():
    b = _case("ten")
    r = R.optimize_sim3(b)
    assert r["n_inliers"][0] == 10 and r["iterations"][0][1] == 5   # nbad == 0: optimize(5)
    assert r["s12"].tobytes() != b["s12"].tobytes()


def test_nine_survivors_return_zero_and_stay_nulled():
    b = _case("twelve_minus_three")
    r = R.optimize_sim3(b)
    assert r["n_inliers"][0] == 0 and r["iterations"][0][1] == 0 and r["s12"].tobytes() == b["s12"].tobytes()
    nulled = (r["match12"] == -1) & (b["match12"] >= 0)
    assert np.array_equal(nulled, b["outlier"])


def test_twelve_survivors_run_optimize_ten():
    """nbad > 0: the second round is optimize(10).  LM's own stop ends it at 6 here, which optimize(5) could
    not have reached."""
    b = _case("fourteen_minus_two")
    r = R.optimize_sim3(b)
    t = r["trace"][0]
    assert len(t["chi2"][0]) == 14 and np.isnan(t["chi2"][1]).all(axis=1).sum() == 2
    assert r["n_inliers"][0] == 12 and r["iterations"][0][1] > 5
    assert np.array_equal((r["match12"] == -1) & (b["match12"] >= 0), b["outlier"])
