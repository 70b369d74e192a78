"""LocalBA problems whose LM loops end before their iteration budget (5, 10), shared by
tests/test_ba_early_end_oracle.py (the oracle's trace: iterations, end reasons, decision margins) and
tests/test_ba_gpu.py (the device against the oracle on the same problems)."""
from collections import namedtuple

import numpy as np

from orb_slam2_refactored_amd.synth import make_ba_problem


def refeed(oracle, pr, rounds):
    """The problem LocalMapping hands over next: `rounds` oracle calls, each one's poses and points the next
    one's start; the observations and everything else stay.  Returns the problem for the next call."""
    for _ in range(rounds):
        o = oracle.local_ba(pr)
        pr = dict(pr, pose_R=o["pose_R"].copy(), pose_t=o["pose_t"].copy(), points=o["points"].copy())
    return pr


def low_noise(pr, s):
    """A make_ba_problem problem with its measurement noise (outlier offsets included) scaled by `s`: each
    observation moves towards the ground truth's projection, then back to float32 as the reference stores it."""
    R, t, X = pr["gt_R"].reshape(-1, 3, 3), pr["gt_t"], pr["gt_points"]
    ep, ek, cam = pr["edge_point"], pr["edge_pose"], pr["edge_cam"]
    Xc = np.einsum("eij,ej->ei", R[ek], X[ep]) + t[ek]
    u = cam[:, 0] * Xc[:, 0] / Xc[:, 2] + cam[:, 2]
    v = cam[:, 1] * Xc[:, 1] / Xc[:, 2] + cam[:, 3]
    clean = np.stack([u, v, u - cam[:, 4] / Xc[:, 2]], axis=1)
    obs = np.asarray(pr["edge_obs"], np.float64)
    new = clean + s * (obs - clean)
    new[obs[:, 2] < 0, 2] = -1.0   # monocular edges stay monocular
    return dict(pr, edge_obs=new.astype(np.float32).astype(np.float64))


def exact_fit_problem():
    """Every residual exactly 0.0 in fp64: identity rotations, translations / points / intrinsics chosen so
    that each projection is a short dyadic number.  b == 0, x == 0, so rho == 0 ends both loops after one
    trial and nothing moves."""
    rng = np.random.default_rng(1234)
    t = np.array([[0, 0, 0], [-1, 0, 0], [-2, 0.5, 0], [1, 0, 0]], np.float64)
    P, N = 4, 40
    fx = fy = 512.0
    cx, cy, bf = 320.0, 240.0, 64.0
    X = np.stack([0.5 * rng.integers(0, 7, N), 0.5 * rng.integers(-2, 3, N), rng.choice([4.0, 8.0, 16.0], N)], axis=1)
    ep, ek, obs, info = [], [], [], []
    for p in range(N):
        for k in range(P):
            e = len(ep)
            Xc = X[p] + t[k]
            u = fx * Xc[0] / Xc[2] + cx
            v = fy * Xc[1] / Xc[2] + cy
            ur = u - bf / Xc[2] if e % 3 == 0 else -1.0
            for val in (u, v) + ((ur,) if ur >= 0 else ()):
                assert val >= 0 and float(np.float32(val)) == val, (p, k, val)
            assert e % 3 != 0 or ur >= 0
            ep.append(p)
            ek.append(k)
            obs.append([u, v, ur])
            info.append(1.0 if rng.integers(0, 2) else 0.25)
    E = len(ep)
    return dict(pose_R=np.tile(np.eye(3).reshape(-1), (P, 1)), pose_t=t.copy(),
                pose_fixed=np.array([1, 0, 0, 1], np.uint8), points=X.copy(),
                edge_point=np.array(ep, np.int32), edge_pose=np.array(ek, np.int32),
                edge_obs=np.array(obs, np.float64), edge_inv_sigma2=np.array(info, np.float64),
                edge_cam=np.tile(np.array([fx, fy, cx, cy, bf]), (E, 1)))


def one_bad_observation(pr, edge=5, du=3.0):
    """The exact-fit problem with `du` px added to the u of one observation: a single residual to spread."""
    obs = np.array(pr["edge_obs"], np.float64)
    obs[edge, 0] += du
    return dict(pr, edge_obs=obs)


# kind "synth": args = (seed, n_kf, n_pts, n_fixed, outlier_frac[, noise scale for low_noise]), re-fed `rounds`
# times; "exact": exact_fit_problem(); "one_bad": args = (edge, du) on the exact-fit problem, re-fed `rounds` times.
# iterations / reasons are the oracle's, per loop, as literals from a CPU run (tests/test_ba_early_end_oracle.py
# holds the oracle to them and to the decision margins that make a device comparison meaningful).
Case = namedtuple("Case", "id kind args rounds iterations reasons")

# What the table covers, and what a bounded CPU search (oracle traces; about 1500 runs: re-fed make_ba_problem
# windows of 5 .. 24 keyframes with the noise scaled by 1 .. 0, started perturbed and at the ground truth, up to 8
# re-feeds; the one-bad-observation problem over 23 edges x 5 offsets x 3 re-feeds) found for the rest:
#   * second loop ended by nbad at 5 .. 8 of 10 iterations: re-fed windows at the generator's noise;
#     23 free keyframes (ba_solve_global_kernel) in large-*; no fixed camera but keyframe 0 in *-nofix.
#   * nbad reset inside a loop that then still ends early (bad, bad, good, bad, bad, bad): refeed-5kf-reset;
#     without the reset the second loop would end after 6 iterations instead of 8.
#   * a first loop shorter than 5: not with the generator's noise (lambda is re-initialised per call and the
#     first Huber steps keep gaining more than 0.1 %), but at a tenth of it (lownoise-*, (3, 3): the minimum
#     in both loops) and on the one-bad-observation problem ((4, 3), re-fed (3, 3)).
#   * rho == 0: the exact-fit problem, (1, 1), nothing moves.
#   * q == 10: seen only on problems re-fed to convergence (one-bad after 2 .. 3 re-feeds, noise-free windows
#     started at the ground truth after 6), where every |cur - tmp| is 1e-14 .. 1e-15 of cur: rounding level,
#     the GPU's and the oracle's decisions are not comparable there.  No case.
EARLY_END_CASES = [
    Case("refeed-5kf", "synth", (40, 5, 120, 1, 0.0), 1, (5, 5), ("budget", "nbad")),
    Case("refeed-8kf", "synth", (51, 8, 600, 1, 0.0), 1, (5, 6), ("budget", "nbad")),
    Case("refeed-6kf-outliers", "synth", (41, 6, 300, 1, 0.03), 1, (5, 7), ("budget", "nbad")),
    Case("refeed-large", "synth", (54, 24, 1500, 2, 0.0), 1, (5, 6), ("budget", "nbad")),
    Case("refeed-large-outliers", "synth", (53, 24, 1500, 2, 0.03), 2, (5, 7), ("budget", "nbad")),
    Case("refeed-8kf-nofix", "synth", (56, 8, 600, 0, 0.0), 1, (5, 6), ("budget", "nbad")),
    Case("refeed-5kf-reset", "synth", (70, 5, 120, 1, 0.0), 3, (5, 8), ("budget", "nbad")),
    Case("lownoise-5kf", "synth", (60, 5, 120, 1, 0.0, 0.1), 1, (3, 3), ("nbad", "nbad")),
    Case("lownoise-large", "synth", (64, 24, 1500, 2, 0.0, 0.1), 1, (3, 3), ("nbad", "nbad")),
    Case("lownoise-8kf-nofix", "synth", (66, 8, 600, 0, 0.0, 0.1), 1, (3, 3), ("nbad", "nbad")),
    Case("exact-fit", "exact", (), 0, (1, 1), ("rho0", "rho0")),
    Case("one-bad", "one_bad", (5, 3.0), 0, (5, 3), ("budget", "nbad")),
    Case("one-bad-133", "one_bad", (133, 3.0), 0, (4, 3), ("nbad", "nbad")),
    Case("one-bad-133-refed", "one_bad", (133, 3.0), 1, (3, 3), ("nbad", "nbad")),
]
CASE_IDS = [c.id for c in EARLY_END_CASES]
REFED_CASES = [c for c in EARLY_END_CASES if c.rounds > 0]

_built = {}


def build_case(oracle, case):
    """The case's problem (built once per process and shared: treat it as read-only)."""
    if case.id not in _built:
        if case.kind == "synth":
            seed, kf, pts, fixed, outl = case.args[:5]
            pr = make_ba_problem(seed, n_kf=kf, n_pts=pts, n_fixed=fixed, outlier_frac=outl)
            if len(case.args) > 5:
                pr = low_noise(pr, case.args[5])
        elif case.kind == "exact":
            pr = exact_fit_problem()
        else:
            pr = one_bad_observation(exact_fit_problem(), *case.args)
        _built[case.id] = refeed(oracle, pr, case.rounds)
    return _built[case.id]


_traced = {}


def oracle_result(oracle, case):
    """The oracle's traced result on the case (computed once per process and shared)."""
    if case.id not in _traced:
        _traced[case.id] = oracle.local_ba(build_case(oracle, case), trace=True)
    return _traced[case.id]
