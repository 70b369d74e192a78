"""Pins tests/initializer_ref.py, the numpy restatement of Initializer::Initialize that csrc/orbinit.hip is checked
against, on hand-built cases, shows that the sign of a singular-vector pair cannot change a result, measures the
restatement's own spread under one-ulp jitter of every H21i / H12i / F21i (JITTER; `-k margin -s` prints it) and
asserts that the GPU batch's decisions are settled at that jitter.  CPU only.

Measured (8 jitter seeds, the GPU batch at max_iterations 200):
    hyp_score   largest spread / ulp(score): see `-k margin -s`; the device gets max(16 x spread, 16 ulp)
    r21t21      rotation and |dt| / |t| spread of the returned pose; the device gets 16 x, floor 16 float ulps
    p3d         |dp| / depth spread; the device gets 16 x, floor 16 float ulps"""
import functools

import numpy as np
import pytest

import initializer_ref as R
from orb_slam2_refactored_amd.synth import make_initializer_batch

GPU_N = (0, 7, 8, 9, 63, 64, 65, 100, 128, 129, 150, 300)
GPU_SCENES = ("plane", "general", "rotation")
GPU_SEED = 14
JITTER_SEEDS = tuple(range(8))
FLOOR = 16 * 2.0 ** -23   # 16 float ulps of a quantity of size 1


@functools.lru_cache(maxsize=None)
def gpu_batch(max_iterations=200, oversized=False):
    n = list(GPU_N) + ([40] if oversized else [])
    frac = [0.1 + 0.2 * ((7 * p) % 11) / 10 for p in range(len(n))]
    return make_initializer_batch(GPU_SEED, n_corr=n, scene=GPU_SCENES, outlier_frac=frac, noise=0.3, max_iterations=max_iterations,
                                  kp1_override={len(GPU_N): 8193} if oversized else None)


@functools.lru_cache(maxsize=None)
def gpu_reference(max_iterations=200, jitter=None, oversized=False):
    return R.initialize(gpu_batch(max_iterations, oversized), jitter=jitter)


@functools.lru_cache(maxsize=None)
def jitter_spread(max_iterations=200, oversized=False):
    """The restatement's own spread over JITTER_SEEDS: score (F, 2, T) absolute, pose (rot, t) and points, each the
    largest over the batch; and whether every decision is the same at every seed."""
    base = gpu_reference(max_iterations, None, oversized)
    b = gpu_batch(max_iterations, oversized)
    score = np.zeros(base["hyp_score"].shape)
    rot = tr = pt = 0.0
    same = True
    for s in JITTER_SEEDS:
        j = gpu_reference(max_iterations, s, oversized)
        with np.errstate(invalid="ignore"):
            score = np.fmax(score, np.abs(j["hyp_score"].astype(np.float64) - base["hyp_score"].astype(np.float64)))
        for k, m in (("best_h", 0), ("best_f", 1)):   # the winner may move only among hypotheses of one set (below)
            for p in range(len(base[k])):
                if base[k][p] >= 0:
                    same &= j[k][p] >= 0 and base["set_id"][p][j[k][p]] == base["set_id"][p][base[k][p]]
                else:
                    same &= j[k][p] < 0
        for k in ("found", "model", "inlier_h", "inlier_f", "triangulated", "counted"):
            same &= np.array_equal(j[k], base[k])
        for p in np.nonzero((base["found"] == 1) & (j["found"] == 1))[0]:
            d = R.pose_distance(base["r21t21"][p], j["r21t21"][p])
            rot, tr = max(rot, d[0]), max(tr, d[1])
            k0, k1 = int(b["kp1_begin"][p]), int(b["kp1_begin"][p + 1])
            m = base["counted"][k0:k1] & j["counted"][k0:k1]
            pt = max(pt, R.point_distance(base["p3d"][k0:k1][m], j["p3d"][k0:k1][m]))
    return dict(score=score, rot=rot, t=tr, p3d=pt, same=bool(same))


def margins(max_iterations=200, oversized=False):
    """What the device is allowed: score margin (F, 2, T), (rot, t) and p3d."""
    sp = jitter_spread(max_iterations, oversized)
    base = gpu_reference(max_iterations, None, oversized)
    score = np.maximum(16 * sp["score"], 16 * R.ulp(base["hyp_score"]))
    return dict(score=score, rot=max(16 * sp["rot"], FLOOR), t=max(16 * sp["t"], FLOOR), p3d=max(16 * sp["p3d"], FLOOR))


# ---------------------------------------------------------------------------------------------------------------
def _case(scene, n=120, noise=0.0, outliers=0.0, seed=5, **kw):
    return make_initializer_batch(seed, n_corr=[n], scene=(scene,), outlier_frac=outliers, noise=noise, **kw)


def _pose_close(r, b, p=0, tol=2e-3):
    d = R.pose_distance(b["gt_r21t21"][p], r["r21t21"][p])
    return d[0] < tol and d[1] < 10 * tol


def test_exact_plane_h_wins_and_the_pose_is_recovered():
    b = _case("plane", seed=6)   # (a seed whose second-best Faugeras solution sees under 0.75 of the points)
    r = R.initialize(b)
    assert r["found"][0] == 1 and r["model"][0] == 0 and r["rh"][0] > 0.40
    assert _pose_close(r, b), R.pose_distance(b["gt_r21t21"][0], r["r21t21"][0])
    assert r["triangulated"].sum() > 100 and r["best_h"][0] >= 0


def test_general_scene_f_wins_and_the_pose_is_recovered():
    b = _case("general")
    r = R.initialize(b)
    assert r["found"][0] == 1 and r["model"][0] == 1 and r["rh"][0] <= 0.40
    assert _pose_close(r, b)
    assert (r["n_good"][0, 4:] == 0).all()
    tri = r["triangulated"].astype(bool)
    assert tri.sum() > 100 and (r["p3d"][tri, 2] > 1.5).all() and (r["p3d"][~r["counted"]] == 0).all()


def test_pure_rotation_is_rejected_by_the_parallax_rule():
    b = _case("rotation", noise=0.3, seed=6)
    r = R.initialize(b)
    assert r["found"][0] == 0 and not r["r21t21"].any() and not r["triangulated"].any()
    # not through too few points: some hypothesis triangulates nearly everything, at no parallax
    j = int(np.argmax(r["n_good"][0]))
    assert r["n_good"][0, j] > 0.9 * 100 and r["parallax"][0, j] < 1.0


def test_a_tie_of_the_two_best_motion_hypotheses_rejects():
    N = 200
    assert R.decide_f([150, 150, 3, 0], np.full(4, 5, np.float32), N, 1.0, 50) == -1
    assert R.decide_f([3, 150, 0, 150], np.full(4, 5, np.float32), N, 1.0, 50) == -1
    assert R.decide_h([150, 0, 150, 0, 0, 0, 0, 0], np.full(8, 5, np.float32), 160, 1.0, 50) == -1
    # and a unique best wins wherever the rule of the data lists it
    for order in ([190, 3, 2, 0], [0, 2, 3, 190], [2, 190, 0, 3]):
        assert R.decide_f(order, np.full(4, 5, np.float32), N, 1.0, 50) == order.index(190)
    for k in range(8):
        g = [3] * 8
        g[k] = 190
        assert R.decide_h(g, np.full(8, 5, np.float32), N, 1.0, 50) == k
    # strict > for F, >= for H at min_parallax
    assert R.decide_f([190, 0, 0, 0], np.full(4, 1, np.float32), N, 1.0, 50) == -1
    assert R.decide_h([190] + [0] * 7, np.full(8, 1, np.float32), N, 1.0, 50) == 0


def test_equal_singular_values_return_early():
    cam = np.array([500, 500, 320, 240], np.float32)
    assert R.decompose_h(np.eye(3, dtype=np.float32), cam) is None           # d1 / d2 = 1 < 1.00001
    K = R.kmat(cam)
    H = (K @ np.diag([1.000005, 1.0, 0.9]) @ np.linalg.inv(K)).astype(np.float32)
    assert R.decompose_h(H, cam) is None
    H = (K @ np.diag([1.1, 1.0, 0.9]) @ np.linalg.inv(K)).astype(np.float32)
    assert len(R.decompose_h(H, cam)) == 8


@pytest.mark.parametrize("n", [0, 7])
def test_fewer_than_eight_matches_evaluate_nothing(n):
    r = R.initialize(_case("general", n=n))
    assert r["found"][0] == 0 and not r["hyp_score"].any() and r["best_h"][0] == -1 and r["best_f"][0] == -1
    assert not r["inlier_h"].any() and not r["n_good"].any()


def test_pick8_is_the_swap_with_back_selection():
    rng = np.random.default_rng(0)
    for n in (8, 9, 15, 300):
        for _ in range(50):
            d = rng.integers(0, 2 ** 31, 8)
            idx = R.pick8(d, 2147483647, n)
            assert len(set(idx)) == 8 and all(0 <= i < n for i in idx)
    assert R.pick8([0] * 8, 2147483647, 8) == [0, 7, 6, 5, 4, 3, 2, 1]


@pytest.mark.parametrize("tag,k", [("h", 8), ("f", 8), ("f3", 0), ("f3", 2), ("e", 0), ("e", 1), ("e", 2), ("hdec", 0),
                                   ("hdec", 1), ("hdec", 2), ("tri", 3)])
def test_the_sign_of_a_singular_vector_pair_changes_nothing(tag, k):
    b = make_initializer_batch(3, n_corr=[120, 120], scene=("plane", "general"), outlier_frac=0.1, noise=0.1)
    base = R.initialize(b)
    assert (base["found"] == 1).all() and base["model"].tolist() == [0, 1]
    R.FLIP[tag] = k
    try:
        got = R.initialize(b)
    finally:
        R.FLIP.clear()
    for name in ("found", "model", "r21t21", "p3d", "triangulated"):
        assert got[name].tobytes() == base[name].tobytes(), name


def test_margin_is_measured_and_the_gpu_batch_is_settled():
    for T in (1, 64, 65, 200):
        sp, base, m = jitter_spread(T), gpu_reference(T), margins(T)
        fin = np.isfinite(base["hyp_score"])
        rel = (sp["score"][fin] / np.maximum(R.ulp(base["hyp_score"][fin]), 1e-300)).max() if fin.any() else 0
        print(f"JITTER T={T}: score spread max {sp['score'][fin].max():.3g} ({rel:.3g} ulp of the score), pose rot {sp['rot']:.3g} rad "
              f"t {sp['t']:.3g}, p3d {sp['p3d']:.3g}; found {base['found'].tolist()} model {base['model'].tolist()}")
        assert sp["same"], "found / model / masks / triangulated differ between the ends of the jitter"
        for p in range(len(GPU_N)):
            for mdl in range(2):
                best = int(base["best_h" if mdl == 0 else "best_f"][p])
                if best < 0 or T == 1:
                    continue
                s = base["hyp_score"][p, mdl].astype(np.float64)
                # Hypotheses that drew the same eight correspondences in another order are one model and tie up to
                # rounding (with N = 8 every hypothesis is that one model): the lead is over the other sets.
                others = np.nonzero(base["set_id"][p] != base["set_id"][p][best])[0]
                gap = s[best] - s[others]
                need = 2 * (m["score"][p, mdl, best] + m["score"][p, mdl, others])
                assert (gap[np.isfinite(gap)] > need[np.isfinite(gap)]).all(), (T, p, mdl, "the best score does not lead by twice the margin")
            sh, sf = float(base["score_h"][p]), float(base["score_f"][p])
            if sh + sf > 0:
                mh = float(m["score"][p, 0].max()) if base["best_h"][p] >= 0 else 0.0
                mf = float(m["score"][p, 1].max()) if base["best_f"][p] >= 0 else 0.0
                lo = (sh - mh) / ((sh - mh) + (sf + mf))
                hi = (sh + mh) / ((sh + mh) + (sf - mf))
                assert not (lo - 1e-6 <= 0.40 <= hi + 1e-6), (T, p, "RH within the margin of 0.40", lo, hi)
    base = gpu_reference(200)
    assert set(base["model"][2:].tolist()) == {0, 1} and (base["found"] == 1).any() and (base["found"][2:] == 0).any()
