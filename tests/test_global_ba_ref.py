"""tests/global_ba_ref.py pinned: the LM restatement against the CPU oracle, the map update against hand-built cases.

Oracle: under RULE_LOCAL, robust, optimize(5), BundleAdjustment is LocalBA's first loop, so the restatement must equal
oracle.local_ba(stop_after=T) with T the first loop's trial count (the flag goes up right after loop 1's last trial and
the oracle returns the state after optimize(5)).  Iterations and the accept sequence are identical; poses and points
lie within 16 x the restatement's own spread under one-ulp jitter of its error evaluations (the project's convention,
tests/essential_graph_ref.py).  Seeds whose accept sequence is the same under every jitter draw (checked below):
(3: 5 KF, 200 points, 1 fixed) and (2: 8 KF, 400 points, 0 fixed, stereo_frac 0.2).  CPU only."""
import numpy as np
import pytest

import global_ba_cases as GC
import global_ba_ref as G
import oracle_api as O
from orb_slam2_refactored_amd.synth import make_ba_problem

ORACLE_CASES = {3: dict(n_kf=5, n_pts=200, n_fixed=1), 2: dict(n_kf=8, n_pts=400, n_fixed=0, stereo_frac=0.2)}


@pytest.mark.parametrize("seed", sorted(ORACLE_CASES))
def test_restatement_equals_the_oracles_first_loop(seed):
    pr = make_ba_problem(seed, **ORACLE_CASES[seed])
    tr = O.local_ba(pr, trace=True)
    T = int((tr["trace"]["loop"] == 0).sum())
    o = O.local_ba(pr, stop_after=T)
    kw = dict(n_iterations=5, robust=True, stereo_rule=G.RULE_LOCAL)
    r = G.bundle_adjustment(pr, **kw)
    dp, dx, same = G.jitter_spread(pr, draws=4, **kw)
    assert same, "the accept sequence depends on the jitter draw: not a seed to pin on"
    assert r["iterations"] == o["iterations"][0] and r["trials"] == T
    assert np.array_equal(r["accept"], tr["trace"]["accepted"][:T] != 0)
    ep, ex = G.rmse(r["pose_t"], o["pose_t"]), G.rmse(r["points"], o["points"])
    eq = G.rmse(r["pose_q"], o["pose_q"])
    print(f"seed {seed}: pose_t {ep:.3g} (spread {dp:.3g}), points {ex:.3g} (spread {dx:.3g}), pose_q {eq:.3g}")
    assert dp > 0 and dx > 0
    assert ep <= 16 * dp and eq <= 16 * dp and ex <= 16 * dx
    assert abs(r["chi2"] - o["chi2"][0]) <= 1e-9 * o["chi2"][0]


def test_schedule_and_rules():
    pr = make_ba_problem(3, n_kf=5, n_pts=200, n_fixed=1)
    z = G.bundle_adjustment(pr, 0)
    assert z["iterations"] == 0 and z["trials"] == 0 and np.array_equal(z["points"], np.asarray(pr["points"], np.float64))
    obs = np.array(pr["edge_obs"], np.float64).reshape(-1, 3)
    obs[:3, 2] = 0.0
    loc, ref = G.edge_types(obs, G.RULE_LOCAL), G.edge_types(obs, G.RULE_REFERENCE)
    assert ref[:3].all() and not ref[3:].any()            # `if (ur)`: only ur == 0 is a stereo edge
    assert np.array_equal(loc, (obs[:, 2] >= 0).astype(np.uint8))


def test_update_hand_built_cases():
    m = GC.hand_case()
    o = G.update_map(m)
    E, RZ, RZT = GC.EYE, GC.RZ, GC.RZT
    # 1 is not in the adjustment: (T1 * T0^-1) * TcwGBA0, T0^-1 = (Rz^T, (-2, 1, -3)), T1 * T0^-1 = (Rz^T, (2, 6, 3))
    assert o["kf_pose_gba"][1].tolist() == RZT + [22, -4, 33]
    assert o["kf_pose_gba"][2].tolist() == E + [7, 8, 9]                 # in the adjustment: kept
    # 3: T2^-1 from the OLD pose of 2 = (I, (-1, -1, -1)); T3 * T2^-1 = (Rz, (1, -1, -1)); times TcwGBA2
    assert o["kf_pose_gba"][3].tolist() == RZ + [-7, 6, 8]
    assert o["kf_in_gba"].tolist() == [1, 1, 1, 1, 1, 0]
    for k in range(4):   # visited: bef = old pose, pose = TcwGBA
        assert np.array_equal(o["kf_pose_bef"][k], m["kf_pose"][k]) and np.array_equal(o["kf_pose"][k], o["kf_pose_gba"][k])
    for k in (4, 5):     # never reached: all three rows kept, the stale bef too
        for a in ("kf_pose", "kf_pose_gba", "kf_pose_bef"):
            assert np.array_equal(o[a][k], m[a][k])
    x = o["mp_xw"].tolist()
    assert x[0] == [2, 1, -4]        # reference 4, unreachable but flagged: stale bef (I, (1, 0, 0)), pose (I, (0, 0, 5))
    assert x[1] == [2, 2, 2]         # reference 5 is unflagged
    assert x[2] == [3, 3, 3]         # bad
    assert x[3] == [5, 6, 7]         # in the adjustment
    assert x[4] == [-9, -17, -27]    # reference 1: Xc = (5, 5, 6) by its old pose; back by (Rz^T, (22, -4, 33))^-1
    assert x[5] == [1, 0, -5]


def test_update_big_case_is_order_independent():
    """A child depends on its parent alone: walking the big table's levels in reverse slot order gives the queue's
    result bit for bit (what the device's level-synchronous walk relies on)."""
    m = GC.big_case()
    o = G.update_map(m)
    m2 = dict(m)
    off, idx = m["kf_child_off"], m["kf_child_idx"].copy()
    for k in range(len(off) - 1):
        idx[off[k]:off[k + 1]] = idx[off[k]:off[k + 1]][::-1]
    m2["kf_child_idx"] = idx
    assert GC.same_bits(o, G.update_map(m2))
    assert o["kf_in_gba"][:370].all() and o["kf_in_gba"][390:].all()
    assert np.array_equal(o["kf_in_gba"][371:390], m["kf_in_gba"][371:390])
    moved = (o["mp_xw"] != m["mp_xw"]).any(axis=1)
    assert 0 < moved.sum() < len(moved)
