"""The oracle on the early-end table (tests/ba_cases.py): its iteration counts and end reasons are the table's
literals, and every accept / reject and relative-improvement decision on the way is far from rounding, which
is what makes comparing the device's decisions with the oracle's meaningful (tests/test_ba_gpu.py).  Also: the
per-trial trace changes no result."""
import numpy as np
import pytest

from ba_cases import CASE_IDS, EARLY_END_CASES, build_case, exact_fit_problem, oracle_result, refeed
from orb_slam2_refactored_amd.synth import make_ba_problem

# A fixed-order fp64 sum over <= 12k edges differs between two orders by about n * eps = 1.3e-12 relative:
# three and six orders below these.
MARGIN_TRIAL = 1e-9   # |cur - tmp| >= MARGIN_TRIAL * cur on every trial with rho != 0
MARGIN_NBAD = 1e-6    # |(ini - cur) * 1e3 - ini| >= MARGIN_NBAD * ini wherever the nbad test is reached


@pytest.mark.parametrize("case", EARLY_END_CASES, ids=CASE_IDS)
def test_early_end_case_on_oracle(oracle, case):
    o = oracle_result(oracle, case)
    tr = o["trace"]
    assert tuple(o["iterations"]) == case.iterations
    assert o["end_reason"] == case.reasons
    assert case.iterations[0] < 5 or case.iterations[1] < 10
    for lp in (0, 1):   # the trace agrees with the counts it explains
        t = tr[tr["loop"] == lp]
        assert int(t["iter_end"].sum()) == case.iterations[lp]
        assert t["loop_end"][-1] != 0 and not t["loop_end"][:-1].any()
    if case.kind == "exact":
        assert len(tr) == 2
        for r in tr:
            assert r["cur"] == 0.0 and r["tmp"] == 0.0 and r["rho"] == 0.0 and not r["accepted"]
        assert o["chi2"] == (0.0, 0.0)
        pr = build_case(oracle, case)
        for k in ("pose_R", "pose_t", "points"):
            assert np.array_equal(o[k], pr[k]), k
        return
    assert (tr["rho"] != 0).all()
    for r in tr:
        assert abs(r["cur"] - r["tmp"]) >= MARGIN_TRIAL * r["cur"], (r["loop"], r["it"], r["q"])
    for r in tr[tr["nbad_tested"] == 1]:
        assert abs((r["ini"] - r["cur_end"]) * 1e3 - r["ini"]) >= MARGIN_NBAD * r["ini"], (r["loop"], r["it"])


def test_table_covers_what_it_claims(oracle):
    by_id = {c.id: c for c in EARLY_END_CASES}
    free = lambda c: int((build_case(oracle, c)["pose_fixed"] == 0).sum())
    nbad2 = [c for c in EARLY_END_CASES if c.rounds > 0 and c.kind == "synth" and c.reasons[1] == "nbad"]
    assert any(free(c) <= 8 for c in nbad2) and any(free(c) > 21 for c in nbad2)
    assert any(3 in c.iterations for c in EARLY_END_CASES)
    assert by_id["exact-fit"].reasons == ("rho0", "rho0")
    assert any(c.rounds > 0 and c.kind == "synth" and c.args[3] == 0 for c in EARLY_END_CASES)
    assert all(c.rounds <= 3 for c in EARLY_END_CASES)
    # refeed-5kf-reset: nbad goes 1, 2, 0 and then 1, 2, 3 inside the second loop
    t = oracle_result(oracle, by_id["refeed-5kf-reset"])["trace"]
    t = t[(t["loop"] == 1) & (t["nbad_tested"] == 1)]
    assert t["nbad"].tolist()[-6:] == [1, 2, 0, 1, 2, 3]


@pytest.mark.parametrize("seed,kf,pts,fixed", [(3, 5, 200, 1), (2, 12, 1500, 0)])
def test_trace_changes_nothing(oracle, seed, kf, pts, fixed):
    pr = make_ba_problem(seed, n_kf=kf, n_pts=pts, n_fixed=fixed)
    a = oracle.local_ba(pr)
    b = oracle.local_ba(pr, trace=True)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert b["end_reason"] == ("budget", "budget") and len(b["trace"]) >= 15
    for after in (3, 7):
        a = oracle.local_ba(pr, stop_after=after)
        b = oracle.local_ba(pr, stop_after=after, trace=True)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        assert len(b["trace"]) == after and "stop" in b["end_reason"]


def test_refeed_keeps_the_observations(oracle):
    pr = make_ba_problem(40, n_kf=5, n_pts=120, n_fixed=1, outlier_frac=0.0)
    nxt = refeed(oracle, pr, 2)
    for k in pr:
        same = np.array_equal(np.asarray(pr[k]), np.asarray(nxt[k]))
        assert same == (k not in ("pose_R", "pose_t", "points")), k
    o = oracle.local_ba(refeed(oracle, pr, 1))
    for k in ("pose_R", "pose_t", "points"):
        assert np.array_equal(nxt[k], o[k]), k


def test_exact_fit_recipe():
    pr = exact_fit_problem()
    assert len(pr["pose_t"]) == 4 and pr["pose_fixed"].tolist() == [1, 0, 0, 1]
    assert len(pr["points"]) == 40 and len(pr["edge_point"]) == 160
    assert set(pr["points"][:, 2]) <= {4.0, 8.0, 16.0} and not (pr["points"][:, :2] % 0.5).any()
    st = pr["edge_obs"][:, 2] >= 0
    assert np.array_equal(st, np.arange(160) % 3 == 0)
    assert set(pr["edge_inv_sigma2"]) == {1.0, 0.25}
