"""Pins tests/essential_graph_ref.py, the restatement of Optimizer::OptimizeEssentialGraph that
tests/test_essential_graph_gpu.py holds the device to: log against exp in each of log's four branches, a consistent
graph, the numeric Jacobian against a coarser difference, fix_scale, an edgeless and the fixed vertex, the edge-list
rules of Optimizer.cc:798-903 one by one, and the GPU cases: each keeps its iteration count and accept sequence under
every jitter seed (a case that does not is replaced here, never skipped), and 16 x the spread of the restatement's own
result under that jitter is the GPU tolerance.  CPU only."""
import functools

import numpy as np
import pytest

import essential_graph_ref as R
import optsim3_ref as S
from essential_graph_cases import make_graph

JITTER_SEEDS = (1, 2, 3, 4)
# name -> make_graph arguments.  D = 7 x (active free vertices) takes 7, 14, 35, 84 (one 16-block short), 273 (not a
# multiple of 16) and more; the solve has one form.  loop6_all_20 runs optimize(20) to its limit, every trial
# accepted: a scale of 8 that fix_scale forbids the vertices to take up, over 120 degrees.
CASES = {
    "kf2_one_edge": dict(seed=1, n_kf=2, n_corrected=1, loop=False),
    "kf3_fixed_middle": dict(seed=1, n_kf=3, n_corrected=1, fixed_slot=1),
    "chain13": dict(seed=1, n_kf=13, n_corrected=2, n_points=40),
    "chain13_fix_scale": dict(seed=2, n_kf=13, n_corrected=2, fix_scale=1, n_points=40),
    "chain13_large_loop": dict(seed=1, n_kf=13, n_corrected=3, corr_deg=40., corr_t=3., corr_s=2.0),
    "chain40_covis_points": dict(seed=1, n_kf=40, n_corrected=4, covis=3, n_points=300, skip_every=7, step_deg=4.),
    "loop6_all_20": dict(seed=0, n_kf=6, n_corrected=1, corr_deg=120., corr_t=3., corr_s=8.0, fix_scale=1, step_deg=30., covis=2),
    "chain12_edgeless": dict(seed=3, n_kf=12, n_corrected=2, isolated=(5,), n_points=30, skip_every=4),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return make_graph(**CASES[name])


@functools.lru_cache(maxsize=None)
def reference(name):
    return R.optimize_essential_graph(case(name))


@functools.lru_cache(maxsize=None)
def jitter_study(name):
    """(seeds under which the iteration count or the accept sequence moved, spread of sim3_g2o over the seeds)."""
    base = reference(name)
    bad, sp = [], np.zeros(3)
    for s in JITTER_SEEDS:
        j = R.optimize_essential_graph(case(name), jitter_seed=s)
        if j["iterations"] != base["iterations"] or list(j["accept"]) != list(base["accept"]):
            bad.append(s)
        sp = np.maximum(sp, R.spread(base["sim3_g2o"], j["sim3_g2o"]))
    return bad, sp


def tolerance(name):
    return 16 * jitter_study(name)[1]


# Two keyframes and one edge have as many equations as unknowns: the error goes to 0 exactly and the last trial's rho
# is rounding noise around 0.  With fix_scale and a scale the vertices cannot take up, the residual is sigma alone, a
# constant the unknowns do not reach: the other components still go to 0 and rho ends at exactly 0, which the jitter
# (a fresh factor on sigma at every evaluation) turns into noise as well.  No seed of 48 tried (either fix_scale,
# corrections up to 150 degrees and a scale of 8) keeps its accept sequence under jitter.  The issue lists the case, so
# it stays in the GPU list, held to the same assertions; it cannot be admitted by the rule below.
UNSTABLE_BY_CONSTRUCTION = ("kf2_one_edge",)


@pytest.mark.parametrize("name", sorted(set(CASES) - set(UNSTABLE_BY_CONSTRUCTION)))
def test_gpu_cases_are_stable_under_jitter(name):
    bad, sp = jitter_study(name)
    r = reference(name)
    print(name, "iterations", r["iterations"], "accept", "".join("1" if a else "0" for a in r["accept"]), "spread", sp)
    assert not bad, (name, bad)


def test_gpu_cases_cover_the_endings():
    runs = {n: reference(n) for n in CASES}
    assert any(not r["accept"].all() for r in runs.values()), "no case with a rejected trial"
    assert any(r["iterations"] < R.MAX_ITERATIONS for r in runs.values())
    assert any(r["iterations"] == R.MAX_ITERATIONS for r in runs.values()), "no case that runs all 20 iterations"
    assert runs["loop6_all_20"]["accept"].all() and runs["loop6_all_20"]["trials"] == R.MAX_ITERATIONS
    assert reference("chain12_edgeless")["sim3_g2o"][5].tobytes() == S.g2o_row(S.to_g2o(case("chain12_edgeless")["vertex_sim3"][5])).tobytes()


def _u(omega, ups, sigma):
    return list(omega) + list(ups) + [sigma]


@pytest.mark.parametrize("u", [_u([3e-6, -2e-6, 1e-6], [0.3, -0.2, 0.1], 2e-6),      # |sigma| < eps, d > 1 - eps
                               _u([0.3, -0.5, 0.2], [0.3, -0.2, 0.1], -3e-6),        # |sigma| < eps, rotation
                               _u([2e-6, 1e-6, -3e-6], [1.0, 2.0, -0.5], 0.4),       # scale, d > 1 - eps
                               _u([-0.7, 0.4, 1.1], [1.0, 2.0, -0.5], -0.6)])        # scale and rotation
def test_log_inverts_exp_in_each_branch(u):
    a = S.sim3_exp(u)
    want = (abs(u[6]) < R.EPS, np.linalg.norm(u[:3]) < 1e-3)
    assert R.log_branch(a) == want
    got = np.array(R.sim3_log(a))
    # the small-angle branch takes omega = deltaR / 2, exact to theta^2 / 6 relative
    tol = 1e-9 * max(1.0, np.abs(u).max()) if not want[1] else 1e-10
    assert np.abs(got - np.array(u)).max() < tol, (got, u)


def test_consistent_graph_has_zero_error_and_ends_early():
    g = make_graph(1, n_kf=8, n_corrected=0)
    G = R.Graph(g)
    assert R.Graph.chi2_of(G.errors()) < 1e-10   # float measurements of float poses: 1e-7 per component at most
    r = R.optimize_essential_graph(g)
    assert r["iterations"] < R.MAX_ITERATIONS and r["chi2"] < 1e-10
    # the poses barely move
    assert R.spread(r["sim3_g2o"], np.array([S.g2o_row(S.to_g2o(v)) for v in g["vertex_sim3"]])).max() < 1e-5


def test_numeric_jacobian_agrees_with_a_coarser_difference():
    g = case("chain13")
    G = R.Graph(g)
    J = G.jacobians()
    h = 1e-6
    for a in range(2):
        ends = G.ei if a == 0 else G.ej
        for d in range(7):
            u = [0.0] * 7
            u[d] = h
            plus = G.errors(moved=(a, [R.oplus(G.est[v], u, False) for v in ends]))
            u[d] = -h
            minus = G.errors(moved=(a, [R.oplus(G.est[v], u, False) for v in ends]))
            coarse = (plus - minus) / (2 * h)
            # delta = 1e-9 carries 2^-53 / 1e-9 ~ 1e-7 of rounding per unit of error, the coarse one h^2 of curvature
            assert np.abs(J[:, a, :, d] - coarse).max() < 5e-6 * max(1.0, np.abs(coarse).max())


def test_fix_scale_leaves_every_scale_bit_equal():
    g = case("chain13_fix_scale")
    r = reference("chain13_fix_scale")
    assert r["iterations"] > 1
    for v in range(len(g["vertex_sim3"])):
        assert r["sim3_g2o"][v][7] == float(np.float32(g["vertex_sim3"][v][12]))
    J = R.Graph(g).jacobians()
    assert not J[:, :, :, 6].any()   # the scale column of every Jacobian is exactly zero


def test_fixed_and_edgeless_vertices_are_untouched():
    g = case("chain12_edgeless")
    r = reference("chain12_edgeless")
    for v in (g["fixed_slot"], 5):
        assert r["sim3_g2o"][v].tobytes() == S.g2o_row(S.to_g2o(g["vertex_sim3"][v])).tobytes()
    moved = [v for v in range(12) if r["sim3_g2o"][v].tobytes() != S.g2o_row(S.to_g2o(g["vertex_sim3"][v])).tobytes()]
    assert len(moved) == 10
    # skipped points stay, the others follow their reference keyframe
    skip = g["point_ref"] < 0
    assert skip.any() and np.array_equal(r["points"][skip], g["points"][skip])
    assert (r["points"][~skip] != g["points"][~skip]).any()


def test_point_correction_is_the_matrix_algebra():
    g = case("chain13")
    r = reference("chain13")
    for p in range(len(g["points"])):
        k = g["point_ref"][p]
        Mw = np.linalg.inv(S.sim3_matrix(tuple([list(r["sim3_g2o"][k][:4]), list(r["sim3_g2o"][k][4:7]), r["sim3_g2o"][k][7]])))
        M = Mw @ S.sim3_matrix(S.to_g2o(g["vertex_sim3"][k]))
        want = (M @ np.append(g["points"][p].astype(np.float64), 1.0))[:3]
        assert np.abs(r["points"][p] - want).max() < 1e-4 * max(1.0, np.abs(want).max())


# ---------------------------------------------------------------- the edge list (Optimizer.cc:798-903), by hand
def _tables(**kw):
    t = dict(kf_id=[0, 1, 2, 3, 4], parent=[-1, 0, 1, 2, 3], loop_edges=[[], [], [], [], []],
             covisibles=[[], [], [], [], []], loop_connections=[], curr_slot=4, loop_slot=0)
    t.update(kw)
    return t


def _edges(t):
    ei, ej, et = R.build_edges(t)
    return list(zip(ei.tolist(), ej.tolist(), et.tolist()))


TREE = [(1, 0, 1), (2, 1, 1), (3, 2, 1), (4, 3, 1)]
EDGE_CASES = {
    "spanning tree only": (_tables(), TREE),
    "loop connection kept for (curr, loop) whatever its weight": (_tables(loop_connections=[(4, [0, 1])]), [(4, 0, 0)] + TREE),
    "loop connection kept at weight 100": (_tables(loop_connections=[(4, [1])], covisibles=[[], [], [], [], [(1, 100)]]),
                                           [(4, 1, 0)] + TREE),
    "loop connection dropped at weight 99": (_tables(loop_connections=[(3, [0])], covisibles=[[], [], [], [(0, 99)], []]), TREE),
    "loop edge to an older keyframe only": (_tables(loop_edges=[[3], [], [], [0], []]), TREE[:3] + [(3, 0, 1)] + TREE[3:]),
    "covisibility edge at weight 100, not at 99": (_tables(covisibles=[[], [], [(0, 100)], [(0, 99)], []]),
                                                  TREE[:2] + [(2, 0, 1)] + TREE[2:]),
    "covisible parent excluded": (_tables(covisibles=[[], [(0, 150)], [], [], []]), TREE),
    "covisible child excluded": (_tables(parent=[-1, 0, 1, 2, 1], kf_id=[0, 9, 2, 3, 4], covisibles=[[], [(4, 150)], [], [], []]),
                                 [(1, 0, 1), (2, 1, 1), (3, 2, 1), (4, 1, 1)]),
    "covisible loop edge excluded": (_tables(loop_edges=[[], [], [], [0], []], covisibles=[[], [], [], [(0, 150)], []]),
                                     TREE[:3] + [(3, 0, 1)] + TREE[3:]),
    "covisible bad keyframe excluded": (_tables(covisibles=[[], [], [], [(-1, 150)], []]), TREE),
    "covisible newer keyframe excluded": (_tables(covisibles=[[(3, 150)], [], [], [], []]), TREE),
    "covisible pair already a loop connection excluded": (_tables(loop_connections=[(1, [3])], covisibles=[[], [(3, 150)], [], [(1, 150)], []]),
                                                          [(1, 3, 0)] + TREE),
    "covisibility order is the row's": (_tables(covisibles=[[], [], [], [], [(1, 300), (0, 200), (2, 100)]]),
                                        TREE + [(4, 1, 1), (4, 0, 1), (4, 2, 1)]),
}


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_edge_list_rules(name):
    t, want = EDGE_CASES[name]
    assert _edges(t) == want
