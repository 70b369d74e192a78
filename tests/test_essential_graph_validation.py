"""OptimizeEssentialGraph's argument checks: every ORB_EINVAL path of the host entry, each refused before any device
call (the tests run without a GPU), the device entry's checks of sizes and pointers through the C-ABI, the edge-list
helper against the restatement and its own refusals, and the C++ wrapper's compile check."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import essential_graph_ref as R
from essential_graph_cases import make_graph
from orb_slam2_refactored_amd._lib import EssentialGraph, EssentialGraphResult, OrbError, lib
from orb_slam2_refactored_amd.optimizer import EG_MAX_KEYFRAMES, OptimizeEssentialGraph, essential_graph_edges
from test_essential_graph_ref import EDGE_CASES

ROOT = Path(__file__).resolve().parents[1]


def _g(**kw):
    return make_graph(1, n_kf=6, n_corrected=1, n_points=5, **kw)


def _set(g, key, idx, value):
    a = np.array(g[key]).copy()
    a[idx] = value
    return dict(g, **{key: a})


BAD = {
    "edge_i == edge_j": lambda g: _set(g, "edge_j", 1, int(g["edge_i"][1])),
    "edge index out of range": lambda g: _set(g, "edge_i", 0, 6),
    "edge index out of range ": lambda g: _set(g, "edge_j", 2, -1),
    "fixed_slot out of range": lambda g: dict(g, fixed_slot=6),
    "fixed_slot out of range ": lambda g: dict(g, fixed_slot=-1),
    "scale must be positive": lambda g: _set(g, "vertex_sim3", (2, 12), 0.0),
    "scale must be positive ": lambda g: _set(g, "edge_sim3", (3, 12), -1.0),
    "non-finite Sim3": lambda g: _set(g, "vertex_sim3", (1, 4), np.nan),
    "non-finite Sim3 ": lambda g: _set(g, "edge_sim3", (1, 10), np.inf),
    "non-finite point": lambda g: _set(g, "points", (0, 1), np.inf),
    "point_ref out of range": lambda g: _set(g, "point_ref", 0, 6),
    "point_ref out of range ": lambda g: _set(g, "point_ref", 1, -2),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_host_entry_refuses(what):
    with pytest.raises(OrbError, match=what.strip()):
        OptimizeEssentialGraph(BAD[what](_g()))


def test_too_many_keyframes_and_short_arrays():
    n = EG_MAX_KEYFRAMES + 1
    big = dict(_g(), vertex_sim3=np.tile(_g()["vertex_sim3"][:1], (n, 1)), edge_sim3=np.tile(_g()["edge_sim3"][:1], (n, 1)))
    with pytest.raises(OrbError, match="ORBBA_EG_MAX_KEYFRAMES"):
        OptimizeEssentialGraph(big)
    with pytest.raises(ValueError, match="edge_sim3"):
        OptimizeEssentialGraph(dict(_g(), edge_sim3=_g()["edge_sim3"][:3]))
    with pytest.raises(ValueError, match="edge_table"):
        OptimizeEssentialGraph(dict(_g(), edge_table=_g()["edge_table"][:2]))
    with pytest.raises(ValueError, match="points"):
        OptimizeEssentialGraph(dict(_g(), points=None))


def test_null_pointers_and_sizes_through_the_c_abi():
    l = lib()
    eg, res = EssentialGraph(), EssentialGraphResult()
    for fn in (l.orbba_optimize_essential_graph, ):
        assert fn(None, C.byref(res), 0) != 0 and fn(C.byref(eg), None, 0) != 0
        eg.n_keyframes = 0
        assert fn(C.byref(eg), C.byref(res), 0) != 0 and b"n_keyframes" in l.orb_last_error()
        eg.n_keyframes = 2
        assert fn(C.byref(eg), C.byref(res), 0) != 0 and b"null" in l.orb_last_error()
    assert l.orbba_optimize_essential_graph_device(C.byref(eg), C.byref(res), None) != 0 and b"null" in l.orb_last_error()
    eg.fixed_slot = 2
    assert l.orbba_optimize_essential_graph_device(C.byref(eg), C.byref(res), None) != 0 and b"fixed_slot" in l.orb_last_error()
    assert l.orbba_essential_graph_profile(C.byref(eg), C.byref(res), 0, None) != 0


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_edge_list_helper_follows_the_rules(name):
    t, want = EDGE_CASES[name]
    ei, ej, et = essential_graph_edges(t)
    assert list(zip(ei.tolist(), ej.tolist(), et.tolist())) == want


def test_edge_list_helper_on_a_random_graph_and_its_refusals():
    rng = np.random.default_rng(3)
    V = 30
    t = dict(kf_id=list(rng.permutation(100)[:V]), parent=[-1] + [int(rng.integers(0, k)) for k in range(1, V)],
             loop_edges=[list(rng.choice(V - 1, rng.integers(0, 3), replace=False)) for _ in range(V)],
             covisibles=[], loop_connections=[(V - 1, [0, 3, 7]), (V - 2, [1, 3])], curr_slot=V - 1, loop_slot=0)
    for k in range(V):
        t["loop_edges"][k] = [int(l) if l < k else int(l) + 1 for l in t["loop_edges"][k]]
        others = [int(o) for o in rng.permutation(V) if o != k][:8]
        t["covisibles"].append([(o if rng.random() > 0.1 else -1, int(w)) for o, w in zip(others, sorted(rng.integers(60, 200, 8), reverse=True))])
    ei, ej, et = essential_graph_edges(t)
    ri, rj, rt = R.build_edges(t)
    assert len(ei) > V and np.array_equal(ei, ri) and np.array_equal(ej, rj) and np.array_equal(et, rt)
    with pytest.raises(OrbError, match="parent"):
        essential_graph_edges(dict(t, parent=[V] + t["parent"][1:]))
    with pytest.raises(OrbError, match="covisibility"):
        essential_graph_edges(dict(t, covisibles=[[(V, 100)]] + t["covisibles"][1:]))
    with pytest.raises(OrbError, match="curr_slot"):
        essential_graph_edges(dict(t, curr_slot=V))


def test_cpp_wrapper_compiles(tmp_path):
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", f"-I{ROOT / 'include'}", "-c",
                    str(ROOT / "tests" / "native" / "essential_graph_wrapper_use.cpp"), "-o", str(tmp_path / "w.o")], check=True)
