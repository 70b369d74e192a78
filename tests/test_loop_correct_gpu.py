"""Loop correction on the GPU (orblc_*, orbba_essential_graph_edges_device; orb_slam2_refactored_amd/loop_correction.py)
against the restatement tests/loop_correct_ref.py: every table and every output identical, floats compared as bits, no
tolerance anywhere; max_connected = conn_cap + 1 against n_connected; the dirty maps through the device entries; a rerun;
the device edge list against the host one at three capacities; and the chain on one stream into
optimize_essential_graph_device with n_edges = capacity against the host optimisation of the restatement's tables.

The chain runs update_connections(cur) -> connected -> propagate -> update_connections(connected) -> fuse_apply (the
matched points: AddObservation into holes of cur's row and Replace on occupied keypoints) -> loop connections -> covis_csr
-> edges -> optimize_essential_graph_device on the chain map, whose observation rows keep free entries; the restatement side
is loop_correct_ref.py with observe_ref.fuse_apply between."""
import numpy as np
import pytest

import loop_correct_cases as LC
import loop_correct_ref as LR
import map_maintenance_ref as R
import observe_ref as OR
from orb_slam2_refactored_amd import loop_correction as L
from orb_slam2_refactored_amd import map_maintenance as MM
from orb_slam2_refactored_amd import observations as OBS
from orb_slam2_refactored_amd import optimizer

pytestmark = pytest.mark.gpu

MIN_WEIGHT = 20          # the small map's weights lie on both sides of it
LOOP_KF = 0


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return a.shape == b.shape and np.array_equal(a, b)


def dev(d):
    import torch
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def trimmed(lc):
    """conn_* cut at n_connections; the rows past it must be skipped ones."""
    n = int(np.asarray(lc["n_connections"]).reshape(-1)[0])
    kf, begin = np.asarray(lc["conn_kf"]), np.asarray(lc["conn_begin"])
    assert (kf[n:len(begin) - 1] == -1).all() and (begin[n:] == begin[n]).all()
    return dict(conn_kf=kf[:n], conn_begin=begin[:n + 1], conn_slot=np.asarray(lc["conn_slot"])[:begin[n]], n_connections=n)


def run_device(name, padded, loop=True):
    """CorrectLoop's steps through the device entries on a fresh copy of the map, nothing read back between them but
    n_connected when not padded.  Everything back as numpy."""
    import torch
    cur = LC.CUR[name]
    m = dev(LC.tables(LC.case(name)))
    if name in ("small", "dirty"):
        MM.update_connections_device(m, torch.tensor([cur], dtype=torch.int32, device="cuda"))
    connected, n = L.connected_device(m, cur)
    max_connected = None if padded else int(n.item())
    prop = L.propagate_device(m, LC.SCALE, cur, torch.from_numpy(LC.scw(name)).cuda(), connected, max_connected)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in m.items()}
    out.update({k: prop[k].cpu().numpy() for k in ("vertex_sim3", "edge_sim3", "point_ref", "items", "status")})
    out.update(connected=connected.cpu().numpy(), n_connected=int(n.item()))
    if loop:
        lc = L.loop_connections_device(m, connected, max_connected)
        torch.cuda.synchronize()
        out["after_loop"] = {k: m[k].cpu().numpy() for k in R.STATE_KEYS}
        out["loop"] = trimmed({k: v.cpu().numpy() for k, v in lc.items()})
        out["loop"]["status"] = lc["status"].cpu().numpy()
    return out


def check_against_restatement(name, got, loop=True):
    conn, n = LC.expected_connected(name)
    assert same(got["connected"], conn) and got["n_connected"] == n
    want = LC.expected_propagate(name)
    for k in LR.UPDATED + ("vertex_sim3", "edge_sim3", "point_ref"):
        assert same(got[k], want[k]), k
    assert same(got["items"][:n], want["items"][:n]) and (got["items"][n:] == -1).all()
    after, status = LC.expected_after_propagate(name)
    for k in R.STATE_KEYS:
        assert same(got[k], after[k]), k
    assert same(got["status"], status)
    if loop:
        state, sets = LC.expected_loop_connections(name)
        for k in R.STATE_KEYS:
            assert same(got["after_loop"][k], state[k]), k
        for k in ("conn_kf", "conn_begin", "conn_slot"):
            assert same(got["loop"][k], sets[k]), k
        assert same(got["loop"]["status"], state["status"]) and got["loop"]["n_connections"] == sets["n_connections"]


@pytest.fixture(scope="module")
def device_runs():
    """One padded and one shortened run per clean map, shared by the tests below."""
    return {(name, padded): run_device(name, padded) for name in ("small", "wide") for padded in (True, False)}


@pytest.mark.parametrize("name", ["small", "wide"])
def test_the_device_entries_equal_the_restatement(device_runs, name):
    check_against_restatement(name, device_runs[(name, False)])
    want = LC.expected_propagate(name)
    m = LC.after_update(name)
    moved = (want["mp_xw"] != m["mp_xw"]).any(axis=1)
    assert moved.sum() > (256 if name == "wide" else 100) and not moved[m["mp_bad"] != 0].any()
    assert LC.expected_connected(name)[1] == (72 if name == "wide" else 7)      # 71 neighbours and cur: more than 64
    assert LC.expected_loop_connections(name)[1]["conn_begin"][-1] > 0


@pytest.mark.parametrize("name", ["small", "wide"])
def test_the_padded_list_gives_the_same_tables_as_the_count(device_runs, name):
    a, b = device_runs[(name, True)], device_runs[(name, False)]
    check_against_restatement(name, a)
    for k in LC.KEYS + ("vertex_sim3", "edge_sim3", "point_ref"):
        assert same(a[k], b[k]), k
    for k in ("conn_kf", "conn_begin", "conn_slot", "status"):
        assert same(a["loop"][k], b["loop"][k]), k


def test_a_rerun_is_byte_identical(device_runs):
    again = run_device("wide", True)
    first = device_runs[("wide", True)]
    for k in LC.KEYS + ("vertex_sim3", "edge_sim3", "point_ref", "items", "connected"):
        assert same(again[k], first[k]), k
    for k in ("conn_kf", "conn_begin", "conn_slot", "status"):
        assert same(again["loop"][k], first["loop"][k]), k


@pytest.mark.parametrize("name", ["dirty", "dirty_rows"])
def test_the_dirty_maps_go_through_the_device_entries(name):
    loop = name == "dirty"                             # UpdateConnections' restatement takes the rows as they are
    for padded in (True, False):
        check_against_restatement(name, run_device(name, padded, loop), loop)
    assert LC.expected_connected("dirty_rows")[1] == 5


@pytest.mark.parametrize("name", ["small", "wide"])
def test_the_host_entries_equal_the_restatement(name):
    cur = LC.CUR[name]
    m = LC.after_update(name)
    conn, n = L.Connected(m, cur)
    assert same(conn, LC.expected_connected(name)[0]) and n == LC.expected_connected(name)[1]
    got = L.Propagate(m, LC.SCALE, cur, LC.scw(name), conn[:n])
    want = LC.expected_propagate(name)
    for k in LR.UPDATED + ("vertex_sim3", "edge_sim3", "point_ref"):
        assert same(got[k], want[k]), k
    assert same(got["items"], want["items"][:n])
    after, status = LC.expected_after_propagate(name)
    for k in R.STATE_KEYS:
        assert same(got[k], after[k]), k
    assert same(got["status"], status)
    state, sets = L.LoopConnections(after, conn)        # the padded list
    want_state, want_sets = LC.expected_loop_connections(name)
    for k in R.STATE_KEYS + ("status",):
        assert same(state[k], want_state[k]), k
    for k in ("conn_kf", "conn_begin", "conn_slot"):
        assert same(sets[k], want_sets[k]), k
    assert sets["n_connections"] == want_sets["n_connections"]


# ------------------------------------------------------------------------------------------ the edge list
def eg_tables(state, loop, cur):
    """orbba_eg_tables as arrays from the graph state and the LoopConnections output, with two planted loop edges."""
    K = len(state["kf_id"])
    loops = [[] for _ in range(K)]
    loops[9], loops[2] = [1], [5, 0]
    csr = R.covis_csr(state)
    return dict(kf_id=state["kf_id"], parent=state["kf_parent"],
                loop_begin=np.concatenate([[0], np.cumsum([len(x) for x in loops])]).astype(np.int32),
                loop_slot=np.array([s for x in loops for s in x], np.int32), covis_begin=csr["covis_begin"],
                covis_slot=csr["covis_slot"], covis_weight=csr["covis_weight"], conn_kf=loop["conn_kf"],
                conn_begin=loop["conn_begin"], conn_slot=loop["conn_slot"], curr_slot=cur, loop_kf_slot=LOOP_KF), loops


def host_edges(t, loops):
    rows = lambda b, v: [list(v[b[k]:b[k + 1]]) for k in range(len(b) - 1)]   # noqa: E731
    cov = [list(zip(s, w)) for s, w in zip(rows(t["covis_begin"], t["covis_slot"]), rows(t["covis_begin"], t["covis_weight"]))]
    lists = dict(kf_id=t["kf_id"], parent=t["parent"], loop_edges=loops, covisibles=cov,
                 loop_connections=list(zip(t["conn_kf"], rows(t["conn_begin"], t["conn_slot"]))), curr_slot=t["curr_slot"],
                 loop_slot=t["loop_kf_slot"])
    return optimizer.essential_graph_edges(lists, MIN_WEIGHT)


def small_edges(planted):
    """The small map's tables and host edge list behind the restatement's CorrectLoop.  planted: every set also holds the
    first two keyframes of its ordered row, so that loop connections on both sides of MIN_WEIGHT are listed and the pairs
    that are kept meet the insertedEdges test of the covisibility pass."""
    state, sets = LC.expected_loop_connections("small")
    if planted:
        rows = [sorted(set(sets["conn_slot"][sets["conn_begin"][i]:sets["conn_begin"][i + 1]].tolist()) |
                       set(state["ord_slot"][k, :2].tolist())) for i, k in enumerate(sets["conn_kf"])]
        sets = dict(sets, conn_begin=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32),
                    conn_slot=np.array([s for r in rows for s in r], np.int32))
    t, loops = eg_tables(dict(LC.expected_after_propagate("small")[0], **{k: state[k] for k in R.STATE_KEYS}), sets, LC.CUR["small"])
    return t, host_edges(t, loops)


@pytest.mark.parametrize("delta", [0, 7, -3])
def test_the_device_edge_list_equals_the_host_one(delta):
    import torch
    t, (ei, ej, et) = small_edges(True)
    E = len(ei)
    assert 2 <= (et == 0).sum() < len(t["conn_slot"]) and (et == 1).sum() > len(t["kf_id"])
    assert len(ei) < len(small_edges(False)[1][0]) + (et == 0).sum() - 1           # insertedEdges left some pairs out
    got = L.essential_graph_edges_device(dev(t), E + delta, MIN_WEIGHT)
    torch.cuda.synchronize()
    gi, gj, gt = (got[k].cpu().numpy() for k in ("edge_i", "edge_j", "edge_table"))
    n = min(E, E + delta)
    assert int(got["n_edges"].item()) == E                                 # the full count, whatever the capacity
    assert same(gi[:n], ei[:n]) and same(gj[:n], ej[:n]) and same(gt[:n], et[:n])
    assert (gi[n:] == -1).all() and (gj[n:] == -1).all() and (gt[n:] == 0).all() and len(gi) == E + delta


def test_the_chain_on_one_stream_equals_the_host_optimisation_of_the_restatement():
    import torch
    name, cur = "chain", LC.CUR["chain"]
    want_m, fused, state, sets = LC.expected_chain()
    t, loops = eg_tables(dict(want_m, **{k: state[k] for k in R.STATE_KEYS}), sets, cur)
    ei, ej, et = host_edges(t, loops)
    want_p = LC.expected_propagate(name)
    host = optimizer.OptimizeEssentialGraph(dict(vertex_sim3=want_p["vertex_sim3"], edge_sim3=want_p["edge_sim3"], fixed_slot=LOOP_KF,
                                                 fix_scale=0, edge_i=ei, edge_j=ej, edge_table=et, points=want_p["mp_xw"],
                                                 point_ref=want_p["point_ref"]))
    # the walk of the matched points changes what UpdateConnections counts: the rows differ from those without it
    plain, _ = LR.loop_connections(LC.expected_after_propagate(name)[0], LC.expected_connected(name)[0])
    assert [tr[0] for tr in fused["trace"]].count("added") == 3 and [tr[0] for tr in fused["trace"]].count("replaced") == 5
    assert any(not same(plain[k], state[k]) for k in R.STATE_KEYS)

    m = dev(LC.tables(LC.case(name)))
    MM.update_connections_device(m, torch.tensor([cur], dtype=torch.int32, device="cuda"))
    connected, _ = L.connected_device(m, cur)
    prop = L.propagate_device(m, LC.SCALE, cur, torch.from_numpy(LC.scw(name)).cuda(), connected)
    walk = OBS.fuse_apply_device(m, OBS.APPLY_LOOP_MATCHED, *[torch.from_numpy(a).cuda() for a in LC.matched()])
    lc = L.loop_connections_device(m, connected)
    csr = MM.covis_csr_device(m)
    tables = dev({k: t[k] for k in ("kf_id", "loop_begin", "loop_slot")})
    tables.update(parent=m["kf_parent"], curr_slot=cur, loop_kf_slot=LOOP_KF, **{k: csr[k] for k in ("covis_begin", "covis_slot", "covis_weight")},
                  **{k: lc[k] for k in ("conn_kf", "conn_begin", "conn_slot")})
    capacity = len(ei) + 9
    edges = L.essential_graph_edges_device(tables, capacity, MIN_WEIGHT)
    got = optimizer.optimize_essential_graph_device(dict(vertex_sim3=prop["vertex_sim3"], edge_sim3=prop["edge_sim3"], fixed_slot=LOOP_KF,
                                                         fix_scale=0, edge_i=edges["edge_i"], edge_j=edges["edge_j"],
                                                         edge_table=edges["edge_table"], points=m["mp_xw"], point_ref=prop["point_ref"]))
    torch.cuda.synchronize()                                              # the first wait of the chain
    assert int(walk["status"].item()) == OBS.OK and int(walk["n_fused"].item()) == int(fused["n_fused"][0])
    for k in OR.UPDATED + LR.UPDATED:                                     # the map behind the walk
        assert same(m[k].cpu().numpy(), want_m[k]), k
    for k in R.STATE_KEYS:
        assert same(m[k].cpu().numpy(), state[k]), k
    dev_sets = trimmed({k: v.cpu().numpy() for k, v in lc.items()})
    for k in ("conn_kf", "conn_begin", "conn_slot"):
        assert same(dev_sets[k], sets[k]), k
    E = len(ei)
    assert int(edges["n_edges"].item()) == E
    assert same(edges["edge_i"].cpu().numpy()[:E], ei) and same(edges["edge_j"].cpu().numpy()[:E], ej)
    assert same(edges["edge_table"].cpu().numpy()[:E], et) and (edges["edge_i"].cpu().numpy()[E:] == -1).all()
    it = got["iterations"].cpu().numpy()
    assert (int(it[0]), int(it[1])) == (host["iterations"], host["trials"]) and host["trials"] > 0
    assert np.array_equal(got["accept"].cpu().numpy()[:host["trials"]].astype(bool), host["accept"])
    assert np.array_equal(got["sim3_g2o"].cpu().numpy().view(np.uint64), host["sim3_g2o"].view(np.uint64))
    assert same(got["pose"].cpu().numpy(), host["pose"]) and same(got["points"].cpu().numpy(), host["points"])
