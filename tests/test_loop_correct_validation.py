"""The loop-correction entries exist and refuse bad arguments with ORB_EINVAL before any device call (CPU only: no test
here reaches a device call)."""
import ctypes as C

import numpy as np
import pytest

import loop_correct_cases as LC
from orb_slam2_refactored_amd import _lib
from orb_slam2_refactored_amd import loop_correction as L

EXPORTS = ("orblc_connected", "orblc_connected_device", "orblc_propagate", "orblc_propagate_device", "orblc_loop_connections",
           "orblc_loop_connections_device", "orbba_essential_graph_edges_device")


def test_the_exports_exist():
    lib = _lib.lib()
    for name in EXPORTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def small():
    return LC.after_update("small")


def refused(fn, *args, **kw):
    with pytest.raises(_lib.OrbError) as e:
        fn(*args, **kw)
    assert "status -1" in str(e.value), str(e.value)


def conn():
    return LC.expected_connected("small")[0]


@pytest.mark.parametrize("cur", [-1, 12])
def test_cur_outside_the_table(cur):
    refused(L.Connected, small(), cur)
    refused(L.Propagate, small(), LC.SCALE, cur, LC.scw("small"), conn())


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
def test_a_scale_that_is_not_positive_and_a_non_finite_scw(bad):
    s = LC.scw("small")
    s[12] = bad
    refused(L.Propagate, small(), LC.SCALE, LC.CUR["small"], s, conn())
    if not np.isfinite(bad):
        s = LC.scw("small")
        s[4] = bad
        refused(L.Propagate, small(), LC.SCALE, LC.CUR["small"], s, conn())


def test_the_checks_of_update_normal_depth_hold_for_propagate():
    cur = LC.CUR["small"]
    for key, at, value in (("mp_obs_kf", 3, 12), ("mp_obs_idx", 3, -1), ("mp_ref_kf", 5, 12), ("kf_n", 2, 129),
                           ("kf_mappoint", (1, 0), 200), ("mp_obs_off", 0, 1)):
        m = small()
        m[key][at] = value
        refused(L.Propagate, m, LC.SCALE, cur, LC.scw("small"), conn())
    refused(L.Propagate, small(), np.ones(33, np.float32), cur, LC.scw("small"), conn())          # n_levels > 32
    refused(L.Propagate, small(), LC.SCALE, cur, LC.scw("small"), np.array([3, 12], np.int32))    # a connected slot outside
    refused(L.Propagate, small(), LC.SCALE, cur, LC.scw("small"), np.zeros(18, np.int32))         # longer than conn_cap + 1


def test_the_checks_of_update_connections_hold_for_the_rows():
    for key, at, value in (("n_ord", 6, 17), ("ord_slot", (6, 0), 12), ("n_conn", 1, -1)):
        m = small()
        m[key][at] = value
        refused(L.Connected, m, LC.CUR["small"])
        refused(L.LoopConnections, m, conn())
    for key, at, value in (("kf_parent", 0, 12), ("kf_covis", (0, 0), -2), ("mp_obs_kf", 0, -1), ("kf_mappoint", (0, 0), -2)):
        m = small()
        m[key][at] = value
        refused(L.LoopConnections, m, conn())
    refused(L.LoopConnections, small(), np.array([3, -2], np.int32))
    refused(L.LoopConnections, small(), np.zeros(18, np.int32))


def test_null_arguments_of_the_device_entries():
    lib = _lib.lib()
    m = _lib.OrblcMap()
    assert lib.orblc_connected_device(C.byref(m), 0, None, None, None) == -1
    assert lib.orblc_propagate_device(C.byref(m), 0, None, None, 0, None, None, None, None, None) == -1
    assert lib.orblc_loop_connections_device(C.byref(m), None, 0, None, None, None, None, None) == -1
    assert lib.orblc_connected_device(None, 0, None, None, None) == -1
    t = _lib.EssentialGraphTables()
    n = np.zeros(1, np.int32)
    assert lib.orbba_essential_graph_edges_device(C.byref(t), 0, 0, 0, 100, 0, None, None, None, _lib.ptr(n), None) == -1
    assert lib.orbba_essential_graph_edges_device(None, 0, 0, 0, 100, 0, None, None, None, None, None) == -1
