"""Argument validation of map maintenance: every ORB_EINVAL path of the host entries orbmm_* (all of them precede the first
device call, so they run without a GPU), the shared checks of the device entries, ValueError from the Python wrapper, and the
C++ wrapper."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import map_maintenance_cases as MC
from orb_slam2_refactored_amd import map_maintenance as MM
from orb_slam2_refactored_amd._lib import OrbError, OrbmmCsr, OrbmmGraph, OrbmmPoints, lib

ROOT = Path(__file__).resolve().parents[1]


def last_error():
    return lib().orb_last_error().decode()


def poke(a, idx, v):
    a = a.copy()
    a[idx] = v
    return a


def refused(fn, text):
    with pytest.raises(OrbError, match="status -1") as e:
        fn()
    assert text in str(e.value), str(e.value)


def test_null_arguments_and_sizes_are_refused_by_both_entries():
    L = lib()
    one = C.c_void_p(8)   # never dereferenced: the checks below come first
    for rc in (L.orbmm_update_normal_depth(None, 0), L.orbmm_update_normal_depth_device(None, None)):
        assert rc == -1 and "null points" in last_error()
    for rc in (L.orbmm_update_connections(None, 0, None, 0), L.orbmm_update_connections_device(None, 0, None, None),
               L.orbmm_covis_csr(None, None, 0), L.orbmm_covis_csr_device(None, None, None)):
        assert rc == -1 and "null graph" in last_error()
    ok = dict(n_keyframes=2, n_mappoints=2, kf_cap=4, n_obs=2, n_levels=8)
    for bad, text in ((dict(n_keyframes=-1), "negative sizes"), (dict(n_mappoints=-1), "negative sizes"), (dict(n_obs=-1), "negative sizes"),
                      (dict(kf_cap=0), "kf_cap must be at least 1"), (dict(n_levels=0), "n_levels"), (dict(n_levels=33), "n_levels"),
                      (dict(n_keyframes=1 << 20, kf_cap=1 << 11), "2^31"), (dict(), "null scale_factors"),
                      (dict(scale_factors=one), "null map-point table")):
        p = OrbmmPoints(**dict(ok, **bad))
        for rc in (L.orbmm_update_normal_depth(C.byref(p), 0), L.orbmm_update_normal_depth_device(C.byref(p), None)):
            assert rc == -1 and text in last_error(), (bad, last_error())
    ok = dict(n_keyframes=2, n_mappoints=2, kf_cap=4, conn_cap=4, n_obs=2)
    rows = dict(conn_slot=one, conn_weight=one, n_conn=one, ord_slot=one, ord_weight=one, n_ord=one)
    for bad, text in ((dict(n_keyframes=-1), "negative sizes"), (dict(kf_cap=0), "kf_cap must be at least 1"),
                      (dict(conn_cap=0), "conn_cap must be at least 1"), (dict(n_keyframes=1 << 20, conn_cap=1 << 11), "2^31"),
                      (dict(), "null row array"), (rows, "null keyframe table")):
        g = OrbmmGraph(**dict(ok, **bad))
        for rc in (L.orbmm_update_connections(C.byref(g), 0, None, 0), L.orbmm_update_connections_device(C.byref(g), 0, None, None)):
            assert rc == -1 and text in last_error(), (bad, last_error())
    g = OrbmmGraph(**dict(ok, **rows))
    for rc in (L.orbmm_covis_csr(C.byref(g), None, 0), L.orbmm_covis_csr_device(C.byref(g), None, None)):
        assert rc == -1 and "null csr" in last_error()
    for c, text in ((OrbmmCsr(covis_begin=one), "null covis array"), (OrbmmCsr(conn_off=one), "null conn array"),
                    (OrbmmCsr(conn_off=one, conn_idx=one, n_queries=-1), "negative sizes"),
                    (OrbmmCsr(conn_off=one, conn_idx=one, n_queries=2), "null query")):
        for rc in (L.orbmm_covis_csr(C.byref(g), C.byref(c), 0), L.orbmm_covis_csr_device(C.byref(g), C.byref(c), None)):
            assert rc == -1 and text in last_error(), last_error()
    for rc in (L.orbmm_children(-1, None, None, None, 0), L.orbmm_children_device(-1, None, None, None, None)):
        assert rc == -1 and "negative sizes" in last_error()
    for rc in (L.orbmm_children(2, None, None, None, 0), L.orbmm_children_device(2, None, None, None, None)):
        assert rc == -1 and "null children array" in last_error()


def test_empty_batches_are_accepted_without_a_device():
    one = C.c_void_p(8)
    p = OrbmmPoints(n_keyframes=2, n_mappoints=0, kf_cap=4, n_levels=8, **{k: one for k in (
        "scale_factors", "mp_bad", "mp_xw", "mp_ref_kf", "mp_obs_off", "mp_obs_kf", "mp_obs_idx", "kf_pose", "kf_n", "kf_kp_octave",
        "mp_normal", "mp_max_min")})
    assert lib().orbmm_update_normal_depth(C.byref(p), 0) == 0
    off = np.ones(1, np.int32)
    assert lib().orbmm_children(0, None, off.ctypes.data_as(C.c_void_p), None, 0) == 0 and off[0] == 0


@pytest.mark.parametrize("key,idx,value,text", [
    ("mp_obs_off", 0, 1, "mp_obs: offsets must start at 0"), ("mp_obs_off", 300, 0, "mp_obs: offsets must not decrease"),
    ("mp_obs_off", -1, 1 << 20, "mp_obs: offsets end past n_obs"),
    ("mp_obs_kf", 11, MC.K, "mp_obs_kf entry outside"), ("mp_obs_kf", 11, -1, "mp_obs_kf entry outside"),
    ("kf_n", 7, MC.KF_CAP + 1, "kf_n outside"), ("kf_n", 7, -1, "kf_n outside"),
    ("kf_mappoint", (23, 255), MC.M, "kf_mappoint entry outside"), ("kf_mappoint", (0, 0), -2, "kf_mappoint entry outside"),
    ("n_conn", 3, MC.CONN_CAP + 1, "n_conn outside"), ("n_conn", 3, -1, "n_conn outside"),
    ("n_ord", 4, MC.CONN_CAP + 1, "n_ord outside"), ("n_ord", 4, -1, "n_ord outside"),
    ("conn_slot", (2, 0), MC.K, "conn_slot entry outside"), ("ord_slot", (2, 1), -1, "ord_slot entry outside"),
    ("kf_parent", 5, MC.K, "kf_parent outside"), ("kf_parent", 5, -2, "kf_parent outside"),
    ("kf_covis", (3, 2), MC.K, "kf_covis entry outside"), ("kf_covis", (0, 0), -2, "kf_covis entry outside"),
])
def test_graph_tables_are_validated_before_any_copy(key, idx, value, text):
    g = MC.graph(MC.case("clean"))
    assert g["n_conn"][2] > 1 and g["n_ord"][2] > 1
    refused(lambda: MM.UpdateConnections(dict(g, **{key: poke(g[key], idx, value)}), [1, 2]), text)


def test_items_queries_and_rows_are_validated():
    g = MC.graph(MC.case("clean"))
    refused(lambda: MM.UpdateConnections(g, [0, MC.K]), "item outside")
    refused(lambda: MM.UpdateConnections(g, [-1]), "item outside")
    refused(lambda: MM.CovisCsr(g, queries=[MC.K]), "query outside")
    refused(lambda: MM.CovisCsr(dict(g, n_ord=poke(g["n_ord"], 1, MC.CONN_CAP + 1))), "n_ord outside")
    refused(lambda: MM.CovisCsr(dict(g, conn_slot=poke(g["conn_slot"], (2, 0), -1)), queries=[2]), "conn_slot entry outside")
    refused(lambda: MM.Children(np.array([1, 2, 3], np.int32)), "kf_parent outside")
    refused(lambda: MM.Children(np.array([1, -2, 0], np.int32)), "kf_parent outside")


@pytest.mark.parametrize("key,idx,value,text", [
    ("mp_obs_off", 0, 1, "mp_obs: offsets must start at 0"), ("mp_obs_off", 300, 0, "mp_obs: offsets must not decrease"),
    ("mp_obs_kf", 11, MC.K, "mp_obs_kf entry outside"), ("mp_obs_kf", 11, -1, "mp_obs_kf entry outside"),
    ("mp_obs_idx", 11, MC.KF_CAP, "mp_obs_idx entry outside"), ("mp_obs_idx", 11, -1, "mp_obs_idx entry outside"),
    ("mp_ref_kf", 9, MC.K, "mp_ref_kf outside"), ("mp_ref_kf", 9, -2, "mp_ref_kf outside"),
    ("kf_n", 7, MC.KF_CAP + 1, "kf_n outside"), ("kf_n", 7, -1, "kf_n outside"),
    ("kf_kp_octave", (2, 0), MC.N_LEVELS, "kf_kp_octave entry outside"), ("kf_kp_octave", (2, 0), -1, "kf_kp_octave entry outside"),
])
def test_point_tables_are_validated_before_any_copy(key, idx, value, text):
    t = MC.points(MC.case("clean"))
    refused(lambda: MM.UpdateNormalAndDepth(dict(t, **{key: poke(t[key], idx, value)}), MC.SCALE), text)


def test_point_lists_scalars_and_the_python_wrapper():
    t, g = MC.points(MC.case("clean")), MC.graph(MC.case("clean"))
    refused(lambda: MM.UpdateNormalAndDepth(t, MC.SCALE, [0, MC.M]), "point outside")
    refused(lambda: MM.UpdateNormalAndDepth(t, MC.SCALE, [-1]), "point outside")
    refused(lambda: MM.UpdateNormalAndDepth(t, np.ones(33, np.float32)), "n_levels")
    refused(lambda: MM.UpdateNormalAndDepth(t, np.ones(0, np.float32)), "n_levels")
    with pytest.raises(ValueError, match="mp_xw must be float32"):
        MM.UpdateNormalAndDepth(dict(t, mp_xw=t["mp_xw"].astype(np.float64)), MC.SCALE)
    with pytest.raises(ValueError, match="mp_obs_off must have shape"):
        MM.UpdateNormalAndDepth(dict(t, mp_obs_off=t["mp_obs_off"][:-1]), MC.SCALE)
    with pytest.raises(ValueError, match="one length"):
        MM.UpdateNormalAndDepth(dict(t, mp_obs_idx=t["mp_obs_idx"][:-1]), MC.SCALE)
    with pytest.raises(ValueError, match="kf_covis must have shape"):
        MM.UpdateConnections(dict(g, kf_covis=g["kf_covis"][:, :9]), [1])
    with pytest.raises(ValueError, match="ord_weight must have shape"):
        MM.UpdateConnections(dict(g, ord_weight=g["ord_weight"][:, :5]), [1])
    with pytest.raises(ValueError, match="kf_id is required"):
        MM.UpdateConnections(dict(g, kf_id=None), [1])
    with pytest.raises(ValueError, match="GPU tensor"):
        MM.update_connections_device(g, np.array([1], np.int32))   # host arrays to the device form
    with pytest.raises(ValueError, match="GPU tensor"):
        MM.update_normal_depth_device(t, MC.SCALE)


def test_cpp_wrapper_compiles_links_and_refuses(tmp_path):
    libso = ROOT / "orb_slam2_refactored_amd" / "liborbslam2_amd.so"
    main = tmp_path / "main.cpp"
    main.write_text("int use_map_maintenance(); int main() { return use_map_maintenance(); }\n")
    exe = tmp_path / "w"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "native" / "map_maintenance_wrapper_use.cpp"),
                    str(main), "-o", str(exe), f"-L{libso.parent}", "-lorbslam2_amd", f"-Wl,-rpath,{libso.parent}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
