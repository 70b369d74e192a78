"""Argument validation of the culls: every ORB_EINVAL path of the host entries orbmm_cull_* / orbmm_compact_observations /
orbmm_children_live (all of them precede the first device call, so they run without a GPU), the shared checks of the device
entries, ValueError from the Python wrapper, and the C++ wrapper."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import culling_cases as CC
from orb_slam2_refactored_amd import culling as CU
from orb_slam2_refactored_amd._lib import OrbError, OrbmmCull, lib

ROOT = Path(__file__).resolve().parents[1]
POINT = ("kf_mappoint", "mp_bad", "mp_nobs", "mp_obs_off", "mp_obs_kf", "mp_obs_idx")
KEYFRAME = ("kf_id", "kf_n", "kf_kp_octave", "kf_uright", "kf_depth", "kf_pose", "kf_bad", "kf_not_erase", "kf_to_be_erased",
            "kf_tcp", "kf_parent", "kf_covis")
ROWS = ("conn_slot", "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord")


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


def points_of(t):
    return {k: t[k] for k in CU.POINT_KEYS}


def test_null_arguments_and_sizes_are_refused_by_both_entries():
    L = lib()
    one = C.c_void_p(8)   # never dereferenced: the checks below come first
    for rc in (L.orbmm_cull_map_points(None, 0, None, 0, 0, one, 0), L.orbmm_cull_map_points_device(None, 0, None, 0, 0, one, None),
               L.orbmm_cull_keyframes(None, 0, 0, 0.0, one, one, one, 0), L.orbmm_cull_keyframes_device(None, 0, 0, 0.0, one, one, one, None)):
        assert rc == -1 and "null cull tables" in last_error()
    ok = dict(n_keyframes=2, n_mappoints=2, kf_cap=4, conn_cap=4, n_obs=2)
    point = {k: one for k in POINT}
    full = dict(point, mp_found=one, mp_visible=one, mp_first_kf_id=one)
    for bad, text in ((dict(n_keyframes=-1), "negative sizes"), (dict(n_mappoints=-1), "negative sizes"), (dict(n_obs=-1), "negative sizes"),
                      (dict(kf_cap=0), "kf_cap must be at least 1"), (dict(n_keyframes=1 << 20, kf_cap=1 << 11), "2^31"),
                      (dict(), "null map-point table"), (point, "null map-point table")):
        c = OrbmmCull(**dict(ok, **bad))
        for rc in (L.orbmm_cull_map_points(C.byref(c), 0, None, 0, 0, one, 0),
                   L.orbmm_cull_map_points_device(C.byref(c), 0, None, 0, 0, one, None)):
            assert rc == -1 and text in last_error(), (bad, last_error())
    c = OrbmmCull(**dict(ok, **full))
    for args, text in (((-1, one, 0, 0, one), "negative sizes"), ((2, None, 0, 0, one), "null recent list"), ((0, None, 0, 0, None), "null recent list")):
        for rc in (L.orbmm_cull_map_points(C.byref(c), *args, 0), L.orbmm_cull_map_points_device(C.byref(c), *args, None)):
            assert rc == -1 and text in last_error(), (args, last_error())
    keyframe = dict(point, mp_ref_kf=one, **{k: one for k in KEYFRAME})
    for bad, text in ((dict(conn_cap=0), "conn_cap must be at least 1"), (dict(n_keyframes=1 << 20, conn_cap=1 << 11), "2^31"),
                      (point, "null map-point table"), (dict(point, mp_ref_kf=one), "null keyframe table"), (keyframe, "null row array")):
        c = OrbmmCull(**dict(ok, **bad))
        for rc in (L.orbmm_cull_keyframes(C.byref(c), 0, 0, 1.0, one, one, one, 0),
                   L.orbmm_cull_keyframes_device(C.byref(c), 0, 0, 1.0, one, one, one, None)):
            assert rc == -1 and text in last_error(), (bad, last_error())
    c = OrbmmCull(**dict(ok, **dict(keyframe, **{k: one for k in ROWS})))
    for rc in (L.orbmm_cull_keyframes(C.byref(c), 0, 0, 1.0, None, one, one, 0),
               L.orbmm_cull_keyframes_device(C.byref(c), 0, 0, 1.0, one, None, one, None)):
        assert rc == -1 and "null output" in last_error()
    for rc in (L.orbmm_compact_observations(-1, 0, one, one, one, one, one, one, 0),
               L.orbmm_compact_observations_device(2, -1, one, one, one, one, one, one, None)):
        assert rc == -1 and "negative sizes" in last_error()
    for rc in (L.orbmm_compact_observations(2, 2, None, one, one, one, one, one, 0),
               L.orbmm_compact_observations_device(2, 2, one, one, one, one, None, one, None)):
        assert rc == -1 and "null observation array" in last_error()
    for rc in (L.orbmm_children_live(-1, None, None, None, None, 0), L.orbmm_children_live_device(-1, None, None, None, None, None)):
        assert rc == -1 and "negative sizes" in last_error()
    for rc in (L.orbmm_children_live(2, one, None, one, one, 0), L.orbmm_children_live_device(2, one, None, one, one, None)):
        assert rc == -1 and "null children array" in last_error()


def test_empty_inputs_are_accepted_without_a_device():
    off = np.ones(1, np.int32)
    assert lib().orbmm_children_live(0, None, None, off.ctypes.data_as(C.c_void_p), None, 0) == 0 and off[0] == 0


def duplicate_in_a_row(t):
    """kf_mappoint with the point of (5, 0) written over another entry of row 5 below kf_n."""
    p = t["kf_mappoint"][5, 0]
    other = next(i for i in range(1, t["kf_n"][5]) if t["kf_mappoint"][5, i] not in (-1, p))
    assert p >= 0
    return poke(t["kf_mappoint"], (5, other), p)


def duplicate_in_the_observations(t):
    """mp_obs_kf with the first observer of a point written over its second."""
    p = next(p for p in range(CC.M) if t["mp_obs_off"][p + 1] - t["mp_obs_off"][p] >= 2)
    e = t["mp_obs_off"][p]
    return poke(t["mp_obs_kf"], e + 1, t["mp_obs_kf"][e])


@pytest.mark.parametrize("key,idx,value,text", [
    ("mp_obs_off", 0, 1, "mp_obs: offsets must start at 0"), ("mp_obs_off", 300, 0, "mp_obs: offsets must not decrease"),
    ("mp_obs_off", -1, 1 << 20, "mp_obs: offsets end past n_obs"),
    ("mp_obs_kf", 11, CC.K, "mp_obs_kf entry outside"), ("mp_obs_kf", 11, -1, "mp_obs_kf entry outside"),
    ("mp_obs_idx", 11, CC.KF_CAP, "mp_obs_idx entry outside"), ("mp_obs_idx", 11, -1, "mp_obs_idx entry outside"),
    ("kf_mappoint", (23, 255), CC.M, "kf_mappoint entry outside"), ("kf_mappoint", (0, 0), -2, "kf_mappoint entry outside"),
])
def test_the_tables_both_culls_read_are_validated_before_any_copy(key, idx, value, text):
    t = CC.tables(CC.case("clean"))
    t[key] = poke(t[key], idx, value)
    refused(lambda: CU.MapPointCulling(points_of(t), [1, 2], CC.CUR_KF_ID, False), text)
    refused(lambda: CU.KeyFrameCulling(t, CC.CUR, False, CC.TH_DEPTH), text)


@pytest.mark.parametrize("key,idx,value,text", [
    ("kf_n", 7, CC.KF_CAP + 1, "kf_n outside"), ("kf_n", 7, -1, "kf_n outside"),
    ("mp_ref_kf", 9, CC.K, "mp_ref_kf outside"), ("mp_ref_kf", 9, -2, "mp_ref_kf outside"),
    ("kf_parent", 5, CC.K, "kf_parent outside"), ("kf_parent", 5, -2, "kf_parent outside"),
    ("n_conn", 3, CC.CONN_CAP + 1, "n_conn outside"), ("n_conn", 3, -1, "n_conn outside"),
    ("n_ord", 4, CC.CONN_CAP + 1, "n_ord outside"), ("n_ord", 4, -1, "n_ord outside"),
    ("conn_slot", (2, 0), CC.K, "conn_slot entry outside"), ("ord_slot", (2, 1), -1, "ord_slot entry outside"),
])
def test_the_keyframe_tables_are_validated_before_any_copy(key, idx, value, text):
    t = CC.tables(CC.case("clean"))
    assert t["n_conn"][2] > 1 and t["n_ord"][2] > 1
    refused(lambda: CU.KeyFrameCulling(dict(t, **{key: poke(t[key], idx, value)}), CC.CUR, False, CC.TH_DEPTH), text)


def test_duplicates_lists_and_slots_are_refused():
    t = CC.tables(CC.case("clean"))
    refused(lambda: CU.KeyFrameCulling(dict(t, kf_mappoint=duplicate_in_a_row(t)), CC.CUR, False, CC.TH_DEPTH),
            "a map point twice in a keyframe's row")
    twice = dict(t, mp_obs_kf=duplicate_in_the_observations(t))
    refused(lambda: CU.KeyFrameCulling(twice, CC.CUR, False, CC.TH_DEPTH), "a keyframe twice in a map point's observations")
    refused(lambda: CU.MapPointCulling(points_of(twice), [1], CC.CUR_KF_ID, False), "a keyframe twice in a map point's observations")
    refused(lambda: CU.MapPointCulling(points_of(t), [0, CC.M], CC.CUR_KF_ID, False), "recent entry outside")
    refused(lambda: CU.MapPointCulling(points_of(t), [-1], CC.CUR_KF_ID, False), "recent entry outside")
    refused(lambda: CU.KeyFrameCulling(t, CC.K, False, CC.TH_DEPTH), "cur outside")
    refused(lambda: CU.KeyFrameCulling(t, -1, False, CC.TH_DEPTH), "cur outside")
    refused(lambda: CU.CompactObservations(poke(t["mp_obs_off"], 300, 0), t["mp_obs_kf"], t["mp_obs_idx"]), "offsets must not decrease")
    refused(lambda: CU.CompactObservations(poke(t["mp_obs_off"], -1, 1 << 20), t["mp_obs_kf"], t["mp_obs_idx"]), "offsets end past n_obs")
    refused(lambda: CU.LiveChildren(np.array([1, 2, 3], np.int32), np.zeros(3, np.uint8)), "kf_parent outside")
    refused(lambda: CU.LiveChildren(np.array([1, -2, 0], np.int32), np.zeros(3, np.uint8)), "kf_parent outside")


def test_the_dirty_case_is_refused():
    t = CC.tables(CC.case("dirty"))
    with pytest.raises(OrbError, match="status -1"):
        CU.KeyFrameCulling(t, CC.CUR, False, CC.TH_DEPTH)
    with pytest.raises(OrbError, match="status -1"):
        CU.MapPointCulling(points_of(t), CC.recent("dirty"), CC.CUR_KF_ID, False)


def test_the_python_wrapper_raises_on_dtype_shape_and_device():
    t = CC.tables(CC.case("clean"))
    with pytest.raises(ValueError, match="kf_depth must be float32"):
        CU.KeyFrameCulling(dict(t, kf_depth=t["kf_depth"].astype(np.float64)), CC.CUR, False, CC.TH_DEPTH)
    with pytest.raises(ValueError, match="kf_bad must be uint8"):
        CU.KeyFrameCulling(dict(t, kf_bad=t["kf_bad"].astype(np.int32)), CC.CUR, False, CC.TH_DEPTH)
    with pytest.raises(ValueError, match="kf_tcp must have shape"):
        CU.KeyFrameCulling(dict(t, kf_tcp=t["kf_tcp"][:, :9]), CC.CUR, False, CC.TH_DEPTH)
    with pytest.raises(ValueError, match="mp_nobs must have shape"):
        CU.MapPointCulling(dict(points_of(t), mp_nobs=t["mp_nobs"][:-1]), [1], CC.CUR_KF_ID, False)
    with pytest.raises(ValueError, match="one length"):
        CU.MapPointCulling(dict(points_of(t), mp_obs_idx=t["mp_obs_idx"][:-1]), [1], CC.CUR_KF_ID, False)
    with pytest.raises(ValueError, match="mp_found is required"):
        CU.MapPointCulling(dict(points_of(t), mp_found=None), [1], CC.CUR_KF_ID, False)
    with pytest.raises(ValueError, match="kf_uright is required"):
        CU.KeyFrameCulling(dict(t, kf_uright=None), CC.CUR, False, CC.TH_DEPTH)
    with pytest.raises(ValueError, match="kf_bad must have shape"):
        CU.LiveChildren(t["kf_parent"], t["kf_bad"][:-1])
    with pytest.raises(ValueError, match="mp_obs_idx must have shape"):
        CU.CompactObservations(t["mp_obs_off"], t["mp_obs_kf"], t["mp_obs_idx"][:-1])
    with pytest.raises(ValueError, match="GPU tensor"):
        CU.keyframe_culling_device(t, CC.CUR, False, CC.TH_DEPTH)   # host arrays to the device forms
    with pytest.raises(ValueError, match="GPU tensor"):
        CU.map_point_culling_device(points_of(t), CC.recent("clean"), CC.CUR_KF_ID, False)
    with pytest.raises(ValueError, match="GPU tensor"):
        CU.compact_observations_device(t["mp_obs_off"], t["mp_obs_kf"], t["mp_obs_idx"])
    with pytest.raises(ValueError, match="GPU tensor"):
        CU.live_children_device(t["kf_parent"], t["kf_bad"])


def test_cpp_wrapper_compiles_links_and_refuses(tmp_path):
    libso = ROOT / "orb_slam2_refactored_amd" / "liborbslam2_amd.so"
    main = tmp_path / "main.cpp"
    main.write_text("int use_culling(); int main() { return use_culling(); }\n")
    exe = tmp_path / "w"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "native" / "culling_wrapper_use.cpp"),
                    str(main), "-o", str(exe), f"-L{libso.parent}", "-lorbslam2_amd", f"-Wl,-rpath,{libso.parent}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
