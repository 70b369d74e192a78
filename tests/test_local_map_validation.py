"""Argument validation of Tracking's local map: every ORB_EINVAL path of the host entry orbtl_track_local_map (all of them
precede the first device call, so they run without a GPU), the shared checks of the device entry, ValueError from the Python
wrapper, and the C++ wrapper."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import local_map_cases as LC
from orb_slam2_refactored_amd import local_map as LM
from orb_slam2_refactored_amd._lib import OrbError, OrbtlFrames, OrbtlMap, OrbtlResult, lib

ROOT = Path(__file__).resolve().parents[1]


def last_error():
    return lib().orb_last_error().decode()


@pytest.fixture()
def small():
    m, fr, _ = LC.batch(LC.case("mixed"), 3)
    return m, fr


def call(m, fr, mp_cap=700, **kw):
    return LM.LocalMap(m).TrackLocalMap(dict(fr, **kw), mp_cap)


def refused(m, fr, text, **kw):
    with pytest.raises(OrbError, match="status -1") as e:
        call(m, fr, **kw)
    assert text in str(e.value), str(e.value)


def test_null_arguments_and_sizes_are_refused_by_both_entries():
    L = lib()
    m, fr, r = OrbtlMap(), OrbtlFrames(), OrbtlResult()
    for rc in (L.orbtl_track_local_map(None, C.byref(fr), C.byref(r), 0), L.orbtl_track_local_map(C.byref(m), None, C.byref(r), 0),
               L.orbtl_track_local_map(C.byref(m), C.byref(fr), None, 0), L.orbtl_track_local_map_device(None, C.byref(fr), C.byref(r), None)):
        assert rc == -1 and "null map, frames or result" in last_error()
    ok = dict(n_frames=1, kp_cap=4, kf_list_cap=4, mp_cap=4, n_levels=8, log_scale_factor=0.18, min_view_cos=0.5)
    for bad, text in ((dict(n_frames=-1), "negative sizes"), (dict(kp_cap=0), "kf_cap and kp_cap"), (dict(kf_list_cap=0), "kf_list_cap must be at least 1"),
                      (dict(mp_cap=0), "mp_cap must be at least 1"), (dict(n_levels=0), "n_levels"), (dict(n_levels=33), "n_levels"),
                      (dict(log_scale_factor=0.0), "log_scale_factor"), (dict(log_scale_factor=float("nan")), "log_scale_factor"),
                      (dict(kf_list_cap=65536), "2^31"), (dict(), "null keyframe table")):
        m = OrbtlMap(n_keyframes=2, n_mappoints=2, kf_cap=1 << 15 if "kf_list_cap" in bad and bad["kf_list_cap"] > 1 else 4)
        fr = OrbtlFrames(**dict(ok, **bad))
        for rc in (L.orbtl_track_local_map(C.byref(m), C.byref(fr), C.byref(r), 0), L.orbtl_track_local_map_device(C.byref(m), C.byref(fr), C.byref(r), None)):
            assert rc == -1 and text in last_error(), (bad, last_error())
    m = OrbtlMap(n_keyframes=2, n_mappoints=2, kf_cap=0)
    assert L.orbtl_track_local_map(C.byref(m), C.byref(OrbtlFrames(**ok)), C.byref(r), 0) == -1 and "kf_cap and kp_cap" in last_error()
    m = OrbtlMap(n_keyframes=-1, n_mappoints=2, kf_cap=4)
    assert L.orbtl_track_local_map(C.byref(m), C.byref(OrbtlFrames(**ok)), C.byref(r), 0) == -1 and "negative sizes" in last_error()


def test_an_empty_batch_is_accepted_without_a_device():
    m, r = OrbtlMap(n_keyframes=2, n_mappoints=2, kf_cap=4), OrbtlResult()
    fr = OrbtlFrames(n_frames=0, kp_cap=4, kf_list_cap=4, mp_cap=4, n_levels=8, log_scale_factor=0.18)
    assert lib().orbtl_track_local_map(C.byref(m), C.byref(fr), C.byref(r), 0) == 0


def poke(a, idx, v):
    a = a.copy()
    a[idx] = v
    return a


@pytest.mark.parametrize("key,idx,value,text", [
    ("kf_covis", (3, 2), 70, "kf_covis entry outside"), ("kf_covis", (0, 0), -2, "kf_covis entry outside"),
    ("kf_parent", 5, 70, "kf_parent outside"), ("kf_parent", 5, -2, "kf_parent outside"),
    ("kf_child_off", 0, 1, "kf_child: offsets must start at 0"), ("kf_child_off", 10, 0, "kf_child: offsets must not decrease"),
    ("kf_child_idx", 3, 70, "kf_child: keyframe slot outside"), ("kf_child_idx", 3, -1, "kf_child: keyframe slot outside"),
    ("kf_n", 7, 97, "kf_n outside"), ("kf_n", 7, -1, "kf_n outside"),
    ("kf_mappoint", (69, 95), 700, "kf_mappoint entry outside"), ("kf_mappoint", (0, 0), -2, "kf_mappoint entry outside"),
    ("mp_obs_off", 0, 2, "mp_obs: offsets must start at 0"), ("mp_obs_off", 300, 0, "mp_obs: offsets must not decrease"),
    ("mp_obs_kf", 11, 70, "mp_obs: keyframe slot outside"), ("mp_obs_kf", 11, -1, "mp_obs: keyframe slot outside"),
])
def test_map_tables_are_validated_before_any_copy(small, key, idx, value, text):
    m, fr = small
    assert len(m["mp_bad"]) == 700 and len(m["kf_bad"]) == 70
    refused(dict(m, **{key: poke(m[key], idx, value)}), fr, text)


@pytest.mark.parametrize("key,idx,value,text", [
    ("frame_n", 1, 161, "frame_n outside"), ("frame_n", 1, -1, "frame_n outside"),
    ("frame_mappoint", (2, 159), 700, "frame_mappoint entry outside"), ("frame_mappoint", (0, 0), -2, "frame_mappoint entry outside"),
    ("n_local_kf", 0, 79, "n_local_kf outside"), ("n_local_kf", 0, -1, "n_local_kf outside"),
])
def test_frame_arrays_are_validated_before_any_copy(small, key, idx, value, text):
    m, fr = small
    assert fr["frame_mappoint"].shape == (3, 160) and fr["local_kf"].shape == (3, 78)
    refused(m, dict(fr, **{key: poke(fr[key], idx, value)}), text)


def test_old_list_entries_scalars_and_capacities_are_validated(small):
    m, fr = small
    lk = fr["local_kf"].copy()
    lk[1, 0] = 70
    refused(m, dict(fr, local_kf=lk, n_local_kf=np.array([0, 1, 0], np.int32)), "local_kf entry outside")
    lk[1, 0] = -1                                       # within the list a null is refused too
    refused(m, dict(fr, local_kf=lk, n_local_kf=np.array([0, 1, 0], np.int32)), "local_kf entry outside")
    refused(m, fr, "n_levels", n_levels=0)
    refused(m, fr, "n_levels", n_levels=33)
    refused(m, fr, "log_scale_factor", log_scale_factor=-0.1)
    with pytest.raises(ValueError, match="mp_cap must be at least 1"):
        call(m, fr, mp_cap=0)


def test_python_wrapper_refuses_wrong_shapes_and_dtypes(small):
    m, fr = small
    with pytest.raises(ValueError, match="kf_covis must have shape"):
        call(dict(m, kf_covis=m["kf_covis"][:, :9]), fr)
    with pytest.raises(ValueError, match="mp_xw must be float32"):
        call(dict(m, mp_xw=m["mp_xw"].astype(np.float64)), fr)
    with pytest.raises(ValueError, match="mp_obs_off must have shape"):
        call(dict(m, mp_obs_off=m["mp_obs_off"][:-1]), fr)
    with pytest.raises(ValueError, match="mp_normal is required"):
        call(dict(m, mp_normal=None), fr)
    with pytest.raises(ValueError, match="pose must have shape"):
        call(m, dict(fr, pose=fr["pose"][:2]))
    with pytest.raises(ValueError, match="camera must have shape"):
        call(m, dict(fr, camera=fr["camera"][:, :4]))
    with pytest.raises(ValueError, match="shorter than its offsets"):
        call(dict(m, mp_obs_kf=m["mp_obs_kf"][:-1]), fr)
    with pytest.raises(ValueError, match="GPU tensor"):
        LM.LocalMap(m).track_local_map_device(fr, 700)   # host arrays to the device form


def test_cpp_wrapper_compiles_links_and_refuses(tmp_path):
    libso = ROOT / "orb_slam2_refactored_amd" / "liborbslam2_amd.so"
    main = tmp_path / "main.cpp"
    main.write_text("int use_local_map(); int main() { return use_local_map(); }\n")
    exe = tmp_path / "w"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "native" / "local_map_wrapper_use.cpp"),
                    str(main), "-o", str(exe), f"-L{libso.parent}", "-lorbslam2_amd", f"-Wl,-rpath,{libso.parent}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
