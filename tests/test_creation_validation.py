"""Argument validation of map creation: every ORB_EINVAL path of the host entries orbmk_insert_keyframes / orbmk_create_points
(all of them precede the first device call, so they run without a GPU), the shared checks of the device entries, ValueError
from the Python wrapper, the C-ABI exports and the C++ wrapper."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import creation_cases as CC
from orb_slam2_refactored_amd import creation as CN
from orb_slam2_refactored_amd._lib import OrbError, OrbmkCreated, OrbmkFrames, OrbmkKeyframes, OrbmkLists, OrbmkMap, lib

ROOT = Path(__file__).resolve().parents[1]
EXPORTS = ("orbmk_insert_keyframes", "orbmk_create_points")
one = C.c_void_p(16)   # never dereferenced: the checks below come first


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


def fields(cls, ints, **over):
    """A struct with every pointer set and the given sizes."""
    vals = {name: (one if typ is C.c_void_p else 0) for name, typ in cls._fields_}
    return cls(**dict(vals, **ints, **over))


def test_the_c_abi_exports_are_present():
    so = C.CDLL(lib()._name)
    for name in EXPORTS:
        assert getattr(so, name) and getattr(so, name + "_device")


def test_insert_refuses_null_arguments_and_sizes_in_both_forms():
    L = lib()
    fr_ok, kf_ok = dict(n_frames=2, kp_cap=8), dict(n_keyframes=3, kf_cap=8, conn_cap=4)

    def both(fr, kf, n=1, items=(one, one, one, one)):
        a = (C.byref(fr) if fr else None, C.byref(kf) if kf else None, n, *items)
        return L.orbmk_insert_keyframes(*a, 0), L.orbmk_insert_keyframes_device(*a, None)
    fr, kf = fields(OrbmkFrames, fr_ok), fields(OrbmkKeyframes, kf_ok)
    for args, text in (((None, kf), "null frames or keyframe tables"), ((fr, None), "null frames or keyframe tables"),
                       ((fields(OrbmkFrames, dict(fr_ok, n_frames=-1)), kf), "negative sizes"),
                       ((fr, fields(OrbmkKeyframes, dict(kf_ok, n_keyframes=-1))), "negative sizes"), ((fr, kf, -1), "negative sizes"),
                       ((fr, kf, 65536), "65536 items"), ((fields(OrbmkFrames, dict(fr_ok, kp_cap=0)), kf), "at least 1"),
                       ((fr, fields(OrbmkKeyframes, dict(kf_ok, kf_cap=0))), "at least 1"),
                       ((fields(OrbmkFrames, dict(fr_ok, kp_cap=9)), kf), "kp_cap must not exceed kf_cap"),
                       ((fr, fields(OrbmkKeyframes, dict(kf_ok, conn_cap=0))), "conn_cap must be at least 1"),
                       ((fr, fields(OrbmkKeyframes, dict(kf_ok, n_keyframes=1 << 20, kf_cap=1 << 10))), "2^31"),
                       ((fields(OrbmkFrames, dict(fr_ok, n_frames=1 << 20, kp_cap=1 << 10)), fields(OrbmkKeyframes, dict(kf_ok, kf_cap=1 << 10))), "2^31"),
                       ((fr, kf, 1, (None, one, one, one)), "null item array"), ((fr, kf, 1, (one, None, one, one)), "null item array"),
                       ((fields(OrbmkFrames, fr_ok, frame_n=None), kf), "null frame_n"), ((fr, kf, 1, (one, one, None, one)), "kf_id without item ids"),
                       ((fr, kf, 1, (one, one, one, None)), "kf_camera without"), ((fields(OrbmkFrames, fr_ok, camera=None), kf), "kf_camera without"),
                       *[((fields(OrbmkFrames, fr_ok, **{src: None}), kf), "a keyframe table without its frame array")
                         for dst, src in CN.KEYFRAME_SOURCE.items() if dst not in ("kf_n", "kf_camera")],
                       ((fields(OrbmkFrames, fr_ok, kp_un=C.c_void_p(18)), kf), "keypoint records are not aligned")):
        for rc in both(*args):
            assert rc == -1 and text in last_error(), (text, last_error())
    odd = fields(OrbmkKeyframes, kf_ok, kf_desc=C.c_void_p(24))
    assert L.orbmk_insert_keyframes_device(C.byref(fr), C.byref(odd), 1, one, one, one, one, None) == -1 and "16-byte aligned" in last_error()
    # every keyframe table is optional, and with none of a group its source may be left out
    bare = OrbmkKeyframes(n_keyframes=3, kf_cap=8, conn_cap=0, kf_n=one)
    assert L.orbmk_insert_keyframes_device(C.byref(OrbmkFrames(n_frames=2, kp_cap=8, frame_n=one)), C.byref(bare), 0, None, None, None, None, None) == 0


def test_insert_refuses_inconsistent_tables_before_any_copy():
    fr, kf = CC.make_frames(F=3, kp_cap=40), CC.make_keyframes(K=5, kf_cap=44, conn_cap=6)
    it = dict(item_frame=np.array([1, 0], np.int32), item_kf=np.array([3, 0], np.int32), item_id=np.array([5, 6], np.int32),
              item_baseline=np.array([.1, .2], np.float32))
    for bad, text in ((dict(item_frame=poke(it["item_frame"], 1, 3)), "item_frame outside"), (dict(item_frame=poke(it["item_frame"], 0, -1)), "item_frame outside"),
                      (dict(item_kf=poke(it["item_kf"], 1, 5)), "item_kf outside"), (dict(item_kf=poke(it["item_kf"], 1, 3)), "a keyframe slot twice")):
        refused(lambda: CN.InsertKeyFrames(fr, kf, **dict(it, **bad)), text)
    for n in (-1, 41):
        refused(lambda: CN.InsertKeyFrames(dict(fr, frame_n=poke(fr["frame_n"], 2, n)), kf, **it), "frame_n outside [0, kp_cap]")


def test_create_refuses_null_arguments_and_sizes_in_both_forms():
    L = lib()
    m_ok, l_ok = dict(n_keyframes=2, n_mappoints=4, kf_cap=8, n_obs=8), dict(n_items=1, list_cap=8, n_frames=1, kp_cap=8)

    def both(m, ls, o):
        a = (C.byref(m) if m else None, C.byref(ls) if ls else None, C.byref(o) if o else None)
        return L.orbmk_create_points(*a, 0), L.orbmk_create_points_device(*a, None)
    m, ls, o = fields(OrbmkMap, m_ok), fields(OrbmkLists, l_ok), fields(OrbmkCreated, dict(recent_cap=4))
    cases = [((None, ls, o), "null map, lists or outputs"), ((m, None, o), "null map, lists or outputs"), ((m, ls, None), "null map, lists or outputs"),
             *[((fields(OrbmkMap, dict(m_ok, **{k: -1})), ls, o), "negative sizes") for k in ("n_keyframes", "n_mappoints", "n_obs")],
             ((m, fields(OrbmkLists, dict(l_ok, n_items=-1)), o), "negative sizes"), ((m, fields(OrbmkLists, dict(l_ok, n_items=65536)), o), "65536 items"),
             ((fields(OrbmkMap, dict(m_ok, kf_cap=0)), ls, o), "kf_cap must be at least 1"),
             ((m, fields(OrbmkLists, dict(l_ok, list_cap=0)), o), "list_cap must be at least 1"),
             ((m, fields(OrbmkLists, l_ok, values_by_keypoint=2), o), "values_by_keypoint must be 0 or 1"),
             ((fields(OrbmkMap, dict(m_ok, n_keyframes=1 << 20, kf_cap=1 << 10)), ls, o), "2^31"),
             ((fields(OrbmkMap, dict(m_ok, n_mappoints=1 << 30)), ls, o), "2^31"),
             ((m, fields(OrbmkLists, dict(l_ok, n_items=60000, list_cap=1 << 14)), o), "2^31"),
             *[((fields(OrbmkMap, m_ok, **{k: None}), ls, o), "null keyframe table") for k in ("kf_id", "kf_n", "kf_mappoint", "kf_uright")],
             *[((fields(OrbmkMap, m_ok, **{k: None}), ls, o), "null map-point table")
               for k in ("mp_bad", "mp_xw", "mp_nobs", "mp_found", "mp_visible", "mp_replaced", "mp_first_kf_id", "mp_ref_kf", "mp_obs_off",
                         "mp_obs_kf", "mp_obs_idx")],
             ((fields(OrbmkMap, m_ok, kf_desc=None), ls, o), "kf_desc and mp_desc go together"),
             ((fields(OrbmkMap, m_ok, mp_desc=None), ls, o), "kf_desc and mp_desc go together"),
             *[((m, fields(OrbmkLists, l_ok, **{k: None}), o), "null list array") for k in ("kf1", "n_list", "idx1", "xw")],
             ((m, fields(OrbmkLists, l_ok, idx2=None), o), "kf2 without idx2"),
             ((m, fields(OrbmkLists, l_ok, item_frame=None), o), "frame_mappoint without"), ((m, fields(OrbmkLists, dict(l_ok, kp_cap=0)), o), "frame_mappoint without"),
             *[((m, ls, fields(OrbmkCreated, dict(recent_cap=4), **{k: None})), "null output") for k in ("alloc", "status", "needed")],
             ((m, ls, fields(OrbmkCreated, dict(recent_cap=4), n_recent=None)), "recent without"),
             ((m, ls, fields(OrbmkCreated, dict(recent_cap=-1))), "recent without")]
    for args, text in cases:
        for rc in both(*args):
            assert rc == -1 and text in last_error(), (text, last_error())
    odd = fields(OrbmkMap, m_ok, mp_desc=C.c_void_p(24))
    assert L.orbmk_create_points_device(C.byref(odd), C.byref(ls), C.byref(o), None) == -1 and "16-byte aligned" in last_error()


def test_create_refuses_inconsistent_tables_before_any_copy():
    t = CC.make_map(K=4, kf_cap=96, M=120, alloc=3, seed=7)
    ls = CC.make_lists(t, (20, 20, 20), 64, two=True, frames=(2, 64))
    call = lambda t=t, ls=ls, alloc=3, **kw: CN.CreatePoints(t, ls, alloc, **kw)   # noqa: E731
    for bad, text in ((dict(mp_obs_off=poke(t["mp_obs_off"], 0, 1)), "offsets must start at 0"),
                      (dict(mp_obs_off=poke(t["mp_obs_off"], 5, 0)), "offsets must not decrease"),
                      (dict(mp_obs_off=poke(t["mp_obs_off"], 120, 1 << 20)), "offsets end past n_obs"),
                      (dict(kf_n=poke(t["kf_n"], 1, 97)), "kf_n outside [0, kf_cap]"), (dict(kf_n=poke(t["kf_n"], 1, -1)), "kf_n outside [0, kf_cap]")):
        refused(lambda: call(t=dict(t, **bad)), text)
    for bad, text in ((dict(kf1=poke(ls["kf1"], 1, 4)), "kf1 outside"), (dict(kf1=poke(ls["kf1"], 1, -1)), "kf1 outside"),
                      (dict(kf2=poke(ls["kf2"], 1, 4)), "kf2 outside"), (dict(kf2=poke(ls["kf2"], 1, -2)), "kf2 outside"),
                      (dict(n_list=poke(ls["n_list"], 2, 65)), "n_list outside"), (dict(n_list=poke(ls["n_list"], 2, -1)), "n_list outside"),
                      (dict(idx1=poke(ls["idx1"], (1, 3), 96)), "idx1 outside"), (dict(idx1=poke(ls["idx1"], (1, 3), -2)), "idx1 outside"),
                      (dict(idx2=poke(ls["idx2"], (2, 19), 96)), "idx2 outside"), (dict(idx2=poke(ls["idx2"], (0, 0), -2)), "idx2 outside"),
                      (dict(item_frame=poke(ls["item_frame"], 0, 2)), "item_frame outside"), (dict(item_frame=poke(ls["item_frame"], 0, -2)), "item_frame outside"),
                      (dict(idx1=poke(ls["idx1"], (1, 3), ls["idx1"][1, 4])), "a keypoint of a keyframe twice"),
                      (dict(idx2=poke(ls["idx2"], (0, 3), ls["idx2"][1, 4])), "a keypoint of a keyframe twice")):   # item 0's kf2 is item 1's kf2
        refused(lambda: call(ls=dict(ls, **bad)), text)
    assert ls["kf2"][0] == ls["kf2"][1]
    for alloc in (-1, 121):
        refused(lambda: call(alloc=alloc), "alloc outside [0, n_mappoints]")
    for n in (-1, 9):
        refused(lambda: call(recent=np.zeros(8, np.int32), n_recent=n), "n_recent outside [0, recent_cap]")


def test_the_python_layer_checks_shapes_and_dtypes():
    t = CC.make_map(K=4, kf_cap=96, M=120, alloc=3, seed=7)
    ls = CC.make_lists(t, (20,), 64, two=True, frames=(2, 64))
    for bad_t, bad_l in ((dict(mp_bad=None), {}), (dict(mp_xw=t["mp_xw"].astype(np.float64)), {}), (dict(mp_desc=t["mp_desc"][:, :16].copy()), {}),
                         (dict(mp_obs_idx=t["mp_obs_idx"][:-1].copy()), {}), ({}, dict(xw=None)), ({}, dict(xw=ls["xw"][:, :, :2].copy())),
                         ({}, dict(idx2=ls["idx2"].astype(np.int64))), ({}, dict(n_list=np.zeros(2, np.int32)))):
        with pytest.raises(ValueError):
            CN.CreatePoints(dict(t, **bad_t), dict(ls, **bad_l), 3)
    fr, kf = CC.make_frames(F=3, kp_cap=40), CC.make_keyframes(K=5, kf_cap=44, conn_cap=6)
    it = (np.array([1], np.int32), np.array([3], np.int32), np.array([5], np.int32), np.array([.1], np.float32))
    for bad_f, bad_k in ((dict(frame_n=None), {}), (dict(kp_desc=fr["kp_desc"][:, :, :8].copy()), {}), ({}, dict(kf_pose=kf["kf_pose"][:, :9].copy())),
                         ({}, dict(kf_covis=kf["kf_covis"].astype(np.int64)))):
        with pytest.raises(ValueError):
            CN.InsertKeyFrames(dict(fr, **bad_f), dict(kf, **bad_k), *it)
    with pytest.raises(ValueError):
        CN.InsertKeyFrames(fr, kf, it[0], np.array([3, 4], np.int32), it[2], it[3])


def test_cpp_wrapper_compiles_links_and_refuses(tmp_path):
    libso = ROOT / "orb_slam2_refactored_amd" / "liborbslam2_amd.so"
    main = tmp_path / "main.cpp"
    main.write_text("int use_map_builder(); int main() { return use_map_builder(); }\n")
    exe = tmp_path / "w"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "native" / "creation_wrapper_use.cpp"), str(main), "-o", str(exe), f"-L{libso.parent}",
                    "-lorbslam2_amd", f"-Wl,-rpath,{libso.parent}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
