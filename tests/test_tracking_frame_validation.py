"""The argument checks of the orbtf_* host entries: each returns ORB_EINVAL before anything is copied, so none of this needs
a GPU (a call that passed its checks would fail later, on the device it names).  CPU only."""
import ctypes as C

import numpy as np
import pytest

from orb_slam2_refactored_amd import _lib
from orb_slam2_refactored_amd import tracking as T

EINVAL = -1
f32 = np.float32


def tables(F=2, cap=6, M=4, K=2, kf_cap=3):
    fr = dict(frame_n=np.full(F, cap - 1, np.int32), frame_mappoint=np.full((F, cap), -1, np.int32),
              frame_outlier=np.zeros((F, cap), np.uint8), pose=np.zeros((F, 12), f32), camera=np.ones((F, 5), f32),
              bounds=np.zeros((F, 4), f32), kp_xy=np.zeros((F, cap, 2), f32), kp_octave=np.zeros((F, cap), np.int32),
              kp_uright=np.zeros((F, cap), f32), kp_depth=np.ones((F, cap), f32), kp_angle=np.zeros((F, cap), f32),
              kp_desc=np.zeros((F, cap, 32), np.uint8))
    fr["frame_mappoint"][:, 0] = M - 1
    m = dict(mp_xw=np.zeros((M, 3), f32), mp_bad=np.zeros(M, np.uint8), mp_nobs=np.ones(M, np.int32), mp_found=np.zeros(M, np.int32),
             mp_replaced=np.full(M, -1, np.int32), mp_desc=np.zeros((M, 32), np.uint8), kf_n=np.full(K, kf_cap, np.int32),
             kf_mappoint=np.full((K, kf_cap), -1, np.int32))
    return fr, m


def edges(F=2, cap=6):
    return dict(edge_begin=np.array([0, 1, 2], np.int32)[:F + 1], edge_kp=np.zeros(F * cap, np.int32))


def result(F=2, cap=6):
    return dict(pose_R=np.zeros((F, 9)), pose_t=np.zeros((F, 3)), outlier=np.zeros(F * cap, np.uint8))


def calls():
    """name -> a function(fr, m, **changes) that makes the host call with otherwise valid arguments."""
    km, src = np.full((2, 6), -1, np.int32), np.full((2, 5), -1, np.int32)
    one = lambda v, dt: np.full(2, v, dt)   # noqa: E731
    return {
        "apply_matches": lambda fr, m, **kw: T.apply_matches(fr, kw.get("mode", T.MERGE), kw.get("kp_match", km), kw.get("src", src), 4,
                                                             src_row=kw.get("src_row")),
        "pose_edges": lambda fr, m, **kw: T.pose_edges(fr, m, kw.get("table", np.ones(3, f32))),
        "finish_pose": lambda fr, m, **kw: T.finish_pose(fr, m, kw.get("mode", T.DISCARD), kw.get("edges", edges()), result(cap=8)),
        "motion_project": lambda fr, m, **kw: T.motion_project(fr, kw.get("last", tables()[0]), m, np.zeros((2, 12), f32), one(0.1, f32), False),
        "end_frame": lambda fr, m, **kw: T.end_frame(fr, m, 8.0, kw.get("reference_kf", one(-1, np.int32)), one(2, np.int32)),
        "drop_outliers": lambda fr, m, **kw: T.drop_outliers(fr),
        "stereo_points": lambda fr, m, **kw: T.stereo_points(fr, m, kw.get("mode", T.KEYFRAME), 8.0),
    }


def rejected(fn, *a, **kw):
    with pytest.raises(_lib.OrbError, match="status -1"):
        fn(*a, **kw)


USES_MAP_SLOTS = ("apply_matches", "pose_edges", "finish_pose", "end_frame", "stereo_points")


@pytest.mark.parametrize("name", list(calls()))
def test_frame_n_outside_its_row_is_rejected(name):
    for bad in (-1, 7):
        fr, m = tables()
        fr["frame_n"][1] = bad
        rejected(calls()[name], fr, m)


@pytest.mark.parametrize("name", USES_MAP_SLOTS + ("motion_project",))
def test_a_map_point_slot_outside_the_table_is_rejected(name):
    for bad in (-2, 4):
        fr, m = tables()
        if name == "motion_project":   # the slots it reads are the last frames'
            last = tables()[0]
            last["frame_mappoint"][1, 2] = bad
            rejected(calls()[name], fr, m, last=last)
        else:
            fr["frame_mappoint"][1, 2] = bad
            rejected(calls()[name], fr, m)


@pytest.mark.parametrize("name", ["apply_matches", "pose_edges", "drop_outliers", "stereo_points"])   # (the others: the raw calls below)
def test_kp_cap_above_the_limit_is_rejected(name):
    fr, m = tables(F=1, cap=T.MAX_KP + 1)
    kw = dict(kp_match=np.full((1, T.MAX_KP + 1), -1, np.int32)) if name == "apply_matches" else {}
    rejected(calls()[name], fr, m, **kw)


def test_unknown_modes_are_rejected():
    fr, m = tables()
    for name in ("apply_matches", "finish_pose", "stereo_points"):
        for mode in (-1, 3):
            rejected(calls()[name], fr, m, mode=mode)


def test_the_other_slots_and_the_octave():
    c = calls()
    fr, m = tables()
    km = np.full((2, 6), -1, np.int32)
    km[0, 1] = 5
    rejected(c["apply_matches"], fr, m, kp_match=km)                       # kp_match outside [-1, src_cap)
    src = np.full((2, 5), -1, np.int32)
    src[1, 1] = 4
    rejected(c["apply_matches"], fr, m, src=src)                           # a source slot outside [-1, n_mappoints)
    rejected(c["apply_matches"], fr, m, src_row=np.array([0, 2], np.int32))
    rejected(c["apply_matches"], fr, m, src=np.full((1, 5), -1, np.int32))   # fewer rows than frames, no src_row
    for bad in (-1, 3):
        fr, m = tables()
        fr["kp_octave"][0, 2] = bad
        rejected(c["pose_edges"], fr, m)
    fr, m = tables()
    fr["kp_octave"][0, 5] = 9                                              # the padding is not read
    rejected(c["pose_edges"], fr, m, table=np.ones(33, f32))               # n_levels above ORBTF_MAX_LEVELS
    fr, m = tables()
    rejected(c["end_frame"], fr, m, reference_kf=np.array([0, 2], np.int32))
    m["kf_n"][1] = 4
    rejected(c["end_frame"], fr, m)
    fr, m = tables()
    m["kf_mappoint"][1, 1] = 4
    rejected(c["end_frame"], fr, m)
    fr, m = tables()
    m["mp_replaced"][2] = 4
    rejected(c["motion_project"], fr, m)
    fr, m = tables()
    rejected(c["finish_pose"], fr, m, edges=dict(edges(), edge_begin=np.array([0, 2, 1], np.int32)))
    rejected(c["finish_pose"], fr, m, edges=dict(edges(), edge_begin=np.array([1, 1, 2], np.int32)))
    rejected(c["finish_pose"], fr, m, edges=dict(edges(), edge_begin=np.array([0, 1, 13], np.int32)))
    e = edges()
    e["edge_kp"][1] = 6
    rejected(c["finish_pose"], fr, m, edges=e)
    rejected(c["motion_project"], fr, m, last=tables(F=2, cap=T.MAX_KP + 1)[0])


def test_null_arrays_negative_sizes_and_caps_through_the_raw_entries():
    L = _lib.lib()
    fr, m = tables()
    d = T._dims(fr, m)

    def frames(**kw):
        s = T._frames(fr, d, False)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def the_map(**kw):
        s = T._map(m, d, False)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    a = lambda x: x.ctypes.data   # noqa: E731
    km, src = np.full((2, 6), -1, np.int32), np.full((2, 5), -1, np.int32)
    ok_map = the_map()
    for bad in (frames(frame_n=None), frames(frame_mappoint=None), frames(n_frames=-1), frames(kp_cap=0), frames(kp_cap=T.MAX_KP + 1),
                frames(n_frames=65536)):
        assert L.orbtf_apply_matches(C.byref(bad), T.MERGE, a(km), a(src), 2, 5, None, 4, 0) == EINVAL
        assert L.orbtf_drop_outliers(C.byref(bad), 0) == EINVAL
        assert L.orbtf_end_frame(C.byref(bad), C.byref(ok_map), 8.0, a(km), a(km), a(km), a(km), 0) == EINVAL
    good = frames()
    assert L.orbtf_apply_matches(None, T.MERGE, a(km), a(src), 2, 5, None, 4, 0) == EINVAL
    assert L.orbtf_apply_matches(C.byref(good), T.MERGE, None, a(src), 2, 5, None, 4, 0) == EINVAL
    assert L.orbtf_apply_matches(C.byref(good), T.MERGE, a(km), None, 2, 5, None, 4, 0) == EINVAL
    assert L.orbtf_apply_matches(C.byref(good), T.MERGE, a(km), a(src), -1, 5, None, 4, 0) == EINVAL
    assert L.orbtf_apply_matches(C.byref(good), T.MERGE, a(km), a(src), 2, 0, None, 4, 0) == EINVAL
    assert L.orbtf_apply_matches(C.byref(good), T.MERGE, a(km), a(src), 2, 5, None, -1, 0) == EINVAL
    assert L.orbtf_drop_outliers(C.byref(frames(frame_outlier=None)), 0) == EINVAL
    e = T._fill(_lib.OrbtfEdges, (), T.EDGE_KEYS, T._new(T.EDGE_KEYS, d, fr["frame_n"], None), d, False)
    table = np.ones(3, f32)
    assert L.orbtf_pose_edges(C.byref(good), C.byref(the_map(mp_xw=None)), a(table), 3, C.byref(e), 0) == EINVAL
    assert L.orbtf_pose_edges(C.byref(good), C.byref(the_map(n_mappoints=-1)), a(table), 3, C.byref(e), 0) == EINVAL
    assert L.orbtf_pose_edges(C.byref(good), C.byref(ok_map), None, 3, C.byref(e), 0) == EINVAL
    assert L.orbtf_pose_edges(C.byref(good), C.byref(ok_map), a(table), 0, C.byref(e), 0) == EINVAL
    assert L.orbtf_pose_edges(C.byref(good), C.byref(ok_map), a(table), 3, None, 0) == EINVAL
    assert L.orbtf_pose_edges(C.byref(frames(kp_uright=None)), C.byref(ok_map), a(table), 3, C.byref(e), 0) == EINVAL
    no_kp = _lib.OrbtfEdges()
    assert L.orbtf_pose_edges(C.byref(good), C.byref(ok_map), a(table), 3, C.byref(no_kp), 0) == EINVAL
    r = T._fill(_lib.PoseResult, (), T.RESULT_KEYS, result(), d, False)
    n = np.zeros(12, np.int32)
    assert L.orbtf_finish_pose(C.byref(good), C.byref(ok_map), T.DISCARD, C.byref(e), C.byref(r), 0, 0, a(n), None, a(n), 0) == EINVAL
    assert L.orbtf_finish_pose(C.byref(good), C.byref(ok_map), T.LOCAL_MAP, C.byref(e), C.byref(r), 0, 0, None, None, None, 0) == EINVAL
    assert L.orbtf_finish_pose(C.byref(good), C.byref(the_map(mp_found=None)), T.LOCAL_MAP, C.byref(e), C.byref(r), 0, 0, a(n), None, None, 0) == EINVAL
    assert L.orbtf_finish_pose(C.byref(frames(kp_cap=T.MAX_KP + 1)), C.byref(ok_map), T.DISCARD, C.byref(e), C.byref(r), 0, 0, a(n), a(n), a(n), 0) == EINVAL
    assert L.orbtf_end_frame(C.byref(good), C.byref(the_map(kf_cap=0)), 8.0, a(km), a(km), a(km), a(km), 0) == EINVAL
    assert L.orbtf_end_frame(C.byref(good), C.byref(the_map(kf_n=None)), 8.0, a(km), a(km), a(km), a(km), 0) == EINVAL
    assert L.orbtf_end_frame(C.byref(good), C.byref(ok_map), 8.0, None, a(km), a(km), a(km), 0) == EINVAL
    mo = T._fill(_lib.OrbtfMotion, (), T.MOTION_KEYS, T._new(T.MOTION_KEYS, dict(d, last_cap=6), fr["frame_n"], None), dict(d, last_cap=6), False)
    vel = np.zeros((2, 12), f32)
    assert L.orbtf_motion_project(C.byref(good), C.byref(frames(n_frames=1)), C.byref(ok_map), a(vel), a(vel), 0, C.byref(mo), 0) == EINVAL
    assert L.orbtf_motion_project(C.byref(good), C.byref(good), C.byref(ok_map), None, a(vel), 0, C.byref(mo), 0) == EINVAL
    assert L.orbtf_motion_project(C.byref(good), C.byref(frames(kp_angle=None)), C.byref(ok_map), a(vel), a(vel), 0, C.byref(mo), 0) == EINVAL
    assert L.orbtf_motion_project(C.byref(good), C.byref(good), C.byref(the_map(mp_replaced=None)), a(vel), a(vel), 0, C.byref(mo), 0) == EINVAL
    assert L.orbtf_motion_project(C.byref(good), C.byref(good), C.byref(ok_map), a(vel), a(vel), 0, None, 0) == EINVAL
    cr = T._fill(_lib.OrbtfCreated, (), T.CREATED_KEYS, T._new(T.CREATED_KEYS, d, fr["frame_n"], None), d, False)
    assert L.orbtf_stereo_points(C.byref(frames(kp_depth=None)), C.byref(ok_map), T.KEYFRAME, 8.0, C.byref(cr), 0) == EINVAL
    assert L.orbtf_stereo_points(C.byref(good), C.byref(the_map(mp_nobs=None)), T.KEYFRAME, 8.0, C.byref(cr), 0) == EINVAL
    assert L.orbtf_stereo_points(C.byref(good), C.byref(ok_map), T.KEYFRAME, 8.0, None, 0) == EINVAL
    assert L.orbtf_stereo_points(C.byref(good), C.byref(ok_map), T.KEYFRAME, 8.0, C.byref(_lib.OrbtfCreated()), 0) == EINVAL
    # the device entries make the checks that need no device read (no launch follows a rejection)
    assert L.orbtf_apply_matches_device(C.byref(frames(kp_cap=0)), T.MERGE, a(km), a(src), 2, 5, None, 4, None) == EINVAL
    assert L.orbtf_stereo_points_device(C.byref(good), C.byref(ok_map), 7, 8.0, C.byref(cr), None) == EINVAL
    assert L.orbtf_pose_edges_device(C.byref(frames(kp_cap=T.MAX_KP + 1)), C.byref(ok_map), a(table), 3, C.byref(e), None) == EINVAL


def test_cpp_wrapper_compiles_links_and_refuses(tmp_path):
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    libso = root / "orb_slam2_refactored_amd" / "liborbslam2_amd.so"
    main = tmp_path / "main.cpp"
    main.write_text("int use_tracking_frames(); int main() { return use_tracking_frames(); }\n")
    exe = tmp_path / "w"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", f"-I{root / 'include'}",
                    str(root / "tests" / "native" / "tracking_frame_wrapper_use.cpp"), str(main), "-o", str(exe), f"-L{libso.parent}",
                    "-lorbslam2_amd", f"-Wl,-rpath,{libso.parent}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
