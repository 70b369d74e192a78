"""Argument validation of the CreateNewMapPoints entries: ORB_EINVAL with a message from the C ABI (no device call is
reached), ValueError from the Python wrappers.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from orb_slam2_refactored_amd import mapping
from orb_slam2_refactored_amd._lib import OrbError, OrblmBatch, OrblmPairs, OrblmPoints, TriBatch, lib
from orb_slam2_refactored_amd.synth import make_new_points_batch


def batch():
    return make_new_points_batch(1, n_kf1=2, n_rounds=2, cap=65, mode="mixed")


def flat(b):
    return dict(b, frame1=b["frame1"].reshape(-1), frame2=b["frame2"].reshape(-1))


def last_error():
    return lib().orb_last_error().decode()


def test_python_wrappers_refuse_wrong_shapes_and_dtypes():
    b = flat(batch())
    with pytest.raises(ValueError, match="pose1"):
        mapping.PreparePairs(dict(b, pose1=b["pose1"][:, :9]))
    with pytest.raises(ValueError, match="kps1"):
        mapping.PreparePairs(dict(b, kps1=np.zeros((8, 65, 6), np.float32)))
    with pytest.raises(ValueError, match="go together"):
        mapping.PreparePairs(dict(b, depth1=None))
    with pytest.raises(ValueError, match="one shape"):
        mapping.PreparePairs(dict(b, frame2=b["frame2"][:-1]))
    with pytest.raises(ValueError, match="monocular"):
        mapping.PreparePairs(dict(b, monocular=True, mp_xw2=None))
    with pytest.raises(ValueError, match="ORBM_TRI_MAX_LEVELS"):
        mapping.PreparePairs(dict(b, scale_factors2=np.ones(33, np.float32), sigma2_2=np.ones(33, np.float32)))
    pairs = {k: np.zeros((4, w), dt) for k, dt, w in mapping._PAIRS}
    with pytest.raises(ValueError, match="match12"):
        mapping.TriangulateMatches(b, pairs, np.zeros((4, 64), np.int32))
    with pytest.raises(ValueError, match="has_mappoint1"):
        mapping.TriangulateMatches(b, pairs, np.zeros((4, 65), np.int32), has_mappoint1=np.zeros((8, 65), np.int32))
    with pytest.raises(ValueError, match="GPU tensor"):
        mapping.prepare_pairs_device(b)   # host arrays to the device form


def test_a_round_with_a_repeated_keyframe_is_refused():
    b = batch()
    flags = b["has_mappoint"].copy()
    search = dict(desc1=b["desc"], desc2=b["desc"])
    f1 = b["frame1"].copy()
    f1[1, 1] = f1[1, 0]
    with pytest.raises(ValueError, match="twice"):
        mapping.CreateNewMapPoints(dict(b, frame1=f1), search, flags, flags)
    f2 = b["frame2"].copy()
    f2[0, 1] = b["frame1"][0, 0]   # a keyframe 1 of the round as somebody's keyframe 2, in one slot set
    with pytest.raises(ValueError, match="as keyframe 1 and as keyframe 2"):
        mapping.CreateNewMapPoints(dict(b, frame2=f2), search, flags, flags)
    mapping.check_plan(b["frame1"], b["frame2"], True)
    mapping.check_plan(np.array([[0, -1]]), np.array([[1, -1]]), True)   # "no pair" entries are free


def c_structs(b, keep, n_levels=8):
    kps = np.ascontiguousarray(b["kps1"])
    arrs = {k: np.ascontiguousarray(b[k]) for k in ("counts1", "uright1", "depth1", "has_mappoint2", "mp_xw2", "pose1", "camera1")}
    f1, f2 = (np.ascontiguousarray(b[k].reshape(-1)) for k in ("frame1", "frame2"))
    tab = np.ones(64, np.float32)
    keep += [kps, arrs, f1, f2, tab]
    p = lambda a: a.ctypes.data   # noqa: E731
    lb = OrblmBatch(2, 65, 65, 6, 6, p(kps), p(arrs["counts1"]), p(arrs["uright1"]), p(arrs["depth1"]), p(kps), p(arrs["counts1"]),
                    p(arrs["uright1"]), p(arrs["depth1"]), p(arrs["has_mappoint2"]), p(arrs["mp_xw2"]), p(arrs["pose1"]),
                    p(arrs["pose1"]), p(arrs["camera1"]), p(arrs["camera1"]), p(f1), p(f2), n_levels, p(tab), p(tab), p(tab), p(tab),
                    1.2, 0)
    n = 4
    pa = {k: np.zeros(n * w, dt) for k, dt, w in mapping._PAIRS}
    po = {k: np.zeros(n * 65 * w, dt) for k, dt, w in mapping._POINTS}
    nc, flags = np.zeros(n, np.int32), np.ascontiguousarray(b["has_mappoint"].copy())
    keep += [pa, po, nc, flags]
    pairs = OrblmPairs(*[p(pa[k]) for k, _, _ in mapping._PAIRS])
    pts = OrblmPoints(*[p(po[k]) for k, _, _ in mapping._POINTS], p(nc), p(flags), p(flags))
    desc = np.ascontiguousarray(b["desc"])
    keep.append(desc)
    s = TriBatch()
    s.desc1 = s.desc2 = p(desc)
    return lb, pairs, pts, s


def test_c_entries_return_einval_with_a_message():
    b = batch()
    keep = []
    L = lib()
    m12, nm = np.full(4 * 65, -1, np.int32), np.zeros(4, np.int32)
    lb, pairs, pts, s = c_structs(b, keep)
    assert L.orblm_prepare_pairs(None, C.byref(pairs), 0) == -1 and "null" in last_error()
    assert L.orblm_prepare_pairs_device(C.byref(lb), None, None) == -1 and "null" in last_error()
    lb, pairs, pts, s = c_structs(b, keep, n_levels=33)
    for rc in (L.orblm_prepare_pairs(C.byref(lb), C.byref(pairs), 0), L.orblm_prepare_pairs_device(C.byref(lb), C.byref(pairs), None),
               L.orblm_triangulate(C.byref(lb), C.byref(pairs), m12.ctypes.data, C.byref(pts), 0),
               L.orblm_create_new_map_points(C.byref(lb), C.byref(s), 2, C.byref(pairs), C.byref(pts), m12.ctypes.data, nm.ctypes.data, 0)):
        assert rc == -1 and "n_levels" in last_error()
    lb, pairs, pts, s = c_structs(b, keep)
    pairs.F12 = None
    assert L.orblm_prepare_pairs(C.byref(lb), C.byref(pairs), 0) == -1 and "null pair array" in last_error()
    lb, pairs, pts, s = c_structs(b, keep)
    pts.status = None
    assert L.orblm_triangulate(C.byref(lb), C.byref(pairs), m12.ctypes.data, C.byref(pts), 0) == -1 and "null output" in last_error()
    assert L.orblm_triangulate_device(C.byref(lb), C.byref(pairs), m12.ctypes.data, C.byref(pts), None) == -1
    lb, pairs, pts, s = c_structs(b, keep)
    assert L.orblm_triangulate(C.byref(lb), C.byref(pairs), None, C.byref(pts), 0) == -1 and "match12" in last_error()
    pts.has_mappoint1 = None
    assert L.orblm_create_new_map_points_device(C.byref(lb), C.byref(s), 2, C.byref(pairs), C.byref(pts), m12.ctypes.data,
                                                nm.ctypes.data, None) == -1 and "writable" in last_error()
    lb, pairs, pts, s = c_structs(b, keep)
    lb.cap1 = 0
    assert L.orblm_prepare_pairs(C.byref(lb), C.byref(pairs), 0) == -1 and "capacities" in last_error()
    lb, pairs, pts, s = c_structs(b, keep)
    f1 = np.ascontiguousarray(b["frame1"].reshape(-1).copy())
    f1[3] = f1[2]
    lb.frame1 = f1.ctypes.data
    assert L.orblm_create_new_map_points(C.byref(lb), C.byref(s), 2, C.byref(pairs), C.byref(pts), m12.ctypes.data, nm.ctypes.data,
                                         0) == -1 and "twice" in last_error()
    lb, pairs, pts, s = c_structs(b, keep)
    cnt = np.ascontiguousarray(b["counts1"].copy())
    cnt[0] = 66
    lb.counts1 = cnt.ctypes.data
    assert L.orblm_prepare_pairs(C.byref(lb), C.byref(pairs), 0) == -1 and "counts1" in last_error()


def test_cpp_wrapper_compiles_links_and_refuses(tmp_path):
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    libso = root / "orb_slam2_refactored_amd" / "liborbslam2_amd.so"
    main = tmp_path / "main.cpp"
    main.write_text("int use_new_points(); int main() { return use_new_points(); }\n")
    exe = tmp_path / "w"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", f"-I{root / 'include'}", str(root / "tests" / "native" / "newpoints_wrapper_use.cpp"),
                    str(main), "-o", str(exe), f"-L{libso.parent}", "-lorbslam2_amd", f"-Wl,-rpath,{libso.parent}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
