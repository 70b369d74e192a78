"""Every ORB_EINVAL of orbba_gba_update_map and orbba_bundle_adjustment, returned before any device call: the tests
run without a GPU (an argument that passed the checks would fail with ORB_EHIP here, not ORB_EINVAL)."""
import ctypes as C

import numpy as np
import pytest

import global_ba_cases as GC
from orb_slam2_refactored_amd._lib import BAProblem, GBAMap, GBAOptions, GBAResult, OrbError, lib
from orb_slam2_refactored_amd.optimizer import BundleAdjustment, GlobalBAUpdateMap
from orb_slam2_refactored_amd.synth import make_ba_problem

ORB_EINVAL = -1


def refused(fn, *a, **kw):
    with pytest.raises(OrbError) as e:
        fn(*a, **kw)
    assert f"status {ORB_EINVAL}:" in str(e.value), e.value
    return str(e.value)


def broken(**changes):
    m = {k: np.array(v) for k, v in GC.hand_case().items()}
    for k, f in changes.items():
        f(m[k])
    return m


def poke(i, v):
    def f(a):
        a.reshape(-1)[i] = v
    return f


@pytest.mark.parametrize("what, changes", [
    ("origin out of range", dict(origins=poke(0, 6))),
    ("origin negative", dict(origins=poke(0, -1))),
    ("child out of range", dict(kf_child_idx=poke(1, 6))),
    ("child negative", dict(kf_child_idx=poke(1, -2))),
    ("child of two parents", dict(kf_child_idx=poke(2, 1))),
    ("origin and child", dict(kf_child_idx=poke(2, 0))),
    ("offsets do not start at 0", dict(kf_child_off=poke(0, 1))),
    ("offsets decrease", dict(kf_child_off=poke(2, 0))),
    ("reference out of range", dict(mp_ref_kf=poke(0, 6))),
    ("reference negative", dict(mp_ref_kf=poke(4, -1))),
    ("NaN pose", dict(kf_pose=poke(13, np.nan))),
    ("infinite pose", dict(kf_pose=poke(70, np.inf))),
    ("NaN TcwGBA of a flagged keyframe", dict(kf_pose_gba=poke(5, np.nan))),
    ("NaN posGBA of a point in the adjustment", dict(mp_pos_gba=poke(10, np.nan))),
])
def test_update_map_refuses(what, changes):
    refused(GlobalBAUpdateMap, broken(**changes))


def test_update_map_refuses_a_repeated_origin():
    m = broken()
    m["origins"] = np.array([0, 0], np.int32)
    refused(GlobalBAUpdateMap, m)


def test_update_map_ignores_what_the_reference_never_reads():
    """A bad point's reference slot and the TcwGBA of an unflagged keyframe are not read: no ORB_EINVAL for them (the
    call then reaches the device and fails or succeeds there)."""
    m = broken(mp_ref_kf=poke(2, -1), kf_pose_gba=poke(12 * 5 + 1, np.nan))
    try:
        GlobalBAUpdateMap(m)
    except OrbError as e:
        assert f"status {ORB_EINVAL}:" not in str(e), e


def test_update_map_refuses_null_pointers_and_negative_sizes():
    m = GC.hand_case()
    keys = ("origins", "kf_child_off", "kf_child_idx", "kf_in_gba", "kf_pose", "kf_pose_gba", "kf_pose_bef", "mp_bad",
            "mp_in_gba", "mp_pos_gba", "mp_ref_kf", "mp_xw")
    ptrs = [m[k].ctypes.data for k in keys]
    assert lib().orbba_gba_update_map(None, 0) == ORB_EINVAL
    assert lib().orbba_gba_update_map_device(None, None) == ORB_EINVAL
    for i in range(len(keys)):
        p = list(ptrs)
        p[i] = None
        gm = GBAMap(6, 6, 1, *p)
        assert lib().orbba_gba_update_map(C.byref(gm), 0) == ORB_EINVAL, keys[i]
        if keys[i] != "kf_child_idx":   # (the device entry takes a null list as "no children": not called here)
            assert lib().orbba_gba_update_map_device(C.byref(gm), None) == ORB_EINVAL, keys[i]
    for sizes in ((-1, 6, 1), (6, -1, 1), (6, 6, -1)):
        gm = GBAMap(*sizes, *ptrs)
        assert lib().orbba_gba_update_map(C.byref(gm), 0) == ORB_EINVAL
        assert lib().orbba_gba_update_map_device(C.byref(gm), None) == ORB_EINVAL


def test_bundle_adjustment_refuses():
    pr = make_ba_problem(3, n_kf=5, n_pts=50, n_fixed=1)
    refused(BundleAdjustment, pr, n_iterations=-1)
    refused(BundleAdjustment, pr, n_iterations=1001)
    bad = dict(pr)
    bad["edge_point"] = np.array(pr["edge_point"], np.int32).copy()
    bad["edge_point"][7] = len(pr["points"])
    refused(BundleAdjustment, bad)
    bad = dict(pr)
    bad["edge_pose"] = np.array(pr["edge_pose"], np.int32).copy()
    bad["edge_pose"][0] = -1
    refused(BundleAdjustment, bad)
    with pytest.raises(ValueError):
        BundleAdjustment(pr, stereo_rule="other")
    with pytest.raises(ValueError):
        BundleAdjustment(dict(pr, pose_t=np.zeros((2, 3))))
    # the C entry: null arguments, an unknown rule, null result buffers
    opt, res, prob = GBAOptions(5, 1, 0), GBAResult(), BAProblem()
    assert lib().orbba_bundle_adjustment(None, C.byref(opt), C.byref(res), None, 0) == ORB_EINVAL
    assert lib().orbba_bundle_adjustment(C.byref(prob), None, C.byref(res), None, 0) == ORB_EINVAL
    assert lib().orbba_bundle_adjustment(C.byref(prob), C.byref(opt), None, None, 0) == ORB_EINVAL
    assert lib().orbba_bundle_adjustment(C.byref(prob), C.byref(opt), C.byref(res), None, 0) == ORB_EINVAL
    bad_rule = GBAOptions(5, 1, 2)
    assert lib().orbba_bundle_adjustment(C.byref(prob), C.byref(bad_rule), C.byref(res), None, 0) == ORB_EINVAL


def test_cpp_wrappers_compile(tmp_path):
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-c", f"-I{root / 'include'}",
                    str(root / "tests" / "native" / "global_ba_wrapper_use.cpp"), "-o", str(tmp_path / "w.o")], check=True)
