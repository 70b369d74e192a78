"""The argument checks of orbfr_build_frames: each returns ORB_EINVAL before anything is copied, so none of this needs a GPU
(a call that passed its checks would fail later, on the device it names).  The new symbols are exported and bound, and the
C++ FrameBuilder compiles, links and refuses.  CPU only."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import frame_ref as R
from orb_slam2_refactored_amd import _lib
from orb_slam2_refactored_amd import frame as FR

EINVAL = -1
f32 = np.float32
ROOT = Path(__file__).resolve().parents[1]


def arrays(F=2, cap=6, rows=8, cols=10, dtype=np.uint16):
    a = dict(kps=np.zeros((F, cap, 7), np.int32), counts=np.full(F, cap - 1, np.int32), camera=np.stack([R.TUM1_CAMERA] * F),
             dist=np.stack([R.TUM1_DIST] * F), depth=np.ones((F, rows, cols), dtype))
    out = {k: np.zeros(tuple({"F": F, "F1": F + 1, "kp_cap": cap}.get(s, s) for s in sp), dt) for k, (dt, sp) in FR.OUT_KEYS.items()}
    return a, out


def call(a, out, rows=8, cols=10, mode=FR.RGBD, **kw):
    return FR.build(a["kps"], a["counts"], a["camera"], a["dist"], rows, cols, mode, depth=a["depth"], out=out, **kw)


def rejected(fn, *a, **kw):
    with pytest.raises(_lib.OrbError, match="status -1"):
        fn(*a, **kw)


def test_the_new_symbols_are_exported_and_bound():
    L = _lib.lib()
    for name in ("orbfr_build_frames", "orbfr_build_frames_device", "orbfr_image_bounds", "orbfr_undistort_points"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    import orb_slam2_refactored_amd as pkg
    assert pkg.frame is FR and callable(FR.build) and callable(FR.build_device)
    assert (FR.MONO, FR.STEREO, FR.RGBD) == (R.MONO, R.STEREO, R.RGBD)
    # the names tracking.py and matcher.py take
    from orb_slam2_refactored_amd import tracking as T
    assert {k for k in FR.OUT_KEYS if k not in ("kp_un", "kp_begin")} <= set(T.FRAME_KEYS)
    for k in FR.OUT_KEYS:
        if k in T.FRAME_KEYS:
            assert FR.OUT_KEYS[k] == T.FRAME_KEYS[k], k


def test_counts_outside_the_row_are_rejected():
    for bad in (-1, 7):
        a, out = arrays()
        a["counts"][1] = bad
        rejected(call, a, out)
        rejected(call, a, out, mode=FR.MONO)


def test_sizes_modes_and_caps_are_rejected():
    a, out = arrays()
    for rows, cols in ((0, 10), (8, 0), (-1, 10)):
        rejected(call, a, out, rows=rows, cols=cols, mode=FR.MONO)
    for mode in (-1, 3):
        rejected(call, a, out, mode=mode)
    a, out = arrays(F=1, cap=FR.MAX_KP + 1)
    rejected(call, a, out, mode=FR.MONO)


def raw(a, out, **kw):
    """The host entry through ctypes with every field settable."""
    F, cap = a["kps"].shape[:2]
    d = a["depth"]
    p = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    fields = dict(n_frames=F, kp_cap=cap, rows=8, cols=10, mode=FR.RGBD, depth_type=FR.DEPTH_U16, kps=p(a["kps"]), counts=p(a["counts"]),
                  camera=p(a["camera"]), dist=p(a["dist"]), depth=p(d), depth_frame_stride=d.strides[0], depth_step=d.strides[1],
                  depth_factor=0.0002)
    fields.update(kw)
    inp = _lib.OrbfrInput(**fields)
    fr = _lib.OrbfrFrames(**{k: p(v) for k, v in out.items()})
    return inp, fr


def test_null_arrays_negative_sizes_and_the_depth_layout_through_the_raw_entry():
    L = _lib.lib()
    a, out = arrays()
    bad = [dict(kps=None), dict(counts=None), dict(camera=None), dict(dist=None), dict(depth=None), dict(n_frames=-1),
           dict(n_frames=65536), dict(kp_cap=0), dict(kp_cap=-3), dict(kp_cap=FR.MAX_KP + 1), dict(rows=0), dict(cols=0), dict(mode=3),
           dict(depth_type=2), dict(depth_type=-1),
           dict(depth_step=18),                          # below cols * 2
           dict(depth_step=21),                          # not a multiple of the element size
           dict(depth_type=FR.DEPTH_F32, depth_step=38),  # below cols * 4
           dict(depth_type=FR.DEPTH_F32, depth_step=42, depth_frame_stride=400),
           dict(depth_frame_stride=161),                 # not a multiple of the element size
           dict(depth_frame_stride=100),                 # shorter than a frame
           dict(depth=a["depth"].ctypes.data + 1)]       # not aligned to its element
    for kw in bad:
        inp, fr = raw(a, out, **kw)
        assert L.orbfr_build_frames(C.byref(inp), C.byref(fr), 0) == EINVAL, kw
        if "depth" not in kw or kw["depth"] is None:   # (the device entry makes the same checks: no launch follows)
            assert L.orbfr_build_frames_device(C.byref(inp), C.byref(fr), None) == EINVAL, kw
    inp, fr = raw(a, out)
    assert L.orbfr_build_frames(None, C.byref(fr), 0) == EINVAL and L.orbfr_build_frames(C.byref(inp), None, 0) == EINVAL
    # outside RGBD the depth fields are not looked at
    a["counts"][0] = 99
    inp, fr = raw(a, out, mode=FR.MONO, depth=None, depth_type=7, depth_step=0)
    assert L.orbfr_build_frames(C.byref(inp), C.byref(fr), 0) == EINVAL   # ... and the count is what is left to refuse
    assert b"counts" in L.orb_last_error()
    # no frames: nothing to do, whatever the pointers
    inp, fr = raw(a, out, n_frames=0, kps=None, counts=None, depth=None)
    assert L.orbfr_build_frames(C.byref(inp), C.byref(fr), 0) == 0
    # the CPU functions
    b = np.zeros(4, f32)
    cam, ds = R.TUM1_CAMERA, R.TUM1_DIST
    assert L.orbfr_image_bounds(0, 640, cam.ctypes.data, ds.ctypes.data, b.ctypes.data) == EINVAL
    assert L.orbfr_image_bounds(480, 640, None, ds.ctypes.data, b.ctypes.data) == EINVAL
    assert L.orbfr_undistort_points(cam.ctypes.data, ds.ctypes.data, None, 3, None) == EINVAL
    assert L.orbfr_undistort_points(cam.ctypes.data, ds.ctypes.data, None, -1, None) == EINVAL
    assert L.orbfr_undistort_points(cam.ctypes.data, ds.ctypes.data, None, 0, None) == 0


def test_the_python_layer_checks_shapes_and_dtypes():
    a, out = arrays()
    with pytest.raises(ValueError):
        call(dict(a, counts=a["counts"].astype(np.int64)), out)
    with pytest.raises(ValueError):
        call(dict(a, camera=a["camera"][:, :4].copy()), out)
    with pytest.raises(ValueError):
        call(dict(a, depth=a["depth"].astype(np.float64)), out)
    with pytest.raises(ValueError):
        call(dict(a, depth=a["depth"][:, :, ::2]), out, cols=5)
    with pytest.raises(ValueError):
        call(dict(a, depth=None), out)
    with pytest.raises(ValueError):
        call(a, dict(out, kp_xy=np.zeros((2, 6), f32)))
    with pytest.raises(ValueError):
        call(a, dict(out, kp_un=np.zeros((2, 5, 7), np.int32)))


def test_cpp_wrapper_compiles_links_and_refuses(tmp_path):
    libso = ROOT / "orb_slam2_refactored_amd" / "liborbslam2_amd.so"
    main = tmp_path / "main.cpp"
    main.write_text("int use_frame_builder(); int main() { return use_frame_builder(); }\n")
    exe = tmp_path / "w"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "native" / "frame_wrapper_use.cpp"), str(main), "-o", str(exe), f"-L{libso.parent}",
                    "-lorbslam2_amd", f"-Wl,-rpath,{libso.parent}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
