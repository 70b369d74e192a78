"""Frame construction (src/System.cc: UndistortKeyPoints :153-174, ComputeImageBounds :177-194, depth.convertTo +
ComputeStereoFromRGBD :515-516 / :197-219) over the gfx950 C-ABI (orbfr_*, include/orbslam2_amd.h), batched over frames: from
the extractor's (kps, counts) to the arrays tracking.py (FRAME_KEYS) and matcher.py (kp_xy, kp_octave, kp_uright, kp_angle,
bounds, kp_begin) take.

build() takes numpy arrays and is synchronous (`device=` the GPU index); build_device() takes CUDA tensors and only enqueues
(on `stream=` or torch's current stream).  kps is (F, kp_cap, 7) int32 as extract_batch_device returns it, or (F, kp_cap)
KP_DTYPE on the host.  Both return a dict of OUT_KEYS; `out=` names the arrays to write (a key left out or None is not
written; rows from frame_n[f] up keep what they held).  In STEREO kp_uright / kp_depth are never written: pass the tensors
stereo_matches_batch_device filled as out["kp_uright"] / out["kp_depth"] and they come back in the result as they are."""
import ctypes as C

import numpy as np

from ._lib import KP_DTYPE, OrbfrFrames, OrbfrInput, check, lib, stream_ptr

MONO, STEREO, RGBD = 0, 1, 2
DEPTH_U16, DEPTH_F32 = 0, 1
MAX_KP = 8192

# name: (dtype, shape); kp_un is the 28-byte record as 7 int32
OUT_KEYS = {
    "frame_n": (np.int32, ("F",)), "kp_xy": (np.float32, ("F", "kp_cap", 2)), "kp_octave": (np.int32, ("F", "kp_cap")),
    "kp_angle": (np.float32, ("F", "kp_cap")), "kp_un": (np.int32, ("F", "kp_cap", 7)), "kp_uright": (np.float32, ("F", "kp_cap")),
    "kp_depth": (np.float32, ("F", "kp_cap")), "bounds": (np.float32, ("F", 4)), "frame_mappoint": (np.int32, ("F", "kp_cap")),
    "frame_outlier": (np.uint8, ("F", "kp_cap")), "kp_begin": (np.int32, ("F1",)),
}


def _addr(a, dtype, name, want, on_device):
    """The address of `a` after checking its place, dtype, layout and shape."""
    if on_device:
        import torch
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            raise ValueError(f"{name} must be a GPU tensor")
        if a.dtype != getattr(torch, np.dtype(dtype).name) or not a.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {np.dtype(dtype).name} tensor")
        shape, address = tuple(a.shape), a.data_ptr()
    else:
        if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous:
            raise ValueError(f"{name} must be a C-contiguous numpy array of {np.dtype(dtype).name}")
        shape, address = a.shape, a.ctypes.data
    if tuple(shape) != tuple(want):
        raise ValueError(f"{name} must have shape {tuple(want)}, not {tuple(shape)}")
    return address


def _depth_fields(depth, F, rows, cols, on_device):
    """(address, type, frame stride, row step) of F depth images (F, rows, cols) with unit column stride; rows and frames
    may be padded (a view of a wider array)."""
    if on_device:
        import torch
        kinds = {torch.uint16: DEPTH_U16, torch.float32: DEPTH_F32}
        if not isinstance(depth, torch.Tensor) or not depth.is_cuda or depth.dtype not in kinds:
            raise ValueError("depth must be a uint16 or float32 GPU tensor")
        e = depth.element_size()
        shape, strides, address, kind = tuple(depth.shape), [s * e for s in depth.stride()], depth.data_ptr(), kinds[depth.dtype]
    else:
        kinds = {np.dtype(np.uint16): DEPTH_U16, np.dtype(np.float32): DEPTH_F32}
        if not isinstance(depth, np.ndarray) or depth.dtype not in kinds:
            raise ValueError("depth must be a uint16 or float32 numpy array")
        e = depth.itemsize
        shape, strides, address, kind = depth.shape, list(depth.strides), depth.ctypes.data, kinds[depth.dtype]
    if tuple(shape) != (F, rows, cols):
        raise ValueError(f"depth must have shape {(F, rows, cols)}, not {tuple(shape)}")
    if strides[2] != e or strides[1] < cols * e or strides[0] < 0:
        raise ValueError("depth must have unit column stride and rows that do not overlap")
    return address, kind, strides[0], strides[1]


def _new(F, cap, like, on_device, mode):
    d = {"F": F, "F1": F + 1, "kp_cap": cap}
    shape = lambda sp: tuple(d[s] if isinstance(s, str) else s for s in sp)   # noqa: E731
    keys = [k for k in OUT_KEYS if mode != STEREO or k not in ("kp_uright", "kp_depth")]
    if on_device:
        import torch
        return {k: torch.zeros(shape(OUT_KEYS[k][1]), dtype=getattr(torch, np.dtype(OUT_KEYS[k][0]).name), device=like.device) for k in keys}
    return {k: np.zeros(shape(OUT_KEYS[k][1]), OUT_KEYS[k][0]) for k in keys}


def _build(on_device, kps, counts, camera, dist, rows, cols, mode, depth, depth_factor, out, last):
    if not on_device and isinstance(kps, np.ndarray) and kps.dtype == KP_DTYPE:
        kps = kps.view(np.int32).reshape(kps.shape + (7,))
    if len(kps.shape) != 3:
        raise ValueError("kps must have shape (F, kp_cap, 7)")
    F, cap = int(kps.shape[0]), int(kps.shape[1])
    d = {"F": F, "F1": F + 1, "kp_cap": cap}
    head = [_addr(kps, np.int32, "kps", (F, cap, 7), on_device), _addr(counts, np.int32, "counts", (F,), on_device),
            _addr(camera, np.float32, "camera", (F, 5), on_device), _addr(dist, np.float32, "dist", (F, 5), on_device)]
    dp = (None, DEPTH_F32, 0, 0)
    if int(mode) == RGBD:
        if depth is None:
            raise ValueError("RGBD needs depth")
        dp = _depth_fields(depth, F, int(rows), int(cols), on_device)
    out = _new(F, cap, kps, on_device, int(mode)) if out is None else out
    inp = OrbfrInput(F, cap, int(rows), int(cols), int(mode), dp[1], *head, dp[0], dp[2], dp[3], float(depth_factor))
    fr = OrbfrFrames(*[None if out.get(k) is None else _addr(out[k], dt, k, tuple(d[s] if isinstance(s, str) else s for s in sp), on_device)
                       for k, (dt, sp) in OUT_KEYS.items()])
    fn = lib().orbfr_build_frames_device if on_device else lib().orbfr_build_frames
    check(fn(C.byref(inp), C.byref(fr), last), fn.__name__)
    return out


def build(kps, counts, camera, dist, rows: int, cols: int, mode: int = MONO, depth=None, depth_factor: float = 1.0,
          out: dict = None, device: int = 0) -> dict:
    """Host arrays, synchronous.  kps (F, kp_cap, 7) int32 or (F, kp_cap) KP_DTYPE, counts (F,) int32 in [0, kp_cap], camera
    (F, 5) float32 = fx, fy, cx, cy, bf, dist (F, 5) float32 = k1, k2, p1, p2, k3; depth (RGBD): (F, rows, cols) uint16 or
    float32, rows and frames may be padded.  Returns the dict of OUT_KEYS."""
    return _build(False, kps, counts, camera, dist, rows, cols, mode, depth, depth_factor, out, int(device))


def build_device(kps, counts, camera, dist, rows: int, cols: int, mode: int = MONO, depth=None, depth_factor: float = 1.0,
                 out: dict = None, stream=None) -> dict:
    """CUDA tensors of the same shapes; one launch enqueued on `stream`, nothing is read back.  kps / counts are
    extract_batch_device's; a count outside [0, kp_cap] is clamped."""
    return _build(True, kps, counts, camera, dist, rows, cols, mode, depth, depth_factor, out, stream_ptr(stream))


def image_bounds(rows: int, cols: int, camera, dist) -> np.ndarray:
    """ComputeImageBounds on the CPU (the reference computes it once per run): (minx, maxx, miny, maxy) float32."""
    cam, ds = np.ascontiguousarray(camera, np.float32).reshape(-1), np.ascontiguousarray(dist, np.float32).reshape(-1)
    if len(cam) < 4 or len(ds) not in (4, 5):
        raise ValueError("camera needs fx, fy, cx, cy and dist 4 or 5 coefficients")
    ds = np.concatenate([ds, np.zeros(5 - len(ds), np.float32)])
    b = np.zeros(4, np.float32)
    check(lib().orbfr_image_bounds(int(rows), int(cols), cam.ctypes.data, ds.ctypes.data, b.ctypes.data), "orbfr_image_bounds")
    return b


def undistort_points(camera, dist, xy) -> np.ndarray:
    """UndistortKeyPoints on the CPU for (n, 2) float32 points."""
    cam, ds = np.ascontiguousarray(camera, np.float32).reshape(-1), np.ascontiguousarray(dist, np.float32).reshape(-1)
    if len(cam) < 4 or len(ds) not in (4, 5):
        raise ValueError("camera needs fx, fy, cx, cy and dist 4 or 5 coefficients")
    ds = np.concatenate([ds, np.zeros(5 - len(ds), np.float32)])
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    o = np.zeros_like(xy)
    check(lib().orbfr_undistort_points(cam.ctypes.data, ds.ctypes.data, xy.ctypes.data, len(xy), o.ctypes.data), "orbfr_undistort_points")
    return o
