"""Initializer (include/Initializer.h, src/Initializer.cc): the H / F RANSAC and reconstruction of
Tracking::MonocularInitialization, batched over (reference frame, current frame) pairs (orb_initializer_batch in
include/orbslam2_amd.h).

    InitializerInitialize(batch, device=0)                        host arrays, synchronous
    initializer_initialize_device(batch, out=None, stream=None)   GPU tensors, enqueue only
    make_draws(n_pairs, max_iterations, seed)                     the rand() table both read

`batch` holds kp1_begin, kp2_begin, kp1_xy, kp2_xy (keypointsUn of the reference and the current frame), matches12
(what SearchForInitialization / search_for_initialization_device return), camera (fx, fy, cx, cy per pair), draws and
the scalars sigma (1.0), max_iterations (200), min_parallax (1.0), min_triangulated (50), rh_threshold (0.40) and
rand_max (2147483647)."""
import ctypes as C

import numpy as np

from ._lib import InitializerBatch, InitializerResult, check, lib, ptr, stream_ptr, tptr
from .optimizer import _need

RAND_MAX = 2147483647   # glibc
DEFAULTS = dict(sigma=1.0, max_iterations=200, min_parallax=1.0, min_triangulated=50, rh_threshold=0.40, rand_max=RAND_MAX)

# orb_initializer_batch arrays in struct order: name -> (dtype, rows, row width)
_KEYS = (("kp1_begin", np.int32, "F1", 1), ("kp2_begin", np.int32, "F1", 1), ("kp1_xy", np.float32, "K1", 2),
         ("kp2_xy", np.float32, "K2", 2), ("matches12", np.int32, "K1", 1), ("camera", np.float32, "F", 4),
         ("draws", np.int32, "D", 8))
# orb_initializer_result arrays in struct order: name -> (numpy dtype, rows, row width)
_OUT = (("found", np.int32, "F", 1), ("model", np.int32, "F", 1), ("r21t21", np.float32, "F", 12),
        ("p3d", np.float32, "K1", 3), ("triangulated", np.uint8, "K1", 1), ("score_h", np.float32, "F", 1),
        ("score_f", np.float32, "F", 1), ("best_h", np.int32, "F", 1), ("best_f", np.int32, "F", 1),
        ("h21", np.float32, "F", 9), ("f21", np.float32, "F", 9), ("inlier_h", np.uint8, "K1", 1),
        ("inlier_f", np.uint8, "K1", 1), ("hyp_score", np.float32, "F", None), ("n_good", np.int32, "F", 8),
        ("parallax", np.float32, "F", 8))


def make_draws(n_pairs: int, max_iterations: int, seed: int = 0, rand_max: int = RAND_MAX) -> np.ndarray:
    """(n_pairs, max_iterations, 8) int32 values uniform in [0, rand_max]: what rand() would have returned for the
    eight draws of every hypothesis of every pair."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, int(rand_max) + 1, (n_pairs, max_iterations, 8), dtype=np.int64).astype(np.int32)


def _params(batch):
    return {k: batch[k] if batch.get(k) is not None else v for k, v in DEFAULTS.items()}


def _struct(batch, conv, F, K1, K2, what):
    prm = _params(batch)
    for k, _, _, _ in _KEYS:
        if batch.get(k) is None:
            raise ValueError(f"{what}: {k} is required")
    dims = {"F": F, "F1": F + 1, "K1": K1, "K2": K2, "D": F * max(int(prm["max_iterations"]), 0)}
    _need(batch, {k: dims[rows] * width for k, _, rows, width in _KEYS}, what)
    ib = InitializerBatch(F, K1, K2, *[conv(batch[k], dt) for k, dt, _, _ in _KEYS], int(prm["rand_max"]), float(prm["sigma"]),
                          int(prm["max_iterations"]), float(prm["min_parallax"]), int(prm["min_triangulated"]),
                          float(prm["rh_threshold"]))
    return ib, prm


def _shape(rows, width, F, K1, T):
    n = max({"F": F, "K1": K1}[rows], 1)
    return (n, 2, T) if width is None else (n, width) if width > 1 else (n,)


def InitializerInitialize(batch: dict, device: int = 0) -> dict:
    """bool Initializer::Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated)
    (src/Initializer.cc:45-122) of every pair, on host arrays.  Returns found (F) = the return value, model (F) =
    0 ReconstructH / 1 ReconstructF, r21t21 (F, 12) = R21 then t21 (0 without a success), p3d (total_kp1, 3) and
    triangulated (total_kp1) in reference-frame keypoint slots, score_h / score_f, best_h / best_f (the winning
    iteration, -1 for none), h21 / f21 (F, 9), inlier_h / inlier_f (total_kp1), hyp_score (F, 2, max_iterations),
    n_good and parallax (F, 8) of the motion hypotheses."""
    for k in ("kp1_begin", "kp2_begin"):
        if batch.get(k) is None:
            raise ValueError(f"InitializerInitialize: {k} is required")
    F = len(batch["kp1_begin"]) - 1
    K1, K2 = int(batch["kp1_begin"][-1]), int(batch["kp2_begin"][-1])
    keep = []

    def k(a, dt):
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return ptr(a)

    ib, prm = _struct(batch, k, F, K1, K2, "InitializerInitialize")
    T = max(int(prm["max_iterations"]), 1)
    out = {name: np.zeros(_shape(rows, width, F, K1, T), dt) for name, dt, rows, width in _OUT}
    res = InitializerResult(*[ptr(out[name]) for name, _, _, _ in _OUT])
    check(lib().orb_initializer_initialize(C.byref(ib), C.byref(res), int(device)), "orb_initializer_initialize")
    return {name: out[name][:K1 if rows == "K1" else F] for name, _, rows, _ in _OUT}


def initializer_initialize_device(batch: dict, out: dict | None = None, stream=None) -> dict:
    """Device form of InitializerInitialize: GPU tensors for the orb_initializer_batch arrays (matches12 as
    search_for_initialization_device returns it; draws int32), host values for the scalars; enqueues on `stream`
    (default: torch's current stream) and returns the output tensors, `out` may hold any of them.  found[p] = -1 for
    a pair either of whose frames has more than ORBM_PROJ_MAX_KP keypoints."""
    import torch
    for k in ("kp1_begin", "kp1_xy", "kp2_xy"):
        if batch.get(k) is None:
            raise ValueError(f"initializer_initialize_device: {k} is required")
    kb = batch["kp1_begin"]
    F = kb.numel() - 1
    K1, K2 = int(batch["kp1_xy"].shape[0]), int(batch["kp2_xy"].shape[0])
    for name, dt, _, _ in _KEYS:
        t = batch.get(name)
        if t is not None and (not hasattr(t, "is_cuda") or t.dtype != getattr(torch, np.dtype(dt).name) or not t.is_contiguous()
                              or not t.is_cuda):
            raise ValueError(f"initializer_initialize_device: {name} must be a contiguous {np.dtype(dt).name} GPU tensor")
    ib, prm = _struct(batch, lambda t, dt: tptr(t), F, K1, K2, "initializer_initialize_device")
    T = max(int(prm["max_iterations"]), 1)
    out = dict(out or {})
    want = {}
    for name, dt, rows, width in _OUT:
        shape = _shape(rows, width, F, K1, T)
        tdt = getattr(torch, np.dtype(dt).name)
        if out.get(name) is None:
            out[name] = torch.empty(shape, dtype=tdt, device=kb.device)
        want[name] = (int(np.prod(shape)) if {"F": F, "K1": K1}[rows] else 0, tdt)
    _need(out, {k: n for k, (n, _) in want.items()}, "initializer_initialize_device")
    for name, (_, dt) in want.items():
        t = out[name]
        if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"initializer_initialize_device: out[{name!r}] must be a contiguous {dt} GPU tensor")
    res = InitializerResult(*[tptr(out[name]) for name, _, _, _ in _OUT])
    check(lib().orb_initializer_initialize_device(C.byref(ib), C.byref(res), stream_ptr(stream)),
          "orb_initializer_initialize_device")
    return out
