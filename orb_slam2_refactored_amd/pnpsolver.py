"""PnPsolver (include/PnPsolver.h, src/PnPsolver.cc): the EPnP RANSAC of Tracking::Relocalization, batched over
candidate keyframes (orb_pnpsolver_batch in include/orbslam2_amd.h).

    PnPsolverIterate(batch, device=0)                          host arrays, synchronous
    pnpsolver_iterate_device(batch, out=None, stream=None)     GPU tensors, enqueue only
    make_draws(n_frames, n_draws, seed)                        the rand() table both read

`batch` holds kp_begin (F + 1), kp_xy (K, 2), kp_octave (K), camera (F, 4), mp_valid (K), mp_xw (K, 3), level_sigma2
(pyramid.sigmaSq), draws (F, D, 4) and the scalars probability (0.99), min_inliers (10), max_iterations (300),
min_set (4), epsilon (0.5), th2 (5.991), maxk (5) and rand_max (2147483647).  The solver's state (iterations,
best_inliers, best_mask, best_tcw) is read from the batch (absent: a fresh solver) and returned, so a result's four
arrays can be passed back in to resume a candidate."""
import ctypes as C

import numpy as np

from ._lib import PnPSolverBatch, PnPSolverResult, check, lib, ptr, stream_ptr, tptr
from .optimizer import _need

RAND_MAX = 2147483647   # glibc
DEFAULTS = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991, maxk=5, rand_max=RAND_MAX)

# orb_pnpsolver_batch arrays in struct order: name -> (dtype, rows, row width)
_KEYS = (("kp_begin", np.int32, "F1", 1), ("kp_xy", np.float32, "K", 2), ("kp_octave", np.int32, "K", 1),
         ("camera", np.float32, "F", 4), ("mp_valid", np.uint8, "K", 1), ("mp_xw", np.float32, "K", 3))
_OUT = ("tcw", "inlier", "found", "n_inliers", "terminate", "iterations", "best_inliers", "best_mask", "best_tcw", "hyp_inliers")
_STATE = (("iterations", np.int32, "F", 1), ("best_inliers", np.int32, "F", 1), ("best_mask", np.uint8, "K", 1),
          ("best_tcw", np.float32, "F", 12))


def make_draws(n_frames: int, n_draws: int, seed: int = 0, rand_max: int = RAND_MAX) -> np.ndarray:
    """(n_frames, n_draws, 4) int32 values uniform in [0, rand_max]: what rand() would have returned for the four
    draws of every hypothesis of every candidate."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, int(rand_max) + 1, (n_frames, n_draws, 4), dtype=np.int64).astype(np.int32)


def _params(batch):
    return {k: batch[k] if batch.get(k) is not None else v for k, v in DEFAULTS.items()}


def _n_draws(batch, F):
    d = batch["draws"]
    n = d.size if isinstance(d, np.ndarray) else int(d.numel()) if hasattr(d, "numel") else int(np.size(d))
    if len(d.shape) == 3:
        if d.shape[0] != F or d.shape[2] != 4:
            raise ValueError(f"draws has shape {tuple(d.shape)}, needs ({F}, n_draws, 4)")
        return int(d.shape[1])
    if F == 0 or n % (4 * F):
        raise ValueError(f"draws has {n} elements, needs a multiple of 4 x {F}")
    return n // (4 * F)


def _struct(batch, conv, F, K, what):
    prm = _params(batch)
    for k, _, _, _ in _KEYS + (("draws", None, None, 0), ("level_sigma2", None, None, 0)):
        if batch.get(k) is None:
            raise ValueError(f"{what}: {k} is required")
    dims = {"F": F, "F1": F + 1, "K": K}
    _need(batch, {k: dims[rows] * width for k, _, rows, width in _KEYS}, what)
    D = _n_draws(batch, F) if F else 1
    sig = np.ascontiguousarray(batch["level_sigma2"], np.float32)
    ptrs = [conv(batch[k], dt) for k, dt, _, _ in _KEYS]
    sb = PnPSolverBatch(F, K, *ptrs, len(sig), ptr(sig), conv(batch["draws"], np.int32), D, int(prm["rand_max"]),
                        float(prm["probability"]), int(prm["min_inliers"]), int(prm["max_iterations"]), int(prm["min_set"]),
                        float(prm["epsilon"]), float(prm["th2"]), int(prm["maxk"]))
    return sb, sig, D


def PnPsolverIterate(batch: dict, device: int = 0) -> dict:
    """cv::Mat PnPsolver::iterate(nIterations, bNoMore, vbInliers, nInliers) (src/PnPsolver.cc:165-258) of a solver
    per candidate, on host arrays.  Returns tcw (F, 12) = Rcw, tcw (0 when nothing is returned), inlier (K) =
    vbInliers, found (F) = 1 refined / 2 best at termination / 0, n_inliers (F), terminate (F) = bNoMore, the state
    after the call (iterations, best_inliers, best_mask, best_tcw) and hyp_inliers (F, n_draws) = the inlier count
    of every hypothesis evaluated, -1 elsewhere."""
    if batch.get("kp_begin") is None:
        raise ValueError("PnPsolverIterate: kp_begin is required")
    F = len(batch["kp_begin"]) - 1
    K = int(batch["kp_begin"][-1])
    keep = []

    def k(a, dt):
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return ptr(a)

    sb, _sig, D = _struct(batch, k, F, K, "PnPsolverIterate")
    dims = {"F": max(F, 1), "K": max(K, 1)}
    state = {}
    for name, dt, rows, width in _STATE:
        v = batch.get(name)
        state[name] = np.zeros(dims[rows] * width, dt) if v is None else np.array(v, dt).reshape(-1)
    _need(state, {"iterations": F, "best_inliers": F, "best_mask": K, "best_tcw": 12 * F}, "PnPsolverIterate")
    out = dict(tcw=np.zeros((max(F, 1), 12), np.float32), inlier=np.zeros(max(K, 1), np.uint8), found=np.zeros(max(F, 1), np.int32),
               n_inliers=np.zeros(max(F, 1), np.int32), terminate=np.zeros(max(F, 1), np.int32),
               hyp_inliers=np.zeros((max(F, 1), D), np.int32), **state)
    res = PnPSolverResult(*[ptr(out[n]) for n in _OUT])
    check(lib().orb_pnpsolver_iterate(C.byref(sb), C.byref(res), int(device)), "orb_pnpsolver_iterate")
    for n in ("inlier", "best_mask"):
        out[n] = out[n][:K]
    for n in ("tcw", "found", "n_inliers", "terminate", "iterations", "best_inliers", "hyp_inliers"):
        out[n] = out[n][:F]
    out["best_tcw"] = out["best_tcw"][:12 * F].reshape(F, 12)
    return out


def pnpsolver_iterate_device(batch: dict, out: dict | None = None, stream=None) -> dict:
    """Device form of PnPsolverIterate: GPU tensors for the orb_pnpsolver_batch arrays (kp_begin, kp_octave and draws
    int32, kp_xy, camera and mp_xw float32, mp_valid uint8), host values for level_sigma2 and the scalars; enqueues
    on `stream` (default: torch's current stream) and returns the output tensors.  `out` may hold any of them;
    out["iterations"], out["best_inliers"], out["best_mask"] and out["best_tcw"] are the state and are updated in
    place (pass the dict of the previous call to resume).  Without them the state starts from the batch's arrays of
    the same names (copied), or from 0.  found[p] = -1 for a candidate with more than ORBM_PROJ_MAX_KP keypoints
    or whose range would pass the draw table."""
    import torch
    what = "pnpsolver_iterate_device"
    for k in ("kp_begin", "mp_xw"):
        if batch.get(k) is None:
            raise ValueError(f"{what}: {k} is required")
    kb = batch["kp_begin"]
    if not hasattr(kb, "is_cuda"):
        raise ValueError(f"{what}: kp_begin must be a contiguous int32 GPU tensor")
    F = kb.numel() - 1
    K = int(batch["mp_xw"].numel()) // 3
    for name, dt, _, _ in _KEYS + (("draws", np.int32, None, 0),):
        t = batch.get(name)
        if t is not None and (not hasattr(t, "is_cuda") or t.dtype != getattr(torch, np.dtype(dt).name) or not t.is_contiguous()
                              or not t.is_cuda):
            raise ValueError(f"{what}: {name} must be a contiguous {np.dtype(dt).name} GPU tensor")
    sb, _sig, D = _struct(batch, lambda t, dt: tptr(t), F, K, what)
    out = dict(out or {})
    dims = {"F": max(F, 1), "K": max(K, 1)}
    for name, dt, rows, width in _STATE:
        if out.get(name) is None:
            v = batch.get(name)
            tdt = getattr(torch, np.dtype(dt).name)
            out[name] = (torch.zeros(dims[rows] * width, dtype=tdt, device=kb.device) if v is None
                         else torch.as_tensor(v, dtype=tdt, device=kb.device).reshape(-1).clone())
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=kb.device)   # noqa: E731
    out.setdefault("tcw", new((max(F, 1), 12), torch.float32))
    out.setdefault("inlier", new(max(K, 1), torch.uint8))
    for name in ("found", "n_inliers", "terminate"):
        out.setdefault(name, new(max(F, 1), torch.int32))
    out.setdefault("hyp_inliers", new((max(F, 1), D), torch.int32))
    want = {"tcw": (12 * F, torch.float32), "inlier": (K, torch.uint8), "found": (F, torch.int32), "n_inliers": (F, torch.int32),
            "terminate": (F, torch.int32), "iterations": (F, torch.int32), "best_inliers": (F, torch.int32),
            "best_mask": (K, torch.uint8), "best_tcw": (12 * F, torch.float32), "hyp_inliers": (F * D, torch.int32)}
    _need(out, {k: n for k, (n, _) in want.items()}, what)
    for name, (_, dt) in want.items():
        t = out[name]
        if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"{what}: out[{name!r}] must be a contiguous {dt} GPU tensor")
    res = PnPSolverResult(*[tptr(out[n]) for n in _OUT])
    check(lib().orb_pnpsolver_iterate_device(C.byref(sb), C.byref(res), stream_ptr(stream)), "orb_pnpsolver_iterate_device")
    return out
