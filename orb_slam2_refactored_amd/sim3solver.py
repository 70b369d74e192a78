"""Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc): the 3-point RANSAC of LoopClosing::FindLoopInCandidateKFs,
batched over loop candidates (orb_sim3solver_batch in include/orbslam2_amd.h).

    Sim3SolverIterate(batch, device=0)                         host arrays, synchronous
    sim3solver_iterate_device(batch, out=None, stream=None)    GPU tensors, enqueue only
    make_draws(n_pairs, max_iterations, seed)                  the rand() table both read

`batch` is SearchBySim3's / OptimizeSim3's slot layout (kp1_begin, kp2_begin, kp1_octave, kp2_octave, pose1,
camera1, pose2, camera2, mp1_valid, mp1_xw, mp2_valid, mp2_xw, match12) plus level_sigma2 (pyramid.sigmaSq),
draws and the scalars fix_scale, probability (0.99), min_inliers (20), max_iterations (300), maxk (5) and
rand_max (2147483647).  The solver's state, iterations and max_inliers per pair, is read from the batch (absent:
a fresh solver) and returned, so a result's two arrays can be passed back in to resume a candidate."""
import ctypes as C

import numpy as np

from ._lib import Sim3SolverBatch, Sim3SolverResult, check, lib, ptr, stream_ptr, tptr
from .optimizer import _need

RAND_MAX = 2147483647   # glibc
DEFAULTS = dict(probability=0.99, min_inliers=20, max_iterations=300, maxk=5, rand_max=RAND_MAX, fix_scale=0)

# orb_sim3solver_batch arrays in struct order: name -> (dtype, rows, row width); None: not read, passed as NULL
_KEYS = (("kp1_begin", np.int32, "F1", 1), ("kp2_begin", np.int32, "F1", 1),
         ("kp1_xy", None, None, 0), ("kp1_octave", np.int32, "K1", 1),
         ("kp2_xy", None, None, 0), ("kp2_octave", np.int32, "K2", 1),
         ("pose1", np.float32, "F", 12), ("camera1", np.float32, "F", 4),
         ("pose2", np.float32, "F", 12), ("camera2", np.float32, "F", 4),
         ("mp1_valid", np.uint8, "K1", 1), ("mp1_xw", np.float32, "K1", 3),
         ("mp2_valid", np.uint8, "K2", 1), ("mp2_xw", np.float32, "K2", 3),
         ("s12", None, None, 0), ("match12", np.int32, "K1", 1))
_OUT = ("s12", "inlier", "match12", "found", "n_inliers", "iterations", "max_inliers", "terminate", "hyp_inliers")


def make_draws(n_pairs: int, max_iterations: int, seed: int = 0, rand_max: int = RAND_MAX) -> np.ndarray:
    """(n_pairs, max_iterations, 3) int32 values uniform in [0, rand_max]: what rand() would have returned for the
    three draws of every hypothesis of every pair."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, int(rand_max) + 1, (n_pairs, max_iterations, 3), dtype=np.int64).astype(np.int32)


def _params(batch):
    return {k: batch[k] if batch.get(k) is not None else v for k, v in DEFAULTS.items()}


def _struct(batch, conv, F, K1, K2, what):
    prm = _params(batch)
    for k, dt, _, _ in _KEYS + (("draws", np.int32, None, 0),):
        if dt is not None and batch.get(k) is None:
            raise ValueError(f"{what}: {k} is required")
    if batch.get("level_sigma2") is None:
        raise ValueError(f"{what}: level_sigma2 is required")
    dims = {"F": F, "F1": F + 1, "K1": K1, "K2": K2}
    need = {k: dims[rows] * width for k, dt, rows, width in _KEYS if dt is not None}
    need["draws"] = 3 * F * max(int(prm["max_iterations"]), 0)
    _need(batch, need, what)
    sig = np.ascontiguousarray(batch["level_sigma2"], np.float32)
    ptrs = [conv(batch[k], dt) if dt is not None else None for k, dt, _, _ in _KEYS]
    sb = Sim3SolverBatch(F, K1, K2, *ptrs, len(sig), ptr(sig), int(bool(prm["fix_scale"])), conv(batch["draws"], np.int32),
                         int(prm["rand_max"]), float(prm["probability"]), int(prm["min_inliers"]),
                         int(prm["max_iterations"]), int(prm["maxk"]))
    return sb, sig, prm


def Sim3SolverIterate(batch: dict, device: int = 0) -> dict:
    """bool Sim3Solver::iterate(maxk, sim3, isInlier) (src/Sim3Solver.cc:289-365) of a solver per pair, on host
    arrays.  Returns s12 (F, 13) = R12, t12, s of the successful hypothesis (0 without one), inlier (total_kp1) =
    isInlier, match12 (total_kp1) = the input's match where inlier else -1, found (F) = the return value, n_inliers
    (F), iterations and max_inliers (F) = the state after the call, terminate (F) and hyp_inliers
    (F, max_iterations) = the inlier count of every hypothesis evaluated, -1 elsewhere."""
    for k in ("kp1_begin", "kp2_begin"):
        if batch.get(k) is None:
            raise ValueError(f"Sim3SolverIterate: {k} is required")
    F = len(batch["kp1_begin"]) - 1
    K1, K2 = int(batch["kp1_begin"][-1]), int(batch["kp2_begin"][-1])
    keep = []

    def k(a, dt):
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return ptr(a)

    sb, _sig, prm = _struct(batch, k, F, K1, K2, "Sim3SolverIterate")
    state = {}
    for name in ("iterations", "max_inliers"):
        v = batch.get(name)
        state[name] = np.zeros(max(F, 1), np.int32) if v is None else np.array(v, np.int32).reshape(-1)
    _need(state, {"iterations": F, "max_inliers": F}, "Sim3SolverIterate")
    T = max(int(prm["max_iterations"]), 1)
    out = dict(s12=np.zeros((F, 13), np.float32), inlier=np.zeros(max(K1, 1), np.uint8), match12=np.zeros(max(K1, 1), np.int32),
               found=np.zeros(max(F, 1), np.int32), n_inliers=np.zeros(max(F, 1), np.int32), iterations=state["iterations"],
               max_inliers=state["max_inliers"], terminate=np.zeros(max(F, 1), np.int32),
               hyp_inliers=np.zeros((max(F, 1), T), np.int32))
    res = Sim3SolverResult(*[ptr(out[n]) for n in _OUT])
    check(lib().orb_sim3solver_iterate(C.byref(sb), C.byref(res), int(device)), "orb_sim3solver_iterate")
    for n in ("inlier", "match12"):
        out[n] = out[n][:K1]
    for n in ("found", "n_inliers", "iterations", "max_inliers", "terminate", "hyp_inliers"):
        out[n] = out[n][:F]
    return out


def sim3solver_iterate_device(batch: dict, out: dict | None = None, stream=None) -> dict:
    """Device form of Sim3SolverIterate: GPU tensors for the orb_sim3solver_batch arrays (search_by_sim3_device's
    dtypes; draws int32), host values for level_sigma2 and the scalars; enqueues on `stream` (default: torch's
    current stream) and returns the output tensors.  `out` may hold any of them; out["iterations"] and
    out["max_inliers"] are the state and are updated in place (pass the dict of the previous call to resume).
    Without them the state starts from batch["iterations"] / batch["max_inliers"] (copied), or from 0.
    found[p] = -1 for a pair either of whose keyframes has more than ORBM_PROJ_MAX_KP keypoints."""
    import torch
    for k in ("kp1_begin", "mp1_xw", "mp2_xw"):
        if batch.get(k) is None:
            raise ValueError(f"sim3solver_iterate_device: {k} is required")
    kb = batch["kp1_begin"]
    F = kb.numel() - 1
    K1, K2 = int(batch["mp1_xw"].shape[0]), int(batch["mp2_xw"].shape[0])
    for name, dt, _, _ in _KEYS + (("draws", np.int32, None, 0),):
        t = batch.get(name)
        if dt is not None and t is not None and (
                not hasattr(t, "is_cuda") or t.dtype != getattr(torch, np.dtype(dt).name) or not t.is_contiguous() or not t.is_cuda):
            raise ValueError(f"sim3solver_iterate_device: {name} must be a contiguous {np.dtype(dt).name} GPU tensor")
    sb, _sig, prm = _struct(batch, lambda t, dt: tptr(t), F, K1, K2, "sim3solver_iterate_device")
    T = max(int(prm["max_iterations"]), 1)
    out = dict(out or {})
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=kb.device)   # noqa: E731
    for name in ("iterations", "max_inliers"):
        if out.get(name) is None:
            v = batch.get(name)
            out[name] = (torch.zeros(max(F, 1), dtype=torch.int32, device=kb.device) if v is None
                         else torch.as_tensor(v, dtype=torch.int32, device=kb.device).reshape(-1).clone())
    out.setdefault("s12", new((F, 13), torch.float32))
    out.setdefault("inlier", new(max(K1, 1), torch.uint8))
    out.setdefault("match12", new(max(K1, 1), torch.int32))
    for name in ("found", "n_inliers", "terminate"):
        out.setdefault(name, new(max(F, 1), torch.int32))
    out.setdefault("hyp_inliers", new((max(F, 1), T), torch.int32))
    want = {"s12": (13 * F, torch.float32), "inlier": (K1, torch.uint8), "match12": (K1, torch.int32),
            "found": (F, torch.int32), "n_inliers": (F, torch.int32), "iterations": (F, torch.int32),
            "max_inliers": (F, torch.int32), "terminate": (F, torch.int32), "hyp_inliers": (F * T, torch.int32)}
    _need(out, {k: n for k, (n, _) in want.items()}, "sim3solver_iterate_device")
    for name, (_, dt) in want.items():
        t = out[name]
        if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"sim3solver_iterate_device: out[{name!r}] must be a contiguous {dt} GPU tensor")
    res = Sim3SolverResult(*[tptr(out[n]) for n in _OUT])
    check(lib().orb_sim3solver_iterate_device(C.byref(sb), C.byref(res), stream_ptr(stream)), "orb_sim3solver_iterate_device")
    return out
