"""LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:380-578) on extractor slots, batched over (keyframe 1,
keyframe 2) pairs (orblm_batch in include/orbslam2_amd.h).

    PreparePairs(batch, device=0)                         host arrays, synchronous
    TriangulateMatches(batch, pairs, match12, ...)        "
    CreateNewMapPoints(batch, search, n_rounds, ...)      "
    prepare_pairs_device / triangulate_matches_device / create_new_map_points_device
                                                          GPU tensors, enqueue only

`batch` holds the slot arrays of both keyframe sets: kps1 / kps2 ([F, cap] orbx_keypoint slots: KP_DTYPE arrays or
[F, cap, 7] 4-byte tensors, keypointsUn), counts1 / counts2 [F] int32, uright1 / depth1 / uright2 / depth2 [F, cap]
float32 or None (all monocular), has_mappoint2 [F2, cap2] uint8 and mp_xw2 [F2, cap2, 3] float32 (monocular batches: the
MapPoints of keyframe 2, for ComputeSceneMedianDepth), pose1 / pose2 [F, 12] (Tcw, 3 x 4 row-major), camera1 / camera2
[F, 6] (fx, fy, cx, cy, bf, baseline), frame1 / frame2 int32 per pair (negative: no pair; for the loop [n_rounds, P]),
and the host values scale_factors1 / sigma2_1 / scale_factors2 / sigma2_2 (the pyramids' tables; the keyframe 1
tables default to keyframe 2's), scale_factor (pyramid.scaleFactor) and monocular."""
import ctypes as C

import numpy as np

from ._lib import OrblmBatch, OrblmPairs, OrblmPoints, TriBatch, check, lib, ptr, stream_ptr, tptr

STATUS = dict(created=0, no_match=1, pair_skipped=2, low_parallax=3, w_zero=4, behind1=5, behind2=6, reproj1=7, reproj2=8,
              dist_zero=9, scale=10)
BRANCH = dict(none=0, triangulated=1, stereo1=2, stereo2=3)
MAX_LEVELS = 32   # ORBM_TRI_MAX_LEVELS

# orblm_pairs / orblm_points arrays in struct order: name -> (dtype, width per pair or per slot)
_PAIRS = (("F12", np.float32, 9), ("ep2", np.float32, 2), ("baseline", np.float32, 1), ("median", np.float32, 1),
          ("skip", np.int32, 1), ("frame1", np.int32, 1), ("frame2", np.int32, 1), ("consts", np.float32, 64))
_POINTS = (("status", np.int32, 1), ("branch", np.int32, 1), ("xw", np.float32, 3), ("normal", np.float32, 3),
           ("min_distance", np.float32, 1), ("max_distance", np.float32, 1), ("new_idx1", np.int32, 1),
           ("new_idx2", np.int32, 1))
# orblm_batch arrays: name -> (dtype, set, trailing width); None = optional
_SLOTS = (("uright1", np.float32, 1, 1), ("depth1", np.float32, 1, 1), ("uright2", np.float32, 2, 1), ("depth2", np.float32, 2, 1),
          ("has_mappoint2", np.uint8, 2, 1), ("mp_xw2", np.float32, 2, 3))
_FRAMES = (("pose1", 1, 12), ("pose2", 2, 12), ("camera1", 1, 6), ("camera2", 2, 6))


def _is_tensor(a):
    return hasattr(a, "data_ptr")


def _nbytes(a):
    return a.numel() * a.element_size() if _is_tensor(a) else a.nbytes


def _dims(batch, what):
    """(F1, cap1, F2, cap2) from the counts and keypoint slots, with the shape checks both forms share."""
    for k in ("kps1", "kps2", "counts1", "counts2", "pose1", "pose2", "camera1", "camera2"):
        if batch.get(k) is None:
            raise ValueError(f"{what}: {k} is required")
    out = []
    for s in ("1", "2"):
        k, c = batch["kps" + s], batch["counts" + s]
        F = int(c.shape[0])
        if len(c.shape) != 1 or len(k.shape) < 2 or int(k.shape[0]) != F or int(k.shape[1]) < 1 or \
                _nbytes(k) != F * int(k.shape[1]) * 28:
            raise ValueError(f"{what}: kps{s} must be [F, cap] orbx_keypoint slots (28 bytes) and counts{s} [F]")
        out += [F, int(k.shape[1])]
    return out


def _tables(batch, what):
    s2 = batch.get("scale_factors2")
    g2 = batch.get("sigma2_2")
    if s2 is None or g2 is None:
        raise ValueError(f"{what}: scale_factors2 and sigma2_2 are required")
    s1 = batch.get("scale_factors1") if batch.get("scale_factors1") is not None else s2
    g1 = batch.get("sigma2_1") if batch.get("sigma2_1") is not None else g2
    t = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in (s1, g1, s2, g2)]
    L = len(t[0])
    if any(len(a) != L for a in t) or L < 1:
        raise ValueError(f"{what}: the four pyramid tables must have one length")
    if L > MAX_LEVELS:
        raise ValueError(f"{what}: n_levels {L} exceeds ORBM_TRI_MAX_LEVELS ({MAX_LEVELS})")
    sf = batch.get("scale_factor")
    if sf is None:
        sf = float(t[0][min(1, L - 1)])
    return t, L, float(sf)


def _struct(batch, n_pairs, total, device_form, what, keep):
    """orblm_batch of `batch`; total = pairs in frame1 / frame2."""
    F1, cap1, F2, cap2 = _dims(batch, what)
    tables, L, sf = _tables(batch, what)
    keep.extend(tables)
    if device_form:
        import torch

    def conv(name, dt, shape, optional=False):
        a = batch.get(name)
        if a is None:
            if optional:
                return None
            raise ValueError(f"{what}: {name} is required")
        n = int(np.prod(shape))
        if device_form:
            if not _is_tensor(a) or not a.is_cuda or not a.is_contiguous() or a.dtype != getattr(torch, np.dtype(dt).name) \
                    or a.numel() != n:
                raise ValueError(f"{what}: {name} must be a contiguous {np.dtype(dt).name} GPU tensor of shape {tuple(shape)}")
            return tptr(a)
        a = np.ascontiguousarray(a, dt)
        if a.size != n:
            raise ValueError(f"{what}: {name} must have shape {tuple(shape)}")
        keep.append(a)
        return ptr(a)

    def kps(name):
        a = batch[name]
        if device_form:
            if not _is_tensor(a) or not a.is_cuda or not a.is_contiguous():
                raise ValueError(f"{what}: {name} must be a contiguous GPU tensor")
            return tptr(a)
        a = np.ascontiguousarray(a)
        keep.append(a)
        return ptr(a)

    dims = {1: (F1, cap1), 2: (F2, cap2)}
    slots = {name: conv(name, dt, dims[s] + ((w,) if w > 1 else ()), optional=True) for name, dt, s, w in _SLOTS}
    for s in ("1", "2"):
        if (slots["uright" + s] is None) != (slots["depth" + s] is None):
            raise ValueError(f"{what}: uright{s} and depth{s} go together")
    mono = bool(batch.get("monocular", False))
    if mono and (slots["has_mappoint2"] is None or slots["mp_xw2"] is None):
        raise ValueError(f"{what}: a monocular batch needs has_mappoint2 and mp_xw2")
    frames = {name: conv(name, np.float32, (dims[s][0], w)) for name, s, w in _FRAMES}
    f1 = conv("frame1", np.int32, (total,), optional=True)
    f2 = conv("frame2", np.int32, (total,), optional=True)
    b = OrblmBatch(n_pairs, cap1, cap2, F1, F2, kps("kps1"), conv("counts1", np.int32, (F1,)), slots["uright1"], slots["depth1"],
                   kps("kps2"), conv("counts2", np.int32, (F2,)), slots["uright2"], slots["depth2"], slots["has_mappoint2"],
                   slots["mp_xw2"], frames["pose1"], frames["pose2"], frames["camera1"], frames["camera2"], f1, f2, L,
                   ptr(tables[0]), ptr(tables[1]), ptr(tables[2]), ptr(tables[3]), sf, int(mono))
    return b, (F1, cap1, F2, cap2)


def _shape(n, w):
    return (n, w) if w > 1 else (n,)


def _host_out(spec, n):
    return {name: np.zeros(_shape(max(n, 1), w), dt) for name, dt, w in spec}


def _dev_out(spec, n, out, device, what):
    import torch
    res = {}
    for name, dt, w in spec:
        t = out.get(name) if out else None
        tdt = getattr(torch, np.dtype(dt).name)
        if t is None:
            t = torch.zeros(_shape(max(n, 1), w), dtype=tdt, device=device)
        elif not _is_tensor(t) or not t.is_cuda or not t.is_contiguous() or t.dtype != tdt or t.numel() < n * w:
            raise ValueError(f"{what}: out[{name!r}] must be a contiguous {tdt} GPU tensor of at least {n * w} elements")
        res[name] = t
    return res


def _pairs_in(pairs, n, device_form, what, keep):
    """orblm_pairs from what prepare returned."""
    vals = []
    for name, dt, w in _PAIRS:
        a = pairs.get(name) if pairs else None
        if a is None:
            raise ValueError(f"{what}: pairs[{name!r}] is required")
        if device_form:
            if not _is_tensor(a) or not a.is_cuda or not a.is_contiguous() or a.numel() < n * w:
                raise ValueError(f"{what}: pairs[{name!r}] must be a contiguous GPU tensor of {n * w} elements")
            vals.append(tptr(a))
        else:
            a = np.ascontiguousarray(a, dt)
            if a.size < n * w:
                raise ValueError(f"{what}: pairs[{name!r}] must hold {n * w} elements")
            keep.append(a)
            vals.append(ptr(a))
    return OrblmPairs(*vals)


def _n_pairs(batch, what):
    f = batch.get("frame1")
    if f is None:
        return int(batch["counts1"].shape[0]) if batch.get("counts1") is not None else 0
    if (batch.get("frame2") is None) or tuple(f.shape) != tuple(batch["frame2"].shape):
        raise ValueError(f"{what}: frame1 and frame2 must have one shape")
    return int(np.prod(f.shape))


def PreparePairs(batch: dict, device: int = 0) -> dict:
    """Per pair: F12 (ComputeF12, :55-71), ep2 (ORBmatcher.cc:772-773), baseline, median (ComputeSceneMedianDepth(2) of
    keyframe 2, monocular batches), skip (0 / 1 by :410-422 / 2 no pair), frame1 / frame2 and consts.  Host arrays."""
    keep = []
    P = _n_pairs(batch, "PreparePairs")
    b, _ = _struct(batch, P, P, False, "PreparePairs", keep)
    out = _host_out(_PAIRS, P)
    pr = OrblmPairs(*[ptr(out[name]) for name, _, _ in _PAIRS])
    check(lib().orblm_prepare_pairs(C.byref(b), C.byref(pr), int(device)), "orblm_prepare_pairs")
    return {k: v[:P] for k, v in out.items()}


def prepare_pairs_device(batch: dict, out: dict | None = None, stream=None) -> dict:
    """Device form of PreparePairs: GPU tensors, enqueue only.  F12 / ep2 are what
    search_for_triangulation_batch_device takes, frame1 / frame2 its (always valid) keyframe indices."""
    keep = []
    P = _n_pairs(batch, "prepare_pairs_device")
    b, _ = _struct(batch, P, P, True, "prepare_pairs_device", keep)
    res = _dev_out(_PAIRS, P, out, batch["counts1"].device, "prepare_pairs_device")
    pr = OrblmPairs(*[tptr(res[name]) for name, _, _ in _PAIRS])
    check(lib().orblm_prepare_pairs_device(C.byref(b), C.byref(pr), stream_ptr(stream)), "orblm_prepare_pairs_device")
    return res


def _flags(f, F, cap, device_form, what, name, keep):
    if f is None:
        return None
    if device_form:
        import torch
        if not _is_tensor(f) or not f.is_cuda or not f.is_contiguous() or f.dtype != torch.uint8 or f.numel() != F * cap:
            raise ValueError(f"{what}: {name} must be a contiguous uint8 GPU tensor [F, cap]")
        return tptr(f)
    if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or not f.flags.c_contiguous or f.size != F * cap or \
            not f.flags.writeable:
        raise ValueError(f"{what}: {name} must be a writable contiguous uint8 array [F, cap] (it is updated in place)")
    keep.append(f)
    return ptr(f)


def TriangulateMatches(batch: dict, pairs: dict, match12, has_mappoint1=None, has_mappoint2=None, device: int = 0) -> dict:
    """One triangulation step (:437-560) on host arrays: match12 [P, cap1] as the search leaves it, pairs = what
    PreparePairs returned.  Returns status, branch [P, cap1], xw, normal [P, cap1, 3], min_distance, max_distance,
    new_idx1, new_idx2 [P, cap1] (the created points, ascending idx1, then -1) and n_created [P].  has_mappoint1 /
    has_mappoint2 (uint8 [F, cap], optional) are updated in place."""
    what = "TriangulateMatches"
    keep = []
    P = _n_pairs(batch, what)
    b, (F1, cap1, F2, cap2) = _struct(batch, P, P, False, what, keep)
    pr = _pairs_in(pairs, P, False, what, keep)
    m = np.ascontiguousarray(match12, np.int32)
    if m.size != P * cap1:
        raise ValueError(f"{what}: match12 must be [P, cap1]")
    out = _host_out(_POINTS, P * cap1)
    out["n_created"] = np.zeros(max(P, 1), np.int32)
    pts = OrblmPoints(*[ptr(out[name]) for name, _, _ in _POINTS], ptr(out["n_created"]),
                      _flags(has_mappoint1, F1, cap1, False, what, "has_mappoint1", keep),
                      _flags(has_mappoint2, F2, cap2, False, what, "has_mappoint2", keep))
    check(lib().orblm_triangulate(C.byref(b), C.byref(pr), ptr(m), C.byref(pts), int(device)), "orblm_triangulate")
    return _reshape(out, P, cap1)


def _reshape(out, P, cap1):
    res = {}
    for name, _, w in _POINTS:
        a = out[name][:P * cap1]
        res[name] = a.reshape((P, cap1, w) if w > 1 else (P, cap1))
    res["n_created"] = out["n_created"][:P]
    return res


def _points_dev(P, cap1, out, device, what, flags1, flags2, dims):
    res = _dev_out(_POINTS, P * cap1, out, device, what)
    res.update(_dev_out((("n_created", np.int32, 1),), P, out, device, what))
    F1, c1, F2, c2 = dims
    pts = OrblmPoints(*[tptr(res[name]) for name, _, _ in _POINTS], tptr(res["n_created"]),
                      _flags(flags1, F1, c1, True, what, "has_mappoint1", []), _flags(flags2, F2, c2, True, what, "has_mappoint2", []))
    for name, _, w in _POINTS:
        if res[name].numel() == P * cap1 * w and P:
            res[name] = res[name].view((P, cap1, w) if w > 1 else (P, cap1))
    return res, pts


def triangulate_matches_device(batch: dict, pairs: dict, match12, has_mappoint1=None, has_mappoint2=None,
                               out: dict | None = None, stream=None) -> dict:
    """Device form of TriangulateMatches: GPU tensors, enqueue only.  The flags, when given, are written in place."""
    import torch
    what = "triangulate_matches_device"
    P = _n_pairs(batch, what)
    b, dims = _struct(batch, P, P, True, what, [])
    cap1 = dims[1]
    pr = _pairs_in(pairs, P, True, what, [])
    if not _is_tensor(match12) or not match12.is_cuda or match12.dtype != torch.int32 or not match12.is_contiguous() or \
            match12.numel() != P * cap1:
        raise ValueError(f"{what}: match12 must be a contiguous int32 GPU tensor [P, cap1]")
    res, pts = _points_dev(P, cap1, out, match12.device, what, has_mappoint1, has_mappoint2, dims)
    check(lib().orblm_triangulate_device(C.byref(b), C.byref(pr), tptr(match12), C.byref(pts), stream_ptr(stream)),
          "orblm_triangulate_device")
    return res


def check_plan(frame1, frame2, same_set: bool):
    """The neighbour loop's precondition on a host plan ([n_rounds, P] each, negative = no pair): within one round all
    keyframes 1 are distinct, all keyframes 2 are distinct and, where both sets are the same slots, none is both."""
    f1, f2 = np.asarray(frame1), np.asarray(frame2)
    if f1.ndim != 2 or f1.shape != f2.shape:
        raise ValueError("the plan must be two [n_rounds, P] arrays")
    for r in range(f1.shape[0]):
        on = f1[r] >= 0
        if np.any((f2[r] >= 0) != on):
            raise ValueError(f"round {r}: an entry with one keyframe only")
        a, c = f1[r][on], f2[r][on]
        if len(np.unique(a)) != len(a) or len(np.unique(c)) != len(c):
            raise ValueError(f"round {r} names a keyframe twice")
        if same_set and len(np.intersect1d(a, c)):
            raise ValueError(f"round {r} names a keyframe as keyframe 1 and as keyframe 2")


def _search_struct(search, device_form, what, keep, F1, cap1, F2, cap2):
    if not search or search.get("desc1") is None or search.get("desc2") is None:
        raise ValueError(f"{what}: search needs desc1 and desc2")
    vals = {}
    for name, F, cap in (("desc1", F1, cap1), ("desc2", F2, cap2)):
        d = search[name]
        if device_form:
            import torch
            if not _is_tensor(d) or not d.is_cuda or d.dtype != torch.uint8 or not d.is_contiguous() or d.numel() != F * cap * 32:
                raise ValueError(f"{what}: search[{name!r}] must be a contiguous uint8 GPU tensor [F, cap, 32]")
            vals[name] = tptr(d)
        else:
            d = np.ascontiguousarray(d, np.uint8)
            if d.size != F * cap * 32:
                raise ValueError(f"{what}: search[{name!r}] must be [F, cap, 32]")
            keep.append(d)
            vals[name] = ptr(d)
    fv = [None] * 8
    fvc = [0, 0]
    if search.get("fv1") is not None or search.get("fv2") is not None:
        if not device_form:
            raise ValueError(f"{what}: the host form searches without FeatureVectors")
        from .matcher import _check_fv
        _check_fv(search.get("fv1"), F1, "fv1")
        _check_fv(search.get("fv2"), F2, "fv2")
        fv = [tptr(t) for t in search["fv1"]] + [tptr(t) for t in search["fv2"]]
        fvc = [int(search["fv1"][0].shape[1]), int(search["fv2"][0].shape[1])]
    return TriBatch(0, cap1, cap2, None, vals["desc1"], None, None, None, None, vals["desc2"], None, None, None, None, None,
                    None, None, *fv, fvc[0], fvc[1], 0, None, None, int(bool(search.get("only_stereo", False))))


def _plan(batch, what):
    f1, f2 = batch.get("frame1"), batch.get("frame2")
    if f1 is None or f2 is None or len(f1.shape) != 2 or tuple(f1.shape) != tuple(f2.shape):
        raise ValueError(f"{what}: the plan frame1 / frame2 must be two [n_rounds, P] arrays")
    return int(f1.shape[0]), int(f1.shape[1])


def CreateNewMapPoints(batch: dict, search: dict, has_mappoint1, has_mappoint2, device: int = 0) -> dict:
    """The neighbour loop of CreateNewMapPoints on host arrays: batch["frame1"] / ["frame2"] are the plan [n_rounds, P]
    (negative: no pair); search = dict(desc1, desc2, only_stereo=False).  Round by round the search
    (SearchForTriangulation) and the triangulation run with has_mappoint1 / has_mappoint2 (uint8 [F, cap], updated in
    place; one array for both where the two sets are the same slots).  Returns what PreparePairs and
    TriangulateMatches return with a leading [n_rounds, P], plus match12 and nmatches."""
    what = "CreateNewMapPoints"
    keep = []
    R, P = _plan(batch, what)
    same = has_mappoint1 is has_mappoint2
    check_plan(batch["frame1"], batch["frame2"], same)
    b, (F1, cap1, F2, cap2) = _struct(batch, P, R * P, False, what, keep)
    s = _search_struct(search, False, what, keep, F1, cap1, F2, cap2)
    if has_mappoint1 is None or has_mappoint2 is None:
        raise ValueError(f"{what}: has_mappoint1 and has_mappoint2 are required")
    n = R * P
    pout = _host_out(_PAIRS, n)
    out = _host_out(_POINTS, n * cap1)
    out["n_created"] = np.zeros(max(n, 1), np.int32)
    m12 = np.full(max(n * cap1, 1), -1, np.int32)
    nm = np.zeros(max(n, 1), np.int32)
    pr = OrblmPairs(*[ptr(pout[name]) for name, _, _ in _PAIRS])
    pts = OrblmPoints(*[ptr(out[name]) for name, _, _ in _POINTS], ptr(out["n_created"]),
                      _flags(has_mappoint1, F1, cap1, False, what, "has_mappoint1", keep),
                      _flags(has_mappoint2, F2, cap2, False, what, "has_mappoint2", keep))
    check(lib().orblm_create_new_map_points(C.byref(b), C.byref(s), R, C.byref(pr), C.byref(pts), ptr(m12), ptr(nm), int(device)),
          "orblm_create_new_map_points")
    res = {k: v[:n].reshape((R, P) + v.shape[1:]) for k, v in pout.items()}
    pts_res = _reshape(out, n, cap1)
    res.update({k: v.reshape((R, P) + v.shape[1:]) for k, v in pts_res.items()})
    res["match12"] = m12[:n * cap1].reshape(R, P, cap1)
    res["nmatches"] = nm[:n].reshape(R, P)
    return res


def create_new_map_points_device(batch: dict, search: dict, has_mappoint1, has_mappoint2, out: dict | None = None,
                                 stream=None, plan=None) -> dict:
    """Device form of CreateNewMapPoints: GPU tensors, enqueue only (no synchronisation, no copy back).  search may
    also hold fv1 / fv2 (ORBVocabulary.transform_batch_device).  The plan is device memory, so its precondition
    (check_plan) is the caller's: pass the host copy as plan=(frame1, frame2) to have it checked here.  Outputs as
    CreateNewMapPoints, flat over the n_rounds * P pairs."""
    import torch
    what = "create_new_map_points_device"
    R, P = _plan(batch, what)
    if has_mappoint1 is None or has_mappoint2 is None:
        raise ValueError(f"{what}: has_mappoint1 and has_mappoint2 are required")
    if plan is not None:
        check_plan(plan[0], plan[1], has_mappoint1 is has_mappoint2 or has_mappoint1.data_ptr() == has_mappoint2.data_ptr())
    b, dims = _struct(batch, P, R * P, True, what, [])
    F1, cap1, F2, cap2 = dims
    s = _search_struct(search, True, what, [], F1, cap1, F2, cap2)
    n = R * P
    dev = batch["counts1"].device
    res = _dev_out(_PAIRS, n, out, dev, what)
    pr = OrblmPairs(*[tptr(res[name]) for name, _, _ in _PAIRS])
    pres, pts = _points_dev(n, cap1, out, dev, what, has_mappoint1, has_mappoint2, dims)
    res.update(pres)
    res.update(_dev_out((("match12", np.int32, cap1), ("nmatches", np.int32, 1)), n, out, dev, what))
    check(lib().orblm_create_new_map_points_device(C.byref(b), C.byref(s), R, C.byref(pr), C.byref(pts), tptr(res["match12"]),
                                                   tptr(res["nmatches"]), stream_ptr(stream)),
          "orblm_create_new_map_points_device")
    return res
