"""A numpy restatement of Initializer::Initialize (src/Initializer.cc:45-122) for the checks of csrc/orbinit.hip.

Every SVD goes through numpy.linalg.svd in fp64 (svd() below, which can negate one singular-vector pair for the
sign test) and every inverse through numpy.linalg.inv; the matrices are rounded to float32 where the reference
holds a CV_32F result that float code then reads: H21i, H12i, F21i, the R and t of every motion hypothesis, d1..d3
and x3D.  CheckHomography, CheckFundamental and CheckRT are float32 element by element, the scores accumulated by
np.float32 in ascending order (a sequential cumsum over the 2 N terms, 0 where the reference adds nothing).
Normalize uses the device's documented summation order (csrc/orbinit.hip).  Matrix products whose order OpenCV does
not show are fixed as in csrc/init_hyp.h.

initialize(batch, jitter=seed) moves every entry of every H21i / H12i / F21i by one float ulp up or down before it
is scored: the restatement's own spread under that jitter is what the device is allowed (test_initializer_ref.py)."""
import numpy as np

f32 = np.float32
f64 = np.float64
ONE = f32(1)
MAXKP = 8192
FLIP = {}   # tag -> index of the singular-vector pair svd() negates (test_initializer_ref.py)


def svd(A, tag):
    U, w, Vt = np.linalg.svd(np.asarray(A, f64))
    k = FLIP.get(tag)
    if k is not None:
        U = U.copy()
        Vt = Vt.copy()
        if k < U.shape[-1]:
            U[..., :, k] *= -1
        Vt[..., k, :] *= -1
    return U, w, Vt


def random_int(r, rand_max, d):
    v = int((float(r) / (float(rand_max) + 1.0)) * d)
    return min(max(v, 0), d - 1)


def pick8(draw, rand_max, n):
    """Initializer.cc:83-98, with the vector."""
    avail = list(range(n))
    out = []
    for j in range(8):
        r = random_int(draw[j], rand_max, len(avail))
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def wave_sum(x):
    part = np.zeros(64, f32)
    for l in range(64):
        s = x[l::64]
        if len(s):
            part[l] = np.cumsum(s, dtype=f32)[-1]
    for d in (32, 16, 8, 4, 2, 1):
        part = part + part[np.arange(64) ^ d]
    return part[0]


def normalize(xy):
    """Normalize (:750-796): mean (2), scale (2) and T (3 x 3), float32."""
    xy = np.asarray(xy, f32).reshape(-1, 2)
    n = f32(len(xy))
    with np.errstate(all="ignore"):
        mean = np.array([wave_sum(xy[:, 0]) / n, wave_sum(xy[:, 1]) / n], f32)
        dev = np.array([wave_sum(np.abs(xy[:, 0] - mean[0])) / n, wave_sum(np.abs(xy[:, 1] - mean[1])) / n], f32)
        s = ONE / dev
    T = np.array([[s[0], 0, -mean[0] * s[0]], [0, s[1], -mean[1] * s[1]], [0, 0, 1]], f32)
    return mean, s, T


def rows_h(pn1, pn2):
    """ComputeH21's A (..., 16, 9) in float32 from (..., 8, 2) points."""
    u1, v1, u2, v2 = pn1[..., 0], pn1[..., 1], pn2[..., 0], pn2[..., 1]
    z, o = np.zeros_like(u1), np.ones_like(u1)
    r0 = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], -1)
    r1 = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], -1)
    return np.stack([r0, r1], -2).reshape(u1.shape[:-1] + (16, 9)).astype(f32)


def rows_f(pn1, pn2):
    u1, v1, u2, v2 = pn1[..., 0], pn1[..., 1], pn2[..., 0], pn2[..., 1]
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1).astype(f32)


def hypothesis_h(pn1, pn2, T1, T2):
    """Hn (fp64, unit), H21i (fp64, before the narrowing) of (..., 8, 2) normalised points."""
    Hn = svd(rows_h(pn1, pn2), "h")[2][..., 8, :].reshape(pn1.shape[:-2] + (3, 3))
    return Hn, (np.linalg.inv(T2.astype(f64)) @ Hn) @ T1.astype(f64)


def hypothesis_f(pn1, pn2, T1, T2):
    Fpre = svd(rows_f(pn1, pn2), "f")[2][..., 8, :].reshape(pn1.shape[:-2] + (3, 3))
    U, w, Vt = svd(Fpre, "f3")
    w = w.copy()
    w[..., 2] = 0
    Fn = (U * w[..., None, :]) @ Vt
    return Fpre, Fn, (T2.astype(f64).T @ Fn) @ T1.astype(f64)


def inverse_f32(M):
    with np.errstate(all="ignore"):
        try:
            return np.linalg.inv(M.astype(f64))
        except np.linalg.LinAlgError:
            return np.full(M.shape, np.nan)


def _accumulate(t1, t2):
    terms = np.stack([t1, t2], -1).reshape(t1.shape[:-1] + (-1,))
    return np.cumsum(terms, axis=-1, dtype=f32)[..., -1]


def check_homography(H21, H12, pts, sigma):
    """(T, 3, 3) float32 matrices against (N, 4) float32 points: scores (T) and vbMatchesInliers (T, N)."""
    th = f32(5.991)
    inv = ONE / (f32(sigma) * f32(sigma))
    u1, v1, u2, v2 = (pts[None, :, k] for k in range(4))
    h = lambda M, r, c: M[:, r, c][:, None]   # noqa: E731
    with np.errstate(all="ignore"):
        w = ONE / ((h(H12, 2, 0) * u2 + h(H12, 2, 1) * v2) + h(H12, 2, 2))
        a = ((h(H12, 0, 0) * u2 + h(H12, 0, 1) * v2) + h(H12, 0, 2)) * w
        b = ((h(H12, 1, 0) * u2 + h(H12, 1, 1) * v2) + h(H12, 1, 2)) * w
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv
        w = ONE / ((h(H21, 2, 0) * u1 + h(H21, 2, 1) * v1) + h(H21, 2, 2))
        a = ((h(H21, 0, 0) * u1 + h(H21, 0, 1) * v1) + h(H21, 0, 2)) * w
        b = ((h(H21, 1, 0) * u1 + h(H21, 1, 1) * v1) + h(H21, 1, 2)) * w
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv
        out1, out2 = chi1 > th, chi2 > th
        score = _accumulate(np.where(out1, f32(0), th - chi1), np.where(out2, f32(0), th - chi2))
    return score, ~out1 & ~out2


def check_fundamental(F, pts, sigma):
    th, ths = f32(3.841), f32(5.991)
    inv = ONE / (f32(sigma) * f32(sigma))
    u1, v1, u2, v2 = (pts[None, :, k] for k in range(4))
    f = lambda r, c: F[:, r, c][:, None]   # noqa: E731
    with np.errstate(all="ignore"):
        a2 = (f(0, 0) * u1 + f(0, 1) * v1) + f(0, 2)
        b2 = (f(1, 0) * u1 + f(1, 1) * v1) + f(1, 2)
        c2 = (f(2, 0) * u1 + f(2, 1) * v1) + f(2, 2)
        num2 = (a2 * u2 + b2 * v2) + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv
        a1 = (f(0, 0) * u2 + f(1, 0) * v2) + f(2, 0)
        b1 = (f(0, 1) * u2 + f(1, 1) * v2) + f(2, 1)
        c1 = (f(0, 2) * u2 + f(1, 2) * v2) + f(2, 2)
        num1 = (a1 * u1 + b1 * v1) + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv
        out1, out2 = chi1 > th, chi2 > th
        score = _accumulate(np.where(out1, f32(0), ths - chi1), np.where(out2, f32(0), ths - chi2))
    return score, ~out1 & ~out2


def one_ulp(M, rng):
    M = np.asarray(M, f32)
    up = rng.integers(0, 2, M.shape).astype(bool)
    return np.where(up, np.nextafter(M, f32(np.inf)), np.nextafter(M, f32(-np.inf))).astype(f32)


def kmat(cam):
    fx, fy, cx, cy = (f64(v) for v in cam)
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f64)


def decompose_e(F21, cam):
    """(R, t) of ReconstructF's four CheckRT calls, float32."""
    K = kmat(cam)
    E = (K.T @ F21.astype(f64)) @ K
    U, _, Vt = svd(E, "e")
    t = U[:, 2] / np.linalg.norm(U[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f64)
    R1 = (U @ W) @ Vt
    if np.linalg.det(R1) < 0:
        R1 = -R1
    R2 = (U @ W.T) @ Vt
    if np.linalg.det(R2) < 0:
        R2 = -R2
    R1, R2, t = R1.astype(f32), R2.astype(f32), t.astype(f32)
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def decompose_h(H21, cam):
    """None where ReconstructH returns early (:598), else its eight (R, t), float32."""
    K = kmat(cam)
    A = (np.linalg.inv(K) @ H21.astype(f64)) @ K
    U, w, Vt = svd(A, "hdec")
    s = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    d1, d2, d3 = (f32(v) for v in w)
    with np.errstate(all="ignore"):
        if f64(d1 / d2) < 1.00001 or f64(d2 / d3) < 1.00001:
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        out = []
        for h in range(8):
            i = h & 3
            Rp = np.eye(3)
            if h < 4:
                Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ct, -st[i], st[i], ct
                tp = np.array([x1[i] * (d1 - d3), 0, -x3[i] * (d1 - d3)], f64)
            else:
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cp, sp[i], -1, sp[i], -cp
                tp = np.array([x1[i] * (d1 + d3), 0, x3[i] * (d1 + d3)], f64)
            R = s * ((U @ Rp) @ Vt)
            t = U[:, 0] * tp[0] + U[:, 2] * tp[2]
            out.append((R.astype(f32), (t / np.linalg.norm(t)).astype(f32)))
    return out


def projections(R, t, cam):
    fx, fy, cx, cy = (f32(v) for v in cam)
    z = f32(0)
    P1 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], f32)
    Rt = np.concatenate([R, t[:, None]], 1).astype(f32)
    with np.errstate(all="ignore"):
        P2 = np.stack([(fx * Rt[0] + z * Rt[1]) + cx * Rt[2], (z * Rt[0] + fy * Rt[1]) + cy * Rt[2],
                       (z * Rt[0] + z * Rt[1]) + ONE * Rt[2]]).astype(f32)
        O2 = ((-R[0]) * t[0] + (-R[1]) * t[1]) + (-R[2]) * t[2]
    return P1, P2, O2.astype(f32)


def triangulate(P1, P2, pts):
    """x3D (n, 3) in fp64, before the narrowing."""
    u1, v1, u2, v2 = (pts[:, k][:, None] for k in range(4))
    A = np.stack([u1 * P1[2] - P1[0], v1 * P1[2] - P1[1], u2 * P2[2] - P2[0], v2 * P2[2] - P2[1]], 1).astype(f32)
    if not np.isfinite(A).all():
        return np.full((len(pts), 3), np.nan)
    v = svd(A, "tri")[2][:, 3, :]
    with np.errstate(all="ignore"):
        return v[:, :3] / v[:, 3:4]


def check_rt(R, t, cam, pts, mask, th2):
    """CheckRT (:799-908): nGood, parallax, p3d (N, 3), counted (N), vbGood (N) over the correspondences."""
    N = len(pts)
    fx, fy, cx, cy = (f32(v) for v in cam)
    P1, P2, O2 = projections(R, t, cam)
    p3d = np.zeros((N, 3), f32)
    counted = np.zeros(N, bool)
    good = np.zeros(N, bool)
    cosp = np.zeros(N, f32)
    idx = np.nonzero(mask)[0]
    if len(idx) == 0:
        return 0, f32(0), p3d, counted, good
    q = pts[idx]
    with np.errstate(all="ignore"):
        x = triangulate(P1, P2, q).astype(f32)
        X, Y, Z = x[:, 0], x[:, 1], x[:, 2]
        ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
        n2 = x - O2[None, :]
        d1 = np.sqrt((X.astype(f64) * X + Y.astype(f64) * Y) + Z.astype(f64) * Z).astype(f32)
        d2 = np.sqrt((n2[:, 0].astype(f64) * n2[:, 0] + n2[:, 1].astype(f64) * n2[:, 1]) + n2[:, 2].astype(f64) * n2[:, 2]).astype(f32)
        dot = (X.astype(f64) * n2[:, 0] + Y.astype(f64) * n2[:, 1]) + Z.astype(f64) * n2[:, 2]
        cp = (dot / (d1 * d2).astype(f64)).astype(f32)
        low = cp.astype(f64) < 0.99998
        ok &= ~((Z <= 0) & low)
        X2 = ((R[0, 0] * X + R[0, 1] * Y) + R[0, 2] * Z) + t[0]
        Y2 = ((R[1, 0] * X + R[1, 1] * Y) + R[1, 2] * Z) + t[1]
        Z2 = ((R[2, 0] * X + R[2, 1] * Y) + R[2, 2] * Z) + t[2]
        ok &= ~((Z2 <= 0) & low)
        iz = ONE / Z
        ix, iy = fx * X * iz + cx, fy * Y * iz + cy
        e1 = (ix - q[:, 0]) * (ix - q[:, 0]) + (iy - q[:, 1]) * (iy - q[:, 1])
        ok &= ~(e1 > th2)
        iz = ONE / Z2
        ix, iy = fx * X2 * iz + cx, fy * Y2 * iz + cy
        e2 = (ix - q[:, 2]) * (ix - q[:, 2]) + (iy - q[:, 3]) * (iy - q[:, 3])
        ok &= ~(e2 > th2)
    counted[idx] = ok
    good[idx] = ok & low
    p3d[idx[ok]] = x[ok]
    cosp[idx] = cp
    n_good = int(ok.sum())
    parallax = f32(0)
    if n_good > 0:
        c = np.nonzero(counted)[0]
        order = c[np.lexsort((c, cosp[c]))]
        pick = cosp[order[min(50, n_good - 1)]]
        with np.errstate(invalid="ignore"):
            parallax = f32(np.arccos(f64(pick)) * 180 / np.pi)
    return n_good, parallax, p3d, counted, good


def decide_f(g, par, N, min_parallax, min_tri):
    """ReconstructF (:500-570): the winning index or -1."""
    max_good = max(g[:4])
    n_min = max(int(0.9 * N), min_tri)
    nsimilar = sum(1 for v in g[:4] if v > 0.7 * max_good)
    if max_good < n_min or nsimilar > 1:
        return -1
    first = [v == max_good for v in g[:4]].index(True)
    return first if par[first] > f32(min_parallax) else -1


def decide_h(g, par, N, min_parallax, min_tri):
    """ReconstructH (:690-730)."""
    best = second = 0
    idx, bp = -1, f32(-1)
    for i in range(8):
        if g[i] > best:
            second, best, idx, bp = best, g[i], i, par[i]
        elif g[i] > second:
            second = g[i]
    if second < 0.75 * best and bp >= f32(min_parallax) and best > min_tri and best > 0.9 * N:
        return idx
    return -1


def params(b):
    d = dict(sigma=1.0, max_iterations=200, min_parallax=1.0, min_triangulated=50, rh_threshold=0.40, rand_max=2147483647)
    return {k: b[k] if b.get(k) is not None else v for k, v in d.items()}


def initialize_pair(b, p, jitter=None):
    prm = params(b)
    T = int(prm["max_iterations"])
    k1, k1e = int(b["kp1_begin"][p]), int(b["kp1_begin"][p + 1])
    k2, k2e = int(b["kp2_begin"][p]), int(b["kp2_begin"][p + 1])
    n1 = k1e - k1
    xy1 = np.asarray(b["kp1_xy"], f32).reshape(-1, 2)[k1:k1e]
    xy2 = np.asarray(b["kp2_xy"], f32).reshape(-1, 2)[k2:k2e]
    m12 = np.asarray(b["matches12"])[k1:k1e]
    cam = np.asarray(b["camera"], f32).reshape(-1, 4)[p]
    r = dict(found=0, model=1, r21t21=np.zeros(12, f32), p3d=np.zeros((n1, 3), f32), triangulated=np.zeros(n1, np.uint8),
             score_h=f32(0), score_f=f32(0), best_h=-1, best_f=-1, h21=np.zeros(9, f32), f21=np.zeros(9, f32),
             inlier_h=np.zeros(n1, np.uint8), inlier_f=np.zeros(n1, np.uint8), hyp_score=np.zeros((2, T), f32),
             n_good=np.zeros(8, np.int32), parallax=np.zeros(8, f32), lead=[np.inf, np.inf], set_id=np.zeros(T, np.int64), rh=np.nan, counted=np.zeros(n1, bool))
    if n1 > MAXKP or k2e - k2 > MAXKP:
        r["found"], r["model"] = -1, 0
        return r
    slots = np.nonzero(m12 >= 0)[0]
    N = len(slots)
    r["N"] = N
    if N < 8:
        return r
    pts = np.concatenate([xy1[slots], xy2[m12[slots]]], 1).astype(f32)
    mean1, s1, T1 = normalize(xy1)
    mean2, s2, T2 = normalize(xy2)
    pn1 = ((pts[:, :2] - mean1) * s1).astype(f32)
    pn2 = ((pts[:, 2:] - mean2) * s2).astype(f32)
    draws = np.asarray(b["draws"]).reshape(-1, T, 8)[p]
    sets = np.array([pick8(draws[it], int(prm["rand_max"]), N) for it in range(T)])
    # hypotheses that drew the same eight correspondences (in any order) share an id: they name one model
    keys = {}
    r["set_id"] = np.array([keys.setdefault(tuple(sorted(row)), len(keys)) for row in sets.tolist()], np.int64)
    with np.errstate(all="ignore"):
        H21 = hypothesis_h(pn1[sets], pn2[sets], T1, T2)[1].astype(f32)
        F21 = hypothesis_f(pn1[sets], pn2[sets], T1, T2)[2].astype(f32)
        if jitter is not None:
            rng = np.random.default_rng([jitter, p])
            H21, F21 = one_ulp(H21, rng), one_ulp(F21, rng)
        H12 = np.stack([inverse_f32(M) for M in H21]).astype(f32)
        if jitter is not None:
            H12 = one_ulp(H12, rng)
    sh, ih = check_homography(H21, H12, pts, prm["sigma"])
    sf, if_ = check_fundamental(F21, pts, prm["sigma"])
    r["hyp_score"] = np.stack([sh, sf])
    mats = {}
    for name, s, inl, M in (("h", sh, ih, H21), ("f", sf, if_, F21)):
        best, bs = -1, f32(0)
        for it in range(T):
            if s[it] > bs:
                best, bs = it, s[it]
        r["score_" + name], r["best_" + name] = bs, best
        if best >= 0:
            mats[name] = M[best]
            r[name + "21"] = M[best].reshape(9).copy()
            r["inlier_" + name][slots] = inl[best]
            rest = s[r["set_id"] != r["set_id"][best]]
            rest = rest[np.isfinite(rest)]
            r["lead"][0 if name == "h" else 1] = float(bs) - float(rest.max()) if len(rest) else np.inf
    with np.errstate(all="ignore"):
        rh = r["score_h"] / (r["score_h"] + r["score_f"])
    r["rh"] = rh
    model = 0 if f64(rh) > prm["rh_threshold"] else 1
    r["model"] = model
    name = "hf"[model]
    if name not in mats:
        return r
    mask = r["inlier_" + name][slots].astype(bool)
    hyps = decompose_h(mats[name], cam) if model == 0 else decompose_e(mats[name], cam)
    if hyps is None:
        return r
    th2 = f32(4) * (f32(prm["sigma"]) * f32(prm["sigma"]))
    runs = [check_rt(R, t, cam, pts, mask, th2) for R, t in hyps]
    for j, run in enumerate(runs):
        r["n_good"][j], r["parallax"][j] = run[0], run[1]
    Nin = int(mask.sum())
    win = (decide_h if model == 0 else decide_f)(r["n_good"].tolist(), r["parallax"], Nin, prm["min_parallax"],
                                                 int(prm["min_triangulated"]))
    if win >= 0:
        R, t = hyps[win]
        _, _, p3d, counted, good = runs[win]
        r["found"] = 1
        r["r21t21"] = np.concatenate([R.reshape(9), t]).astype(f32)
        r["p3d"][slots] = p3d
        r["triangulated"][slots] = good
        r["counted"][slots] = counted
    return r


_FLAT = ("found", "model", "r21t21", "score_h", "score_f", "best_h", "best_f", "h21", "f21", "hyp_score", "n_good", "parallax", "set_id")
_SLOT = ("p3d", "triangulated", "inlier_h", "inlier_f", "counted")


def initialize(b, jitter=None):
    """Every pair of the batch; the outputs in orb_initializer_result's shapes, plus lead (F, 2) = the best score's
    lead over the runner-up per model among the hypotheses of another set_id (F, T), rh (F) and counted (total_kp1) = where p3d was set."""
    F = len(b["kp1_begin"]) - 1
    rs = [initialize_pair(b, p, jitter) for p in range(F)]
    out = {k: np.stack([np.asarray(r[k]) for r in rs]) for k in _FLAT + ("lead", "rh")}
    for k in _SLOT:
        out[k] = np.concatenate([r[k] for r in rs]) if rs else np.zeros(0)
    return out


def rot_angle(Ra, Rb):
    c = (np.trace(Ra.astype(f64).reshape(3, 3).T @ Rb.astype(f64).reshape(3, 3)) - 1) / 2
    d = np.linalg.norm(Ra.astype(f64) - Rb.astype(f64))
    return float(d) if c > 0.999999 else float(np.arccos(np.clip(c, -1, 1)))   # |Ra - Rb|_F ~ sqrt(2) x the angle


def pose_distance(a, c):
    """(rotation in rad, |dt| / |t|) between two r21t21."""
    a, c = np.asarray(a, f32), np.asarray(c, f32)
    nt = max(float(np.linalg.norm(a[9:].astype(f64))), 1e-30)
    return rot_angle(a[:9], c[:9]), float(np.linalg.norm(a[9:].astype(f64) - c[9:].astype(f64))) / nt


def point_distance(a, c):
    """max over points of |da| / depth."""
    a, c = np.asarray(a, f64).reshape(-1, 3), np.asarray(c, f64).reshape(-1, 3)
    if len(a) == 0:
        return 0.0
    return float((np.linalg.norm(a - c, axis=1) / np.maximum(np.abs(a[:, 2]), 1e-30)).max())


def ulp(x):
    x = np.abs(np.asarray(x, f32))
    return (np.nextafter(x, f32(np.inf)) - x).astype(f64)
