"""numpy restatement of PnPsolver (src/PnPsolver.cc) in the batch layout of orb_pnpsolver_batch
(include/orbslam2_amd.h): float64 where the reference computes in double, float32 where it computes in float
(CheckInliers, mvMaxError).  tests/test_pnpsolver_ref.py pins it; tests/test_pnpsolver_gpu.py holds the device to it.

Where the reference reads an OpenCV SVD whose rounding decides the answer, the rules of DESIGN.md section 4
(PnPsolver) stand, computed through numpy.linalg and not through the device's Jacobi:
  control-point axes   numpy.linalg.eigh of PW0^T PW0, descending, largest-magnitude component positive
  minimal-set basis    n = 4: the projector P = N^T N onto the null space of M from numpy.linalg.svd, then pivoted
                       Gram-Schmidt on its columns (largest remaining diagonal, lowest index on a tie), v[0..3] in
                       pivot order
  Refine null vectors  numpy.linalg.eigh of MtM, the four smallest ascending, largest-magnitude component positive
  R of ABt             U Vh of numpy.linalg.svd, then the reference's det < 0 rule (row 2 negated)
The three cv::solve(DECOMP_SVD) calls and qr_solve are least-squares solves: the device uses Householder QR, this
file numpy.linalg.pinv.  Sums are numpy's.

Every hypothesis of a candidate is evaluated at once (arrays over k); the control flow of iterate() then walks the
counts.  iterate() also returns per hypothesis the bounds lo[k] <= n[k] <= hi[k] of the count when every
correspondence whose error2 lies within the relative margin `margin` of its gate is flipped."""
import math

import numpy as np

f32 = np.float32
RAND_MAX = 2147483647
RELOC = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991, maxk=5)


# ---------------------------------------------------------------- SetRansacParameters (:121-157)
def ransac_parameters(N, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5):
    """(minInliers, eps, cap) for N correspondences; libm through math.*."""
    mi = max(int(f32(N) * f32(epsilon)), min_inliers, min_set)
    eps = f32(epsilon)
    if N > 0 and eps < f32(mi) / f32(N):
        eps = f32(mi) / f32(N)
    if mi == N:
        it = 1
    elif N < mi:
        it = 1   # not used: iterate() returns first
    else:
        try:
            it = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3)))
        except (ZeroDivisionError, ValueError):
            it = max_iterations
    return mi, float(eps), max(1, min(it, max_iterations))


# ---------------------------------------------------------------- draws (:188-201)
def random_int(r, d, rand_max=RAND_MAX):
    return int((float(r) / (float(rand_max) + 1.0)) * d)


def pick(draw, n, rand_max=RAND_MAX):
    """The four indices of a hypothesis (swap with the back, pop) without the vector."""
    over, idx = {}, []
    for c in range(4):
        d = n - c
        r = random_int(draw[c], d, rand_max)
        idx.append(over.get(r, r))
        over[r] = over.get(d - 1, d - 1)
    return idx


# ---------------------------------------------------------------- EPnP (:375-955), arrays over k
def _sign_rows(V):
    """(K, m, d): every row signed so that its largest-magnitude component (lowest index on a tie) is positive."""
    at = np.argmax(np.abs(V), -1)
    s = np.where(np.take_along_axis(V, at[..., None], -1)[..., 0] < 0, -1.0, 1.0)
    return V * s[..., None]


def _clean(A):
    """A with every non-finite matrix replaced by the identity pattern, and the mask of the replaced ones."""
    bad = ~np.isfinite(A).all((-1, -2))
    if bad.any():
        A = A.copy()
        A[bad] = np.eye(A.shape[-2], A.shape[-1])
    return A, bad


def _lstsq(A, b):
    A, bad = _clean(A)
    x = (np.linalg.pinv(A) @ np.where(np.isfinite(b), b, 0.0)[..., None])[..., 0]
    x[bad | ~np.isfinite(b).all(-1)] = np.nan
    return x


def null_basis_minimal(M, rotate=None):
    """v (K, 4, 12) of M (K, 8, 12).  rotate: a (4, 4) orthogonal matrix applied to the SVD's null vectors first
    (the rule must not see it)."""
    M, bad = _clean(M)
    N = np.linalg.svd(M)[2][:, 8:, :]
    if rotate is not None:
        N = np.einsum("ij,kjd->kid", rotate, N)
    P = np.einsum("kid,kie->kde", N, N)
    v = np.zeros((len(M), 4, 12))
    ar = np.arange(len(M))
    for t in range(4):
        j = np.argmax(np.diagonal(P, axis1=1, axis2=2), 1)
        col = P[ar, :, j]
        v[:, t] = col / np.sqrt(P[ar, j, j])[:, None]
        P = P - v[:, t, :, None] * v[:, t, None, :]
    v[bad] = np.nan
    return v


def null_basis_refine(MtM):
    MtM, bad = _clean(MtM)
    _, V = np.linalg.eigh(MtM)
    v = _sign_rows(np.swapaxes(V[:, :, :4], 1, 2))
    v[bad] = np.nan
    return v


_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def epnp(pw, us, cam, minimal, jitter=None, rotate=None, detail=False):
    """compute_pose for K problems of n correspondences: pw (K, n, 3), us (K, n, 2) float64, cam = fu, fv, uc, vc.
    Returns R (K, 3, 3), t (K, 3).  jitter: a Generator; every non-zero entry of M moves one ulp up or down."""
    with np.errstate(all="ignore"):
        pw, us = np.asarray(pw, np.float64), np.asarray(us, np.float64)
        K, n, _ = pw.shape
        fu, fv, uc, vc = (float(c) for c in cam)
        c0 = pw.sum(1) / n
        PW0 = pw - c0[:, None]
        S, bad0 = _clean(np.einsum("kni,knj->kij", PW0, PW0))
        w, E = np.linalg.eigh(S)
        w, E = w[:, ::-1], _sign_rows(np.swapaxes(E, 1, 2)[:, ::-1])   # rows: axes, descending
        kk = np.sqrt(np.maximum(w, 0.0) / n)
        cws = np.concatenate([c0[:, None], c0[:, None] + kk[:, :, None] * E], 1)   # (K, 4, 3)
        ci = E / kk[:, :, None]
        al = np.zeros((K, n, 4))
        al[:, :, 1:] = (ci[:, None, :, 0] * PW0[:, :, None, 0] + ci[:, None, :, 1] * PW0[:, :, None, 1]) + ci[:, None, :, 2] * PW0[:, :, None, 2]
        al[:, :, 0] = 1.0 - al[:, :, 1] - al[:, :, 2] - al[:, :, 3]
        M = np.zeros((K, 2 * n, 12))
        for i in range(4):
            M[:, 0::2, 3 * i] = al[:, :, i] * fu
            M[:, 0::2, 3 * i + 2] = al[:, :, i] * (uc - us[:, :, 0])
            M[:, 1::2, 3 * i + 1] = al[:, :, i] * fv
            M[:, 1::2, 3 * i + 2] = al[:, :, i] * (vc - us[:, :, 1])
        if jitter is not None:
            up = jitter.integers(0, 2, M.shape).astype(bool)
            M = np.where(M == 0, 0.0, np.where(up, np.nextafter(M, np.inf), np.nextafter(M, -np.inf)))
        v = null_basis_minimal(M, rotate) if minimal else null_basis_refine(np.einsum("kri,krj->kij", M, M))
        dv = np.stack([v[:, :, 3 * a:3 * a + 3] - v[:, :, 3 * b:3 * b + 3] for a, b in _PAIRS], 2)   # (K, 4, 6, 3)
        dot = lambda i, j: (dv[:, i] * dv[:, j]).sum(-1)   # noqa: E731
        L = np.stack([dot(0, 0), 2 * dot(0, 1), dot(1, 1), 2 * dot(0, 2), 2 * dot(1, 2), dot(2, 2), 2 * dot(0, 3), 2 * dot(1, 3),
                      2 * dot(2, 3), dot(3, 3)], 2)   # (K, 6, 10)
        rho = np.stack([((cws[:, a] - cws[:, b]) ** 2).sum(-1) for a, b in _PAIRS], 1)
        betas = []
        x = _lstsq(L[:, :, [0, 1, 3, 6]], rho)
        sg = np.where(x[:, 0] < 0, -1.0, 1.0)
        b0 = np.sqrt(sg * x[:, 0])
        betas.append(np.stack([b0, sg * x[:, 1] / b0, sg * x[:, 2] / b0, sg * x[:, 3] / b0], 1))
        for cols in ([0, 1, 2], [0, 1, 2, 3, 4]):
            x = _lstsq(L[:, :, cols], rho)
            neg = x[:, 0] < 0
            b0 = np.sqrt(np.where(neg, -x[:, 0], x[:, 0]))
            b1 = np.where(neg, np.where(x[:, 2] < 0, np.sqrt(-x[:, 2]), 0.0), np.where(x[:, 2] > 0, np.sqrt(x[:, 2]), 0.0))
            b0 = np.where(x[:, 1] < 0, -b0, b0)
            b2 = x[:, 3] / b0 if len(cols) == 5 else np.zeros(K)
            betas.append(np.stack([b0, b1, b2, np.zeros(K)], 1))
        Rs, ts, errs = [], [], []
        for be in betas:
            for _ in range(5):   # gauss_newton
                A = np.stack([2 * L[:, :, 0] * be[:, None, 0] + L[:, :, 1] * be[:, None, 1] + L[:, :, 3] * be[:, None, 2] + L[:, :, 6] * be[:, None, 3],
                              L[:, :, 1] * be[:, None, 0] + 2 * L[:, :, 2] * be[:, None, 1] + L[:, :, 4] * be[:, None, 2] + L[:, :, 7] * be[:, None, 3],
                              L[:, :, 3] * be[:, None, 0] + L[:, :, 4] * be[:, None, 1] + 2 * L[:, :, 5] * be[:, None, 2] + L[:, :, 8] * be[:, None, 3],
                              L[:, :, 6] * be[:, None, 0] + L[:, :, 7] * be[:, None, 1] + L[:, :, 8] * be[:, None, 2] + 2 * L[:, :, 9] * be[:, None, 3]], 2)
                bb = [be[:, 0] * be[:, 0], be[:, 0] * be[:, 1], be[:, 1] * be[:, 1], be[:, 0] * be[:, 2], be[:, 1] * be[:, 2],
                      be[:, 2] * be[:, 2], be[:, 0] * be[:, 3], be[:, 1] * be[:, 3], be[:, 2] * be[:, 3], be[:, 3] * be[:, 3]]
                b = rho - sum(L[:, :, i] * bb[i][:, None] for i in range(10))
                be = be + _lstsq(A, b)
            ccs = np.einsum("ki,kid->kd", be, v).reshape(K, 4, 3)
            pcs = np.einsum("kni,kid->knd", al, ccs)
            flip = np.where(pcs[:, 0, 2] < 0, -1.0, 1.0)
            pcs = pcs * flip[:, None, None]
            pc0, pw0 = pcs.sum(1) / n, pw.sum(1) / n
            ABt, bad = _clean(np.einsum("kni,knj->kij", pcs - pc0[:, None], pw - pw0[:, None]))
            U, _, Vh = np.linalg.svd(ABt)
            R = U @ Vh
            R[np.linalg.det(R) < 0, 2] *= -1
            R[bad | bad0] = np.nan
            t = pc0 - np.einsum("kij,kj->ki", R, pw0)
            Xc = np.einsum("kij,knj->kni", R, pw) + t[:, None]
            inv = 1.0 / Xc[:, :, 2]
            ue, ve = uc + fu * Xc[:, :, 0] * inv, vc + fv * Xc[:, :, 1] * inv
            errs.append(np.sqrt((us[:, :, 0] - ue) ** 2 + (us[:, :, 1] - ve) ** 2).sum(1) / n)
            Rs.append(R)
            ts.append(t)
        N_ = np.zeros(K, np.int64)
        N_[errs[1] < errs[0]] = 1
        e_n = np.where(N_ == 1, errs[1], errs[0])
        N_[errs[2] < e_n] = 2
        R = np.choose(N_[:, None, None], Rs)
        t = np.choose(N_[:, None], ts)
        if detail:
            return R, t, dict(v=v, cws=cws, alphas=al, M=M, choice=N_)
        return R, t


def error2(R, t, cam, X, p2d):
    """CheckInliers (:308-339): R (K, 3, 3), t (K, 3) float64, X (N, 3), p2d (N, 2) float32 -> error2 (K, N) float32."""
    with np.errstate(all="ignore"):
        fu, fv, uc, vc = (float(c) for c in cam)
        Xd = X.astype(np.float64)
        q = [(((R[:, i, 0, None] * Xd[None, :, 0] + R[:, i, 1, None] * Xd[None, :, 1]) + R[:, i, 2, None] * Xd[None, :, 2]) + t[:, i, None])
             for i in range(3)]
        Xc, Yc, invZc = q[0].astype(f32), q[1].astype(f32), (1 / q[2]).astype(f32)
        ue = uc + fu * Xc.astype(np.float64) * invZc.astype(np.float64)
        ve = vc + fv * Yc.astype(np.float64) * invZc.astype(np.float64)
        dx = (p2d[None, :, 0].astype(np.float64) - ue).astype(f32)
        dy = (p2d[None, :, 1].astype(np.float64) - ve).astype(f32)
        return (dx * dx + dy * dy).astype(f32)


def gates(e2, max_err, margin=0.0):
    """(inlier (K, N), lo (K), hi (K)): the strict float < and the counts with the gate moved by the margin."""
    inl = e2 < max_err[None]
    e, g = e2.astype(np.float64), max_err.astype(np.float64)[None]
    with np.errstate(all="ignore"):
        return inl, (e < g * (1 - margin)).sum(1), (e < g * (1 + margin)).sum(1)


# ---------------------------------------------------------------- the constructor (:67-110)
class Candidate:
    def __init__(self, b, p):
        k0, k1 = int(b["kp_begin"][p]), int(b["kp_begin"][p + 1])
        self.k0, self.nkp = k0, k1 - k0
        self.slots = np.nonzero(np.asarray(b["mp_valid"][k0:k1]))[0]
        self.N = len(self.slots)
        self.cam = np.asarray(b["camera"], f32).reshape(-1, 4)[p]
        self.P2D = np.asarray(b["kp_xy"], f32).reshape(-1, 2)[k0:k1][self.slots]
        self.P3D = np.asarray(b["mp_xw"], f32).reshape(-1, 3)[k0:k1][self.slots]
        sig = np.asarray(b["level_sigma2"], f32)
        self.max_err = (sig[np.asarray(b["kp_octave"])[k0:k1][self.slots]] * f32(_param(b, "th2"))).astype(f32)

    def hypotheses(self, draws, rand_max=RAND_MAX, jitter=None):
        idx = np.array([pick(d, self.N, rand_max) for d in draws], np.int64).reshape(-1, 4)
        return epnp(self.P3D[idx], self.P2D[idx], self.cam, True, jitter)

    def refine(self, mask, jitter=None):
        """Refine() (:260-305) on a mask over the correspondences: R, t (3, 3), (3,), error2 (N,)."""
        R, t = epnp(self.P3D[mask][None], self.P2D[mask][None], self.cam, False, jitter)
        return R[0], t[0], error2(R, t, self.cam, self.P3D, self.P2D)[0]


def _param(b, k):
    return RELOC[k] if b.get(k) is None else b[k]


def _tcw(R, t):
    return np.concatenate([np.asarray(R).reshape(9), np.asarray(t).reshape(3)]).astype(f32)


def iterate(b, margin=0.0, jitter_seed=None, cands=None):
    """One iterate(maxk) of every candidate's solver.  Returns the outputs of orb_pnpsolver_iterate plus n, lo, hi
    (F, n_draws; -1 where not evaluated), refines (per candidate: a list of dicts k, n, lo, hi, tcw, near) and cap,
    min_inliers_adj, N."""
    F, K = len(b["kp_begin"]) - 1, int(b["kp_begin"][-1])
    prm = {k: _param(b, k) for k in RELOC}
    rand_max = RAND_MAX if b.get("rand_max") is None else int(b["rand_max"])
    draws = np.asarray(b["draws"]).reshape(F, -1, 4)
    D = draws.shape[1]
    st = lambda k, shape, dt: np.zeros(shape, dt) if b.get(k) is None else np.array(b[k], dt).reshape(shape)   # noqa: E731
    out = dict(tcw=np.zeros((F, 12), f32), inlier=np.zeros(K, np.uint8), found=np.zeros(F, np.int32), n_inliers=np.zeros(F, np.int32),
               terminate=np.zeros(F, np.int32), iterations=st("iterations", F, np.int32), best_inliers=st("best_inliers", F, np.int32),
               best_mask=st("best_mask", K, np.uint8), best_tcw=st("best_tcw", (F, 12), f32),
               hyp_inliers=np.full((F, D), -1, np.int32), n=np.full((F, D), -1, np.int32), lo=np.full((F, D), -1, np.int32),
               hi=np.full((F, D), -1, np.int32), refines=[[] for _ in range(F)], cap=np.zeros(F, np.int32),
               min_inliers_adj=np.zeros(F, np.int32), N=np.zeros(F, np.int32), err=[None] * F, best_in=st("best_inliers", F, np.int32).copy())
    for p in (range(F) if cands is None else cands):
        g = Candidate(b, p)
        out["N"][p] = g.N
        if g.nkp > 8192:
            out["found"][p], out["terminate"][p] = -1, 1
            continue
        mi, _, cap = ransac_parameters(g.N, prm["probability"], int(prm["min_inliers"]), int(prm["max_iterations"]), int(prm["min_set"]),
                                       prm["epsilon"])
        out["cap"][p], out["min_inliers_adj"][p] = cap, mi
        if g.N < mi:
            out["terminate"][p] = 1
            continue
        k0 = int(out["iterations"][p])
        k1 = max(cap, k0 + int(prm["maxk"]))   # the OR of :182
        if k1 > D:
            out["found"][p], out["terminate"][p] = -1, 1
            continue
        jit = None if jitter_seed is None else np.random.default_rng([jitter_seed, p])
        R, t = g.hypotheses(draws[p, k0:k1], rand_max, jit)
        e2 = error2(R, t, g.cam, g.P3D, g.P2D)
        inl, lo, hi = gates(e2, g.max_err, margin)
        out["err"][p] = e2
        out["n"][p, k0:k1], out["lo"][p, k0:k1], out["hi"][p, k0:k1] = inl.sum(1), lo, hi
        best = int(out["best_inliers"][p])
        mask = out["best_mask"][g.k0 + g.slots].astype(bool)
        first, done = True, False
        for k in range(k0, k1):
            nk = int(out["n"][p, k])
            out["hyp_inliers"][p, k] = nk
            if nk < mi:
                continue
            record = nk > best
            if record:
                best, mask = nk, inl[k - k0].copy()
                out["best_tcw"][p] = _tcw(R[k - k0], t[k - k0])
            if record or first:   # an unchanged mask refines to the same failure
                Rr, tr, er = g.refine(mask, jit)
                ri, rlo, rhi = gates(er[None], g.max_err, margin)
                out["refines"][p].append(dict(k=k, n=int(ri.sum()), lo=int(rlo[0]), hi=int(rhi[0]), tcw=_tcw(Rr, tr), err=er))
                if ri.sum() > mi:
                    out["found"][p], out["n_inliers"][p], out["iterations"][p] = 1, ri.sum(), k + 1
                    out["tcw"][p] = _tcw(Rr, tr)
                    out["inlier"][g.k0 + g.slots[ri[0]]] = 1
                    done = True
            first = False
            if done:
                break
        out["best_inliers"][p] = best
        full = np.zeros(g.nkp, np.uint8)
        full[g.slots[mask]] = 1
        if best >= mi or mask.any():
            out["best_mask"][g.k0:g.k0 + g.nkp] = full
        if not done:
            out["iterations"][p] = k1
            out["terminate"][p] = int(k1 >= cap)
            if out["terminate"][p] and best >= mi:
                out["found"][p], out["n_inliers"][p] = 2, best
                out["tcw"][p] = out["best_tcw"][p]
                out["inlier"][g.k0:g.k0 + g.nkp] = full
    return out


def stop_is_decided(r, b, p):
    """The control flow of candidate p in the result r of iterate(b, margin) is the same for every count inside
    [lo, hi]: every evaluated hypothesis is an event for all of them or for none (lo >= minInliers or hi <
    minInliers), the events are ordered against the running best the same way (a record has lo > every earlier
    event's hi and the incoming best, a non-record hi <= some earlier lo or the incoming best), and every Refine()
    succeeds for all counts or for none (lo > minInliers or hi <= minInliers)."""
    mi = int(r["min_inliers_adj"][p])
    ev = np.nonzero(r["hyp_inliers"][p] >= 0)[0]
    best_lo = best_hi = int(r["best_in"][p])
    for k in ev:
        lo, hi, n = int(r["lo"][p, k]), int(r["hi"][p, k]), int(r["n"][p, k])
        if not (lo >= mi or hi < mi):
            return False
        if hi < mi:
            continue
        if n > best_hi or lo > best_hi:
            if not lo > best_hi:
                return False
            best_lo, best_hi = lo, hi
        elif not hi <= best_lo:
            return False
    return all(f["lo"] > mi or f["hi"] <= mi for f in r["refines"][p])


def spread(a, b):
    """(rotation angle [rad], |dt| / |t|) between two rows R, t."""
    Ra, Rb = np.asarray(a[:9], np.float64).reshape(3, 3), np.asarray(b[:9], np.float64).reshape(3, 3)
    dR = Ra @ Rb.T
    ang = math.atan2(np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2, (np.trace(dR) - 1) / 2)
    ta, tb = np.asarray(a[9:12], np.float64), np.asarray(b[9:12], np.float64)
    return np.array([abs(ang), np.linalg.norm(ta - tb) / np.linalg.norm(ta)])
