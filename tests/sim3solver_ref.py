"""numpy restatement of Sim3Solver (src/Sim3Solver.cc:206-365, include/Sim3.h:40-47) in the batch layout of
orb_sim3solver_batch (include/orbslam2_amd.h): float32 wherever the reference computes in float, float64 where it
computes in double, the rotation by numpy.linalg.svd in float64 on the float32 M (U S Vh of svd(M^T) with the
determinant rule), then rounded to float32.  tests/test_sim3solver_ref.py pins it; tests/test_sim3solver_gpu.py
holds the device to it.

The accumulation orders OpenCV's sources would decide and the reference checkout does not show are fixed as in
csrc/sim3_hyp.h: the centroid ((P(i,0) + P(i,1)) + P(i,2)) / 3.f, the 3x3 products ((a0 b0 + a1 b1) + a2 b2) in
float, Mat::dot with products and sum in double, row-major.

Every hypothesis of a pair is evaluated at once (arrays over k); the control flow of iterate() then walks the
counts.  Besides the result, iterate() returns per hypothesis the bounds lo[k] <= n[k] <= hi[k] of the count when
every correspondence whose errorSq lies within the relative margin `margin` of its threshold is flipped."""
import math

import numpy as np

f32 = np.float32
RAND_MAX = 2147483647


# ---------------------------------------------------------------- SetRansacParameters (:266-287)
def iteration_cap(nmatches, probability=0.99, min_inliers=20, max_iterations=300):
    """maxIterations_ for a pair with nmatches correspondences; libm through math.*.  Below min_inliers the value
    is not used (iterate() terminates first): 1."""
    if nmatches <= min_inliers:
        return 1
    epsilon = float(f32(f32(1.0) * f32(min_inliers)) / f32(nmatches))
    try:
        it = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(epsilon, 3)))
    except (ZeroDivisionError, ValueError):   # log(1 - 0) = 0 in the denominator: no bound from the probability
        it = max_iterations
    return max(1, min(it, max_iterations))


# ---------------------------------------------------------------- sampling (:307-322)
def random_int(r, d, rand_max=RAND_MAX):
    """DUtils::Random::RandomInt(0, d - 1) given rand() = r."""
    return int((float(r) / (float(rand_max) + 1.0)) * d)


def pick(draw, n, rand_max=RAND_MAX):
    """The three indices iterate() draws from availableIndices = 0 .. n - 1 (swap with the back, pop)."""
    avail = list(range(n))
    idx = []
    for c in range(3):
        randi = random_int(draw[c], len(avail), rand_max)
        idx.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return idx


# ---------------------------------------------------------------- ComputeSim3 (:111-163), arrays over k
def _mm(A, B):
    """(K, 3, 3) x (K, 3, 3) in float32, ((a0 b0 + a1 b1) + a2 b2)."""
    return (A[:, :, 0, None] * B[:, None, 0, :] + A[:, :, 1, None] * B[:, None, 1, :]) + A[:, :, 2, None] * B[:, None, 2, :]


def rotation(M, jitter=None):
    """R12 (K, 3, 3) float32 of the float32 M (K, 3, 3): U S Vh of svd(M^T) in float64, S(2,2) = -1 when
    det(U) det(Vh) < 0.  jitter: a Generator; every entry of M moves one float ulp up or down first."""
    M = np.asarray(M, f32)
    if jitter is not None:
        up = jitter.integers(0, 2, M.shape).astype(bool)
        M = np.where(up, np.nextafter(M, f32(np.inf)), np.nextafter(M, f32(-np.inf))).astype(f32)
    U, _, Vh = np.linalg.svd(np.swapaxes(M, 1, 2).astype(np.float64))
    S = np.tile(np.eye(3), (len(M), 1, 1))
    S[:, 2, 2] = np.where(np.linalg.det(U) * np.linalg.det(Vh) < 0, -1.0, 1.0)
    return (U @ S @ Vh).astype(f32)


def inverse(S):
    """Sim3::Inverse (Sim3.h:43-47) of rows (K, 13) float32: R^T, ((-(1 / s)) * R^T) * t, 1 / s."""
    R, t, s = S[:, :9].reshape(-1, 3, 3), S[:, 9:12], S[:, 12]
    inv_s = f32(1.0) / s
    A = (-inv_s)[:, None, None] * np.swapaxes(R, 1, 2)
    ti = (A[:, :, 0] * t[:, None, 0] + A[:, :, 1] * t[:, None, 1]) + A[:, :, 2] * t[:, None, 2]
    return np.concatenate([np.swapaxes(R, 1, 2).reshape(-1, 9), ti, inv_s[:, None]], 1).astype(f32)


def compute_sim3(P1, P2, fix_scale, jitter=None):
    """P1, P2 (K, 3 points, 3) float32 -> S12, S21 (K, 13) float32: R (row-major), t, s."""
    P1, P2 = np.swapaxes(np.asarray(P1, f32), 1, 2), np.swapaxes(np.asarray(P2, f32), 1, 2)   # (K, coordinate, point)
    with np.errstate(all="ignore"):
        O1 = ((P1[:, :, 0] + P1[:, :, 1]) + P1[:, :, 2]) / f32(3)
        O2 = ((P2[:, :, 0] + P2[:, :, 1]) + P2[:, :, 2]) / f32(3)
        Pr1, Pr2 = P1 - O1[:, :, None], P2 - O2[:, :, None]
        M = _mm(Pr2, np.swapaxes(Pr1, 1, 2))
        R = rotation(M, jitter)
        P3 = _mm(R, Pr2)
        K = len(P1)
        s = np.ones(K, f32)
        if not fix_scale:
            a, b = Pr1.reshape(K, 9), P3.reshape(K, 9)
            nom, den = np.zeros(K), np.zeros(K)
            for i in range(9):
                nom = nom + a[:, i].astype(np.float64) * b[:, i].astype(np.float64)
                den = den + (b[:, i] * b[:, i]).astype(np.float64)
            s = (nom / den).astype(f32)
        sR = s[:, None, None] * R
        t = O1 - ((sR[:, :, 0] * O2[:, None, 0] + sR[:, :, 1] * O2[:, None, 1]) + sR[:, :, 2] * O2[:, None, 2])
        S12 = np.concatenate([R.reshape(K, 9), t, s[:, None]], 1).astype(f32)
        return S12, inverse(S12)


def error_sq(S, cam, X, pts):
    """|pts - Project(X, S, cam)|^2 (:165-184, :335-338) in float32: S (K, 13), X (n, 3), pts (n, 2) -> (K, n)."""
    with np.errstate(all="ignore"):
        m = (S[:, 12, None] * S[:, :9]).reshape(-1, 3, 3)
        t = S[:, 9:12]
        q = [((m[:, i, 0, None] * X[None, :, 0] + m[:, i, 1, None] * X[None, :, 1]) + m[:, i, 2, None] * X[None, :, 2]) + t[:, i, None]
             for i in range(3)]
        invZ = f32(1.0) / q[2]
        u, v = q[0] * invZ, q[1] * invZ
        dx = pts[None, :, 0] - (cam[0] * u + cam[2])
        dy = pts[None, :, 1] - (cam[1] * v + cam[3])
        return (dx * dx + dy * dy).astype(f32)


# ---------------------------------------------------------------- the constructor (:206-264)
class Pair:
    def __init__(self, b, p):
        k1, k1e = int(b["kp1_begin"][p]), int(b["kp1_begin"][p + 1])
        k2, k2e = int(b["kp2_begin"][p]), int(b["kp2_begin"][p + 1])
        self.k1, self.n1 = k1, k1e - k1
        m = np.asarray(b["match12"][k1:k1e], np.int64)
        v2 = np.asarray(b["mp2_valid"][k2:k2e]).astype(bool)
        keep = np.asarray(b["mp1_valid"][k1:k1e]).astype(bool) & (m >= 0) & (m < k2e - k2)
        keep[keep] &= v2[m[keep]]
        self.slots = np.nonzero(keep)[0]
        self.m12 = m
        i2 = m[self.slots]
        self.n = len(self.slots)
        self.cam1, self.cam2 = np.asarray(b["camera1"][p], f32), np.asarray(b["camera2"][p], f32)

        def to_camera(P, X):
            P, X = np.asarray(P, f32), np.asarray(X, f32).reshape(-1, 3)
            return np.stack([((P[3 * i] * X[:, 0] + P[3 * i + 1] * X[:, 1]) + P[3 * i + 2] * X[:, 2]) + P[9 + i] for i in range(3)], 1)

        def to_image(cam, X):
            with np.errstate(all="ignore"):
                invZ = f32(1) / X[:, 2]
                return np.stack([cam[0] * (X[:, 0] * invZ) + cam[2], cam[1] * (X[:, 1] * invZ) + cam[3]], 1).astype(f32)

        self.X1 = to_camera(b["pose1"][p], np.asarray(b["mp1_xw"])[k1:k1e][self.slots])
        self.X2 = to_camera(b["pose2"][p], np.asarray(b["mp2_xw"])[k2:k2e][i2])
        self.pts1, self.pts2 = to_image(self.cam1, self.X1), to_image(self.cam2, self.X2)
        sig = np.asarray(b["level_sigma2"], f32)
        self.thr1 = 9.21 * sig[np.asarray(b["kp1_octave"])[k1:k1e][self.slots]].astype(np.float64)
        self.thr2 = 9.21 * sig[np.asarray(b["kp2_octave"])[k2:k2e][i2]].astype(np.float64)

    def hypotheses(self, draws, fix_scale, rand_max=RAND_MAX, jitter=None):
        """S12, S21 (K, 13) of the hypotheses with the draws (K, 3)."""
        idx = np.array([pick(d, self.n, rand_max) for d in draws], np.int64).reshape(-1, 3)
        return compute_sim3(self.X1[idx], self.X2[idx], fix_scale, jitter)

    def errors(self, S12, S21):
        """errorSq1, errorSq2 (K, n) float32."""
        return error_sq(S12, self.cam1, self.X2, self.pts1), error_sq(S21, self.cam2, self.X1, self.pts2)

    def inliers(self, e1, e2, margin=0.0):
        """(inlier (K, n), lo (K), hi (K))."""
        e1, e2 = e1.astype(np.float64), e2.astype(np.float64)
        inl = (e1 < self.thr1) & (e2 < self.thr2)
        lo = ((e1 < self.thr1 * (1 - margin)) & (e2 < self.thr2 * (1 - margin))).sum(1)
        hi = ((e1 < self.thr1 * (1 + margin)) & (e2 < self.thr2 * (1 + margin))).sum(1)
        return inl, lo, hi


def walk(counts, k0, k1, max_inliers, min_inliers):
    """:305-359 on the counts n[k0 .. k1): (k of the first success or -1, max_inliers afterwards)."""
    for k in range(k0, k1):
        if counts[k] >= max_inliers:
            max_inliers = int(counts[k])
            if counts[k] > min_inliers:
                return k, max_inliers
    return -1, max_inliers


def _param(b, k, default):
    return default if b.get(k) is None else b[k]


def iterate(b, margin=0.0, jitter_seed=None, pairs=None, stop=True):
    """One iterate(maxk) of every pair's solver (stop=False: the whole range is evaluated and no hypothesis succeeds).  Returns the outputs of orb_sim3solver_iterate plus n, lo, hi
    (F, max_iterations; -1 where not evaluated) and err (per pair: errorSq1, errorSq2 of the evaluated range)."""
    F, K1 = len(b["kp1_begin"]) - 1, int(b["kp1_begin"][-1])
    prob, mn, T, maxk = (_param(b, "probability", 0.99), int(_param(b, "min_inliers", 20)), int(_param(b, "max_iterations", 300)),
                         int(_param(b, "maxk", 5)))
    rand_max, fix_scale = int(_param(b, "rand_max", RAND_MAX)), bool(_param(b, "fix_scale", 0))
    draws = np.asarray(b["draws"]).reshape(F, T, 3)
    it_in = np.zeros(F, np.int32) if b.get("iterations") is None else np.asarray(b["iterations"], np.int32)
    mx_in = np.zeros(F, np.int32) if b.get("max_inliers") is None else np.asarray(b["max_inliers"], np.int32)
    out = dict(s12=np.zeros((F, 13), f32), inlier=np.zeros(K1, np.uint8), match12=np.full(K1, -1, np.int32),
               found=np.zeros(F, np.int32), n_inliers=np.zeros(F, np.int32), iterations=it_in.copy(), max_inliers=mx_in.copy(),
               terminate=np.zeros(F, np.int32), hyp_inliers=np.full((F, T), -1, np.int32), n=np.full((F, T), -1, np.int32),
               lo=np.full((F, T), -1, np.int32), hi=np.full((F, T), -1, np.int32), err=[None] * F, cap=np.zeros(F, np.int32),
               nmatches=np.zeros(F, np.int32))
    for p in (range(F) if pairs is None else pairs):
        g = Pair(b, p)
        out["nmatches"][p] = g.n
        if g.n < mn:
            out["terminate"][p] = 1
            continue
        cap = iteration_cap(g.n, prob, mn, T)
        out["cap"][p] = cap
        k0 = min(int(it_in[p]), cap)
        k1 = min(k0 + maxk, cap)
        if k1 > k0:
            jit = None if jitter_seed is None else np.random.default_rng([jitter_seed, p])
            S12, S21 = g.hypotheses(draws[p, k0:k1], fix_scale, rand_max, jit)
            e1, e2 = g.errors(S12, S21)
            inl, lo, hi = g.inliers(e1, e2, margin)
            out["err"][p] = (e1, e2)
            out["n"][p, k0:k1], out["lo"][p, k0:k1], out["hi"][p, k0:k1] = inl.sum(1), lo, hi
        ks, mx = walk(out["n"][p], k0, k1, int(mx_in[p]), mn if stop else 10 ** 9)
        out["max_inliers"][p] = mx
        if ks >= 0:
            out["found"][p] = 1
            out["iterations"][p] = ks + 1
            out["s12"][p] = S12[ks - k0]
            sl = g.k1 + g.slots[inl[ks - k0]]
            out["inlier"][sl] = 1
            out["match12"][sl] = g.m12[g.slots[inl[ks - k0]]]
            out["n_inliers"][p] = out["n"][p, ks]
            out["hyp_inliers"][p, k0:ks + 1] = out["n"][p, k0:ks + 1]
        else:
            out["iterations"][p] = k1
            out["terminate"][p] = int(k1 >= cap)
            out["hyp_inliers"][p, k0:k1] = out["n"][p, k0:k1]
    return out


def stop_is_decided(r, b, p):
    """The stop decision of pair p in the result r of iterate(b, margin) is the same for every count inside
    [lo, hi]: the success k* has lo > min_inliers and lo >= every earlier hi (and the incoming max_inliers); every
    earlier k has hi <= min_inliers or hi < some earlier lo (or the incoming max_inliers)."""
    mn = int(_param(b, "min_inliers", 20))
    mx = 0 if b.get("max_inliers") is None else int(b["max_inliers"][p])
    ev = np.nonzero(r["n"][p] >= 0)[0]
    if len(ev) == 0:
        return True
    k0 = ev[0]
    ks = int(r["iterations"][p]) - 1 if r["found"][p] == 1 else -1
    lo, hi = r["lo"][p], r["hi"][p]
    for k in (range(k0, ks) if ks >= 0 else ev):
        max_lo = max([mx] + [int(lo[j]) for j in range(k0, k)])
        if not (hi[k] <= mn or hi[k] < max_lo):
            return False
    if ks >= 0:
        max_hi = max([mx] + [int(hi[j]) for j in range(k0, ks)])
        return bool(lo[ks] > mn and lo[ks] >= max_hi)
    return True


def spread(a, b):
    """(rotation angle [rad], |dt| / |t|, |ds| / s) between two rows R, t, s."""
    Ra, Rb = np.asarray(a[:9], np.float64).reshape(3, 3), np.asarray(b[:9], np.float64).reshape(3, 3)
    dR = Ra @ Rb.T
    ang = math.atan2(np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2, (np.trace(dR) - 1) / 2)
    ta, tb = np.asarray(a[9:12], np.float64), np.asarray(b[9:12], np.float64)
    return np.array([abs(ang), np.linalg.norm(ta - tb) / np.linalg.norm(ta), abs(float(a[12]) - float(b[12])) / float(a[12])])
