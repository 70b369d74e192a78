"""Optimizer::BundleAdjustment and the GlobalBA thread's map update restated in numpy (test infrastructure).

bundle_adjustment(): g2o's Levenberg-Marquardt over BlockSolver_6_3 in fp64:
  errors          EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ::computeError (types_six_dof_expmap.h:90-127), the stereo
                  edge's invz and bf * invz narrowed to float (types_six_dof_expmap.cpp:148-156)
  robust kernel   Huber, delta = sqrt(5.991) mono / sqrt(7.815) stereo (Optimizer.cc:44-47, robust_kernel_impl.cpp:78-91)
  Jacobians       linearizeOplus (types_six_dof_expmap.cpp:103-139, :188-234), quadratic form base_binary_edge.hpp:54-120
  solver          Schur complement on the points (block_solver.hpp:377-419), dense solve of the reduced system
  LM              optimization_algorithm_levenberg.cpp:61-189: lambda0 = 1e-5 max |diag H|, rho, lambda / nu, ten trials;
                  sparse_optimizer.cpp:376-420: the nBad rule; SE3Quat::exp update (se3quat.h:217-257)
It takes a schedule (a list of optimize() iteration counts, with LocalBA's classification between two of them), the
robust flag and the stereo rule, and records every trial's accept flag.  `jitter_seed`: every error component is moved
by -1, 0 or +1 ulp, drawn per evaluation; the spread of the outputs under it is the restatement's own uncertainty.

update_map(): LoopClosing.cc:392-446 in np.float32, one rounding per operation, walked with the reference's queue."""
import math

import numpy as np

F32 = np.float32
RULE_REFERENCE, RULE_LOCAL = 0, 1
DBL_MAX = 1.7976931348623157e308
CHI2_MONO, CHI2_STEREO = 5.991, 7.815


# ---------------------------------------------------------------- SE3Quat (Eigen's quaternion formulas)
def q_from_R(m):
    m = [float(v) for v in np.asarray(m).reshape(9)]
    t = m[0] + m[4] + m[8]
    if t > 0:
        s = math.sqrt(t + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        return [(m[7] - m[5]) * s, (m[2] - m[6]) * s, (m[3] - m[1]) * s, w]
    i = (2 if m[8] > m[4] else 1) if m[4] > m[0] else (2 if m[8] > m[0] else 0)
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0)
    q = [0.0] * 4
    q[i] = 0.5 * s
    s = 0.5 / s
    q[3] = (m[3 * k + j] - m[3 * j + k]) * s
    q[j] = (m[3 * j + i] + m[3 * i + j]) * s
    q[k] = (m[3 * k + i] + m[3 * i + k]) * s
    return q


def q_normalized(q):
    if q[3] < 0:
        q = [-v for v in q]
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [v / n for v in q] if n > 0 else q


def q_to_R(q):
    """toRotationMatrix; q [..., 4] -> [..., 9]."""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
                     1 - (txx + tyy)], axis=-1)


def q_rotate(q, v):
    """Eigen's q * v; q [..., 4], v [..., 3]."""
    qx, qy, qz, qw = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    uv = [qy * v[..., 2] - qz * v[..., 1], qz * v[..., 0] - qx * v[..., 2], qx * v[..., 1] - qy * v[..., 0]]
    uv = [u + u for u in uv]
    c = [qy * uv[2] - qz * uv[1], qz * uv[0] - qx * uv[2], qx * uv[1] - qy * uv[0]]
    return np.stack([v[..., i] + qw * uv[i] + c[i] for i in range(3)], axis=-1)


def se3_exp_update(upd, q, t):
    """pose <- SE3Quat::exp(upd) * pose (se3quat.h:217-257, :99-105)."""
    w = np.asarray(upd[:3], np.float64)
    theta = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    O2 = O @ O
    I = np.eye(3)
    if theta < 0.00001:
        R = I + O + O2
        V = R
    else:
        s, c = math.sin(theta), math.cos(theta)
        R = I + s / theta * O + (1 - c) / (theta * theta) * O2
        V = I + (1 - c) / (theta * theta) * O + (theta - s) / (theta * theta * theta) * O2
    E = np.array(q_normalized(q_from_R(R.reshape(9))))
    tn = V @ np.asarray(upd[3:6]) + q_rotate(E, np.asarray(t, np.float64))
    ax, ay, az, aw = E
    bx, by, bz, bw = q
    r = [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
         aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz]
    return np.array(q_normalized(r)), tn


# ---------------------------------------------------------------- the problem
def edge_types(obs, stereo_rule):
    """1 = stereo edge.  RULE_LOCAL: ur < 0 => mono (Optimizer.cc:595); RULE_REFERENCE: `if (ur)` (:253)."""
    ur = np.asarray(obs, np.float64).reshape(-1, 3)[:, 2]
    return (~(ur < 0) if stereo_rule == RULE_LOCAL else ~(ur != 0)).astype(np.uint8)


class Problem:
    def __init__(self, pr, stereo_rule, robust, jitter_seed=None):
        f = lambda k, n: np.array(pr[k], np.float64).reshape(-1, n)   # noqa: E731
        self.R0, self.t = f("pose_R", 9), f("pose_t", 3).copy()
        self.P = len(self.R0)
        self.q = np.array([q_normalized(q_from_R(r)) for r in self.R0]).reshape(-1, 4)
        self.fixed = np.array(pr["pose_fixed"], bool).reshape(-1)
        self.X = f("points", 3).copy()
        self.N = len(self.X)
        self.ep = np.array(pr["edge_point"], np.int64).reshape(-1)
        self.ek = np.array(pr["edge_pose"], np.int64).reshape(-1)
        self.E = len(self.ep)
        self.obs, self.info, self.cam = f("edge_obs", 3), f("edge_inv_sigma2", 1)[:, 0], f("edge_cam", 5)
        self.stereo = edge_types(self.obs, stereo_rule).astype(bool)
        self.robust = np.full(self.E, bool(robust))
        self.level = np.zeros(self.E, bool)
        self.rng = None if jitter_seed is None else np.random.default_rng(jitter_seed)
        self.err = np.zeros((self.E, 3))
        self.accept = []
        self.trials = 0

    # -- errors of the edges in `act` (indices) at the current estimates
    def errors(self, act):
        Xc = q_rotate(self.q[self.ek[act]], self.X[self.ep[act]]) + self.t[self.ek[act]]
        c, z, st = self.cam[act], self.obs[act], self.stereo[act]
        e = np.zeros((len(act), 3))
        with np.errstate(all="ignore"):
            e[:, 0] = z[:, 0] - (Xc[:, 0] / Xc[:, 2] * c[:, 0] + c[:, 2])
            e[:, 1] = z[:, 1] - (Xc[:, 1] / Xc[:, 2] * c[:, 1] + c[:, 3])
            invz = (1.0 / Xc[:, 2]).astype(F32)   # const float invz = 1.0f / z: a double division, narrowed
            u = Xc[:, 0] * invz.astype(np.float64) * c[:, 0] + c[:, 2]
            v = Xc[:, 1] * invz.astype(np.float64) * c[:, 1] + c[:, 3]
            bfz = (c[:, 4].astype(F32) * invz).astype(np.float64)
            es = np.stack([z[:, 0] - u, z[:, 1] - v, z[:, 2] - (u - bfz)], axis=1)
        e[st] = es[st]
        if self.rng is not None and len(act):
            e = e * (1.0 + self.rng.integers(-1, 2, size=e.shape).astype(np.float64) * 2.0 ** -52)
        return e, Xc

    def chi2(self, e, act):
        c = e[:, 0] * self.info[act] * e[:, 0] + e[:, 1] * self.info[act] * e[:, 1]
        return np.where(self.stereo[act], c + e[:, 2] * self.info[act] * e[:, 2], c)

    def robustify(self, chi, act):
        """(rho, rho') of the edges' robust kernels."""
        delta = np.where(self.stereo[act], math.sqrt(CHI2_STEREO), math.sqrt(CHI2_MONO))
        dsqr = delta * delta
        with np.errstate(all="ignore"):
            s = np.sqrt(chi)
            out = self.robust[act] & (chi > dsqr)
            r0 = np.where(out, 2 * s * delta - dsqr, chi)
            r1 = np.where(out, delta / s, 1.0)
        return r0, r1

    def active_chi2(self, act):
        e, _ = self.errors(act)
        self.err[act] = e
        r0, _ = self.robustify(self.chi2(e, act), act)
        return float(np.sum(r0))

    # -- one optimize(iters) over the level-0 edges
    def optimize(self, iters):
        act = np.flatnonzero(~self.level)
        if iters <= 0 or len(act) == 0:
            return 0, 0.0
        ek, ep = self.ek[act], self.ep[act]
        pose_used = np.zeros(self.P, bool)
        pose_used[ek] = True
        free = np.flatnonzero(pose_used & ~self.fixed)
        hp = np.full(self.P, -1)
        hp[free] = np.arange(len(free))
        pts = np.unique(ep)
        hl = np.full(self.N, -1)
        hl[pts] = np.arange(len(pts))
        n_p, n_l = len(free), len(pts)
        if n_p + n_l == 0:
            return 0, 0.0
        ip, il = hp[ek], hl[ep]
        fe = ip >= 0   # edges to a free pose
        lam, ni, nbad, done, cur = 0.0, 2.0, 0, 0, 0.0
        for it in range(iters):
            done += 1
            e, Xc = self.errors(act)
            self.err[act] = e
            chi = self.chi2(e, act)
            r0, r1 = self.robustify(chi, act)
            cur = ini = float(np.sum(r0))
            A, B = self.jacobians(act, Xc)
            d_mask = np.stack([np.ones(len(act), bool)] * 2 + [self.stereo[act]], axis=1)
            om_r = np.where(d_mask, -self.info[act, None] * e * r1[:, None], 0.0)
            w = r1 * self.info[act]
            Hll, bl = np.zeros((n_l, 3, 3)), np.zeros((n_l, 3))
            np.add.at(Hll, il, np.einsum("eri,e,erj->eij", A, w, A))
            np.add.at(bl, il, np.einsum("eri,er->ei", A, om_r))
            Hpp, bp = np.zeros((n_p, 6, 6)), np.zeros((n_p, 6))
            np.add.at(Hpp, ip[fe], np.einsum("eri,e,erj->eij", B[fe], w[fe], B[fe]))
            np.add.at(bp, ip[fe], np.einsum("eri,er->ei", B[fe], om_r[fe]))
            Hpl = np.einsum("eri,e,erj->eij", B, w, A)   # [Ea, 6, 3]
            if it == 0:   # computeLambdaInit
                diag = [np.abs(np.einsum("nii->ni", Hll)).max(initial=0.0), np.abs(np.einsum("nii->ni", Hpp)).max(initial=0.0)]
                lam, ni, nbad = 1e-5 * max(diag), 2.0, 0
            rho, qn = 0.0, 0
            while True:
                sv = (self.q.copy(), self.t.copy(), self.X.copy())
                ok, xp, xl = self.solve(lam, Hll, bl, Hpp, bp, Hpl, ip, il, fe, n_p)
                for k, i in enumerate(free):
                    self.q[i], self.t[i] = se3_exp_update(xp[k], self.q[i], self.t[i])
                self.X[pts] += xl
                with np.errstate(all="ignore"):
                    tmp = self.active_chi2(act)
                if not ok:
                    tmp = DBL_MAX
                scale = float(np.sum(xl * (lam * xl + bl)) + np.sum(xp * (lam * xp + bp)))
                rho = (cur - tmp) / (scale + 1e-3)
                acc = rho > 0 and math.isfinite(tmp)
                self.accept.append(bool(acc))
                self.trials += 1
                if acc:
                    alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni = 2.0
                    cur = tmp
                else:
                    lam *= ni
                    ni *= 2
                    self.q, self.t, self.X = sv
                qn += 1
                if not (rho < 0 and qn < 10):
                    break
            if qn == 10 or rho == 0:
                break
            nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
            if nbad >= 3:
                break
        return done, cur

    def jacobians(self, act, Xc):
        """(A [Ea, 3, 3] = d error / d point, B [Ea, 3, 6] = d error / d pose); row 2 zero for a mono edge."""
        R = q_to_R(self.q[self.ek[act]]).reshape(-1, 3, 3)
        x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
        c, st = self.cam[act], self.stereo[act]
        fx, fy, bf = c[:, 0], c[:, 1], c[:, 4]
        n = len(act)
        with np.errstate(all="ignore"):
            z2 = z * z
            tmp = np.zeros((n, 2, 3))
            tmp[:, 0, 0], tmp[:, 0, 2] = fx, -x / z * fx
            tmp[:, 1, 1], tmp[:, 1, 2] = fy, -y / z * fy
            A = np.zeros((n, 3, 3))
            A[:, :2] = -1. / z[:, None, None] * np.einsum("erm,emj->erj", tmp, R)
            As = np.zeros((n, 3, 3))
            for j in range(3):
                As[:, 0, j] = -fx * R[:, 0, j] / z + fx * x * R[:, 2, j] / z2
                As[:, 1, j] = -fy * R[:, 1, j] / z + fy * y * R[:, 2, j] / z2
                As[:, 2, j] = As[:, 0, j] - bf * R[:, 2, j] / z2
            A[st] = As[st]
            B = np.zeros((n, 3, 6))
            B[:, 0, 0], B[:, 0, 1], B[:, 0, 2] = x * y / z2 * fx, -(1 + (x * x / z2)) * fx, y / z * fx
            B[:, 0, 3], B[:, 0, 5] = -1. / z * fx, x / z2 * fx
            B[:, 1, 0], B[:, 1, 1], B[:, 1, 2] = (1 + y * y / z2) * fy, -x * y / z2 * fy, -x / z * fy
            B[:, 1, 4], B[:, 1, 5] = -1. / z * fy, y / z2 * fy
            B2 = np.stack([B[:, 0, 0] - bf * y / z2, B[:, 0, 1] + bf * x / z2, B[:, 0, 2], B[:, 0, 3], np.zeros(n),
                           B[:, 0, 5] - bf / z2], axis=1)
            B[st, 2] = B2[st]
        return A, B

    @staticmethod
    def solve(lam, Hll, bl, Hpp, bp, Hpl, ip, il, fe, n_p):
        """BlockSolver::solve: (ok, x_poses [np, 6], x_points [nl, 3])."""
        n_l = len(Hll)
        with np.errstate(all="ignore"):
            D = Hll + lam * np.eye(3)
            det = np.linalg.det(D) if n_l else np.zeros(0)
            good = det != 0
            Dinv = np.zeros_like(D)
            if good.any():
                Dinv[good] = np.linalg.inv(D[good])
            xp = np.zeros((n_p, 6))
            ok = True
            if n_p:
                S = np.zeros((n_p, n_p, 6, 6))
                S[np.arange(n_p), np.arange(n_p)] = Hpp + lam * np.eye(6)
                bs = bp.copy()
                W = np.einsum("eij,ejk->eik", Hpl[fe], Dinv[il[fe]])   # [Ef, 6, 3]
                np.subtract.at(bs, ip[fe], np.einsum("eik,ek->ei", W, bl[il[fe]]))
                # S(i1, i2) -= sum over the point's edge pairs W(e1) Hpl(e2)^T
                order = np.argsort(il[fe], kind="stable")
                fi, fl = ip[fe][order], il[fe][order]
                Wo, Ho = W[order], Hpl[fe][order]
                beg = np.searchsorted(fl, np.arange(n_l))
                end = np.searchsorted(fl, np.arange(n_l), side="right")
                for a, b in zip(beg, end):
                    if b > a:
                        blk = np.einsum("aik,bjk->abij", Wo[a:b], Ho[a:b])
                        np.subtract.at(S, (fi[a:b, None], fi[None, a:b]), blk)
                Sd = S.transpose(0, 2, 1, 3).reshape(6 * n_p, 6 * n_p)
                try:
                    L = np.linalg.cholesky(Sd)
                    y = np.linalg.solve(L, bs.reshape(-1))
                    xp = np.linalg.solve(L.T, y).reshape(n_p, 6)
                    ok = bool(np.isfinite(xp).all())
                except np.linalg.LinAlgError:
                    ok = False
                if not ok:
                    xp = np.zeros((n_p, 6))
            cl = bl.copy()
            if n_p:
                np.subtract.at(cl, il[fe], np.einsum("eij,ei->ej", Hpl[fe], xp[ip[fe]]))
            xl = np.einsum("nij,nj->ni", Dinv, cl)
        return ok, xp, xl


def bundle_adjustment(pr, n_iterations=5, robust=True, stereo_rule=RULE_REFERENCE, jitter_seed=None, schedule=None):
    """dict(pose_q, pose_R, pose_t, points, pose_f, points_f, point_included, edge_chi2, iterations, trials, chi2,
    accept).  schedule (default [n_iterations]): the optimize() calls; between two of them LocalBA's classification
    (Optimizer.cc:644-670: outliers to level 1, robust kernels off)."""
    G = Problem(pr, stereo_rule, robust, jitter_seed)
    its, chi = [], []
    for k, n in enumerate(schedule or [n_iterations]):
        if k:
            e = G.err
            c = G.chi2(e, np.arange(G.E))
            Xc = q_rotate(G.q[G.ek], G.X[G.ep]) + G.t[G.ek]
            G.level |= (c > np.where(G.stereo, CHI2_STEREO, CHI2_MONO)) | ~(Xc[:, 2] > 0)
            G.robust[:] = False
        i, c = G.optimize(n)
        its.append(i)
        chi.append(c)
    inc = np.zeros(G.N, np.uint8)
    inc[G.ep] = 1
    R = q_to_R(G.q)
    return dict(pose_q=G.q, pose_R=R, pose_t=G.t, points=G.X, pose_f=np.hstack([R, G.t]).astype(F32), points_f=G.X.astype(F32),
                point_included=inc, edge_chi2=G.chi2(G.err, np.arange(G.E)), iterations=its[0] if len(its) == 1 else tuple(its),
                trials=G.trials, chi2=chi[0] if len(chi) == 1 else tuple(chi), accept=np.array(G.accept, bool))


def jitter_spread(pr, draws=4, **kw):
    """(pose rmse: the larger of pose_t's and pose_q's, point rmse) spread of the restatement over `draws` one-ulp jitter draws, the unjittered run
    included, and whether every draw took the same accept sequence."""
    runs = [bundle_adjustment(pr, **kw)] + [bundle_adjustment(pr, jitter_seed=s, **kw) for s in range(draws)]
    same = all(np.array_equal(r["accept"], runs[0]["accept"]) and r["iterations"] == runs[0]["iterations"] for r in runs)
    dp = max(max(rmse(a["pose_t"], b["pose_t"]), rmse(a["pose_q"], b["pose_q"])) for a in runs for b in runs)
    dx = max(rmse(a["points"], b["points"]) for a in runs for b in runs)
    return dp, dx, same


def rmse(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


# ---------------------------------------------------------------- the map update, float, one rounding per operation
def f_matvec(R, v):
    """cv::Matx33f * Matx31f: s = 0, then the k = 0, 1, 2 terms in order."""
    out = []
    for i in range(3):
        s = F32(0)
        for k in range(3):
            s = F32(s + F32(R[3 * i + k] * v[k]))
        out.append(s)
    return out


def f_inverse(T):
    """CameraPose::Inverse (CameraPose.h:44-48): (R^T, (-R^T) * t)."""
    T = [F32(v) for v in T]
    Rt = [T[3 * j + i] for i in range(3) for j in range(3)]
    return Rt + f_matvec([F32(-v) for v in Rt], T[9:12])


def f_mul(A, B):
    """CameraPose::operator* (CameraPose.h:50-56): t = R1 * t2 + t1, R = R1 * R2."""
    A, B = [F32(v) for v in A], [F32(v) for v in B]
    t = [F32(a + b) for a, b in zip(f_matvec(A, B[9:12]), A[9:12])]
    R = []
    for i in range(3):
        for j in range(3):
            s = F32(0)
            for k in range(3):
                s = F32(s + F32(A[3 * i + k] * B[3 * k + j]))
            R.append(s)
    return R + t


def f_move_point(bef, pose_new, X):
    """LoopClosing.cc:435-444."""
    bef, X = [F32(v) for v in bef], [F32(v) for v in X]
    Xc = [F32(a + b) for a, b in zip(f_matvec(bef, X), bef[9:12])]
    Twc = f_inverse(pose_new)
    return [F32(a + b) for a, b in zip(f_matvec(Twc, Xc), Twc[9:12])]


def update_map(m):
    """LoopClosing.cc:392-446 on the orbba_gba_map tables (a dict); returns the five updated arrays."""
    with np.errstate(all="ignore"):
        K, M = len(m["kf_in_gba"]), len(m["mp_bad"])
        flag = np.array(m["kf_in_gba"], np.uint8).reshape(K).copy()
        pose = np.array(m["kf_pose"], F32).reshape(K, 12).copy()
        gba = np.array(m["kf_pose_gba"], F32).reshape(K, 12).copy()
        bef = np.array(m["kf_pose_bef"], F32).reshape(K, 12).copy()
        xw = np.array(m["mp_xw"], F32).reshape(M, 3).copy()
        off, idx = np.asarray(m["kf_child_off"]).reshape(-1), np.asarray(m["kf_child_idx"]).reshape(-1)
        queue = [int(o) for o in np.asarray(m["origins"]).reshape(-1)]
        while queue:
            kf = queue[0]
            Twc = f_inverse(pose[kf])
            for c in idx[off[kf]:off[kf + 1]]:
                c = int(c)
                if not flag[c]:
                    gba[c] = f_mul(f_mul(pose[c], Twc), gba[kf])
                    flag[c] = 1
                queue.append(c)
            bef[kf] = pose[kf]
            pose[kf] = gba[kf]
            queue.pop(0)
        for p in range(M):
            if m["mp_bad"][p]:
                continue
            if m["mp_in_gba"][p]:
                xw[p] = np.asarray(m["mp_pos_gba"], F32).reshape(M, 3)[p]
                continue
            r = int(m["mp_ref_kf"][p])
            if not flag[r]:
                continue
            xw[p] = f_move_point(bef[r], pose[r], xw[p])
    return dict(kf_in_gba=flag, kf_pose=pose, kf_pose_gba=gba, kf_pose_bef=bef, mp_xw=xw)
