"""Optimizer::PoseOptimization restated a second time, in sequential numpy fp64.  TEST INFRASTRUCTURE ONLY.

Written from the reference text, not from oracle/orb_oracle.cpp:
  src/Optimizer.cc:345-489                        the four rounds and the chi2 classification between them
  g2o/types/types_six_dof_expmap.{h,cpp}          EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose
  g2o/core/optimization_algorithm_levenberg.cpp   solve(), computeLambdaInit(), computeScale()
  g2o/core/sparse_optimizer.cpp                   optimize(): the iteration loop around solve()
  g2o/core/robust_kernel_impl.cpp                 RobustKernelHuber::robustify
  g2o/solvers/linear_solver_dense.h               LDL^T of H + lambda I, rejected unless positive
  g2o/types/se3quat.h                             exp, operator*, map, normalizeRotation (Eigen's quaternion)

Every per-edge quantity is a numpy array over the frame's edges (elementwise IEEE operations, spelled in the
reference's order); every sum over edges runs strictly in edge order (np.cumsum, never np.sum's pairwise
tree), as g2o walks its active edges.  That is also the oracle's order, so the two restatements are expected
to agree to the bit or an ulp; tests/test_pose_ref.py measures and bounds the difference.  It records the
trace that oracle_pose_optimization_trace records (tests/oracle_api.py PO_*_DTYPE).

One deliberate simplification, shared with the oracle: Eigen's LDLT pivots, this one does not.  The inertia
(what isPositive() reports) is the same and H + lambda I is positive definite whenever a step is accepted.
"""
import math

import numpy as np

from oracle_api import PO_END_REASONS, PO_FRAME_DTYPE, PO_ROUND_DTYPE, PO_TRIAL_DTYPE

CHI2_MONO, CHI2_STEREO = 5.991, 7.815   # Optimizer.cc:44-45
F = np.float64
DBL_MAX = np.finfo(np.float64).max


def seq_sum(a):
    """Sum over axis 0 strictly in order, as a loop `s += a[e]` would."""
    a = np.asarray(a, F)
    return np.cumsum(a, axis=0)[-1] if len(a) else np.zeros(a.shape[1:])


# --- Eigen's quaternion, as se3quat.h uses it (x, y, z, w) ---------------------------------------------------

def quaternion_from_matrix(R):
    """Eigen::Quaterniond(Matrix3d) (Shepperd).  Returns (q, branch): branch 0 for trace > 0, else 1 + i of the
    largest diagonal element."""
    R = np.asarray(R, F).reshape(3, 3)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + F(1.0))
        q[3] = F(0.5) * t
        t = F(0.5) / t
        q[0] = (R[2, 1] - R[1, 2]) * t
        q[1] = (R[0, 2] - R[2, 0]) * t
        q[2] = (R[1, 0] - R[0, 1]) * t
        return q, 0
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + F(1.0))
    q[i] = F(0.5) * t
    t = F(0.5) / t
    q[3] = (R[k, j] - R[j, k]) * t
    q[j] = (R[j, i] + R[i, j]) * t
    q[k] = (R[k, i] + R[i, k]) * t
    return q, 1 + i


def normalize_rotation(q):
    """SE3Quat::normalizeRotation: w made non-negative, then Quaternion::normalize (four divisions)."""
    if q[3] < 0:
        q = -q
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return q / n if n > 0 else q


def to_rotation_matrix(q):
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([1 - (tyy + tzz), txy - twz, txz + twy,
                     txy + twz, 1 - (txx + tzz), tyz - twx,
                     txz - twy, tyz + twx, 1 - (txx + tyy)])


def quaternion_product(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def rotate(q, v):
    """Quaternion * vector (Eigen's _transformVector: uv = 2 q.vec x v; v + w uv + q.vec x uv); v is [..., 3]."""
    x, y, z, w = q
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    u0, u1, u2 = y * v2 - z * v1, z * v0 - x * v2, x * v1 - y * v0
    u0, u1, u2 = u0 + u0, u1 + u1, u2 + u2
    c0, c1, c2 = y * u2 - z * u1, z * u0 - x * u2, x * u1 - y * u0
    return np.stack([v0 + w * u0 + c0, v1 + w * u1 + c1, v2 + w * u2 + c2], axis=-1)


def se3_map(pose, X):
    q, t = pose
    return rotate(q, X) + t


def se3_exp(update):
    """SE3Quat::exp (se3quat.h:223-257): update = (omega, upsilon)."""
    omega, upsilon = np.asarray(update[:3], F), np.asarray(update[3:], F)
    theta = np.sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    Om = np.array([[0, -omega[2], omega[1]], [omega[2], 0, -omega[0]], [-omega[1], omega[0], 0]], F)
    Om2 = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            s = F(0.0)
            for k in range(3):
                s = s + Om[i, k] * Om[k, j]
            Om2[i, j] = s
    I = np.eye(3)
    if theta < 0.00001:
        R = I + Om + Om2
        V = R
    else:
        s, c = F(math.sin(theta)), F(math.cos(theta))
        R = I + s / theta * Om + (1 - c) / (theta * theta) * Om2
        V = I + (1 - c) / (theta * theta) * Om + (theta - s) / F(math.pow(theta, 3)) * Om2
    q, _ = quaternion_from_matrix(R)
    t = np.array([V[i, 0] * upsilon[0] + V[i, 1] * upsilon[1] + V[i, 2] * upsilon[2] for i in range(3)])
    return normalize_rotation(q), t


def se3_mul(a, b):
    """SE3Quat::operator* (se3quat.h:104-110)."""
    (qa, ta), (qb, tb) = a, b
    return normalize_rotation(quaternion_product(qa, qb)), ta + rotate(qa, tb)


# --- the graph of one frame: one VertexSE3Expmap, unary edges ----------------------------------------------------

class Frame:
    def __init__(self, Xw, obs, info, cam):
        self.Xw, self.obs, self.info = (np.asarray(a, F) for a in (Xw, obs, info))
        self.fx, self.fy, self.cx, self.cy, self.bf = (F(c) for c in cam)
        self.E = len(self.info)
        self.stereo = ~(self.obs[:, 2] < 0)            # Optimizer.cc:378: ur < 0 is a monocular edge
        self.error = np.zeros((self.E, 3))             # each edge's _error as last computed
        self.robust = True
        self.th = np.where(self.stereo, CHI2_STEREO, CHI2_MONO)

    def compute_error(self, idx, pose):
        """computeError of the edges idx (types_six_dof_expmap.h:153-158, :184-189)."""
        Xc = se3_map(pose, self.Xw[idx])
        z, st = self.obs[idx], self.stereo[idx]
        x, y, d = Xc[:, 0], Xc[:, 1], Xc[:, 2]
        # mono: project2d, then * fx + cx (.cpp:290-296)
        em = np.stack([z[:, 0] - (x / d * self.fx + self.cx), z[:, 1] - (y / d * self.fy + self.cy),
                       np.zeros(len(d))], axis=1)
        # stereo: invz narrowed to float (.cpp:299-306)
        invz = (F(1.0) / d).astype(np.float32).astype(F)
        u = x * invz * self.fx + self.cx
        v = y * invz * self.fy + self.cy
        es = np.stack([z[:, 0] - u, z[:, 1] - v, z[:, 2] - (u - self.bf * invz)], axis=1)
        self.error[idx] = np.where(st[:, None], es, em)

    def chi2(self, idx):
        """BaseEdge::chi2 = error . (information * error), information = invSigma2 * I."""
        e, w = self.error[idx], self.info[idx]
        s = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
        return np.where(self.stereo[idx], s + e[:, 2] * (w * e[:, 2]), s)

    def robustify(self, idx, c):
        """RobustKernelHuber::robustify -> (rho, rho'), delta = sqrt(chi2 threshold) (Optimizer.cc:46-47)."""
        if not self.robust:
            return c, np.ones(len(c))
        delta = np.sqrt(self.th[idx])
        dsqr = delta * delta
        s = np.sqrt(c)
        inl = c <= dsqr
        return np.where(inl, c, 2 * s * delta - dsqr), np.where(inl, 1.0, delta / s)

    def active_robust_chi2(self, act):
        return seq_sum(self.robustify(act, self.chi2(act))[0]) if len(act) else F(0.0)

    def build_system(self, act, pose):
        """linearizeOplus (.cpp:266-288, :335-364) and BaseUnaryEdge::constructQuadraticForm of every active
        edge: H += J^T (rho' Omega) J, b -= rho' J^T Omega e, summed in edge order."""
        Xc = se3_map(pose, self.Xw[act])
        x, y = Xc[:, 0], Xc[:, 1]
        invz = F(1.0) / Xc[:, 2]
        invz_2 = invz * invz
        fx, fy, bf = self.fx, self.fy, self.bf
        zero = np.zeros(len(act))
        J0 = [x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, zero, x * invz_2 * fx]
        J1 = [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, zero, -invz * fy, y * invz_2 * fy]
        J2 = [J0[0] - bf * y * invz_2, J0[1] + bf * x * invz_2, J0[2], J0[3], zero, J0[5] - bf * invz_2]
        J = np.stack([np.stack(r, axis=1) for r in (J0, J1, J2)], axis=1)   # [n, 3, 6]
        st = self.stereo[act]
        info, err = self.info[act], self.error[act]
        _, r1 = self.robustify(act, self.chi2(act))
        w = r1 * info
        oe = info[:, None] * err
        s = J[:, 0, :] * oe[:, 0:1] + J[:, 1, :] * oe[:, 1:2]
        s = np.where(st[:, None], s + J[:, 2, :] * oe[:, 2:3], s)
        b = seq_sum(-(r1[:, None] * s))
        term = lambda r: (J[:, r, :, None] * w[:, None, None]) * J[:, r, None, :]
        h = term(0) + term(1)
        h = np.where(st[:, None, None], h + term(2), h)
        return seq_sum(h), b


def linear_solver_dense(H, b, lam):
    """LinearSolverDense::solve of (H + lambda I) x = b (linear_solver_dense.h:65-113): LDL^T, false unless
    every pivot is finite and >= 0; zero pivots give zero components.  Returns (ok, x); x is None when not ok."""
    A = np.array(H, F)
    for i in range(6):
        A[i, i] = A[i, i] + lam
    L, D = np.eye(6), np.zeros(6)
    for j in range(6):
        v = A[j, j]
        for k in range(j):
            v = v - L[j, k] * L[j, k] * D[k]
        if not (v >= 0) or not np.isfinite(v):
            return False, None
        D[j] = v
        for i in range(j + 1, 6):
            s = A[i, j]
            for k in range(j):
                s = s - L[i, k] * L[j, k] * D[k]
            L[i, j] = s / v if v != 0 else F(0.0)
    y = np.zeros(6)
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i, k] * y[k]
        y[i] = s
    for i in range(6):
        y[i] = y[i] / D[i] if D[i] != 0 else F(0.0)
    x = np.zeros(6)
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k, i] * x[k]
        x[i] = s
    return True, x


def _optimize(fr, act, pose, iterations, max_trials, rec, where):
    """SparseOptimizer::optimize(iterations) around OptimizationAlgorithmLevenberg::solve.  Returns
    (pose, iterations done, end reason); appends one dict per trial to rec."""
    if len(act) == 0:   # "0 vertices to optimize, maybe forgot to call initializeOptimization()"
        return pose, 0, "none"
    lam = ni = F(0.0)
    nbad = done = 0
    reason = "budget"
    for it in range(iterations):
        fr.compute_error(act, pose)
        cur = fr.active_robust_chi2(act)
        ini = cur
        H, b = fr.build_system(act, pose)
        if it == 0:   # computeLambdaInit: tau * max |H_jj| by std::max(fabs(h), maxDiagonal), which returns its
            m = F(0.0)   # first argument unless that is smaller: a NaN diagonal element becomes the maximum
            for j in range(6):
                d = np.abs(H[j, j])
                m = m if d < m else d
            lam, ni, nbad = F(1e-5) * m, F(2.0), 0
        rho, q = F(0.0), 0
        while True:
            t = dict(where, it=it, q=q, cur=cur)
            t["lambda"] = lam
            saved = pose
            ok, x = linear_solver_dense(H, b, lam)
            if not ok:
                x = np.zeros(6)
            pose = se3_mul(se3_exp(x), pose)   # VertexSE3Expmap::oplusImpl
            fr.compute_error(act, pose)
            tmp = fr.active_robust_chi2(act)
            if not ok:
                tmp = DBL_MAX
            rho = cur - tmp
            scale = seq_sum(x * (lam * x + b)) + F(1e-3)   # computeScale(), "make sure it's non-zero :)"
            rho = rho / scale
            good = bool(rho > 0 and np.isfinite(tmp))
            t.update(ok=int(ok), tmp=tmp, scale=scale, rho=rho, accepted=int(good))
            rec.append(t)
            if good:
                alpha = F(1.0) - F(math.pow(2 * rho - 1, 3))
                alpha = min(alpha, F(2.0) / 3)
                lam = lam * max(F(1.0) / 3, alpha)
                ni = F(2.0)
                cur = tmp
            else:
                lam = lam * ni
                ni = ni * 2
                pose = saved
            q += 1
            if not (rho < 0 and q < max_trials):
                break
        done += 1
        t.update(iter_end=1, ini=ini, cur_end=cur, nbad=nbad)
        if q == max_trials or rho == 0:
            reason = "q10" if q == max_trials else "rho0"
            break
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        t.update(nbad_tested=1, nbad=nbad)
        if nbad >= 3:
            reason = "nbad"
            break
    return pose, done, reason


def pose_optimization(batch, max_iters=10, max_trials=10):
    """Optimizer::PoseOptimization per frame of a batch dict (the layout of synth.make_pose_batch).  Returns
    pose_R, pose_t, n_inliers, outlier and the trace records trials / rounds / frames."""
    eb = np.asarray(batch["edge_begin"])
    n, Etot = len(eb) - 1, int(eb[-1])
    out = dict(pose_R=np.zeros((n, 9)), pose_t=np.zeros((n, 3)), n_inliers=np.zeros(n, np.int32),
               outlier=np.zeros(Etot, np.uint8))
    trials, rounds, frames = [], [], []
    with np.errstate(all="ignore"):
        for f in range(n):
            e0, e1 = int(eb[f]), int(eb[f + 1])
            R0, t0 = np.asarray(batch["pose_R"][f], F), np.asarray(batch["pose_t"][f], F)
            if e1 - e0 < 3:   # Optimizer.cc:413-415
                out["pose_R"][f], out["pose_t"][f] = R0, t0
                continue
            fr = Frame(batch["xw"][e0:e1], batch["obs"][e0:e1], batch["inv_sigma2"][e0:e1], batch["cam"][f])
            q0, branch = quaternion_from_matrix(R0)   # ToSE3Quat -> SE3Quat(R, t)
            frames.append((f, branch, int(q0[3] < 0)))
            init = (normalize_rotation(q0), t0.copy())
            outlier = np.zeros(fr.E, bool)
            pose = init
            for k in range(4):
                act = np.flatnonzero(~outlier)   # initializeOptimization(0): the level-0 edges
                pose, done, reason = _optimize(fr, act, init, max_iters, max_trials, trials, dict(frame=f, round=k))
                was = np.flatnonzero(outlier)
                fr.compute_error(was, pose)      # an outlier was not active: its error is recomputed
                chi = fr.chi2(np.arange(fr.E))
                new = chi > fr.th
                margin = np.abs(chi - fr.th) / fr.th
                margin = margin[~np.isnan(margin)]
                rounds.append((f, k, len(act), done, PO_END_REASONS.index(reason), int(new.sum()),
                               int((outlier & ~new).sum()), 0, margin.min() if len(margin) else np.inf))
                outlier = new
                if k == 2:
                    fr.robust = False
                if fr.E < 10:
                    break
            out["pose_R"][f], out["pose_t"][f] = to_rotation_matrix(pose[0]), pose[1]
            out["n_inliers"][f] = fr.E - int(outlier.sum())
            out["outlier"][e0:e1] = outlier
    tr = np.zeros(len(trials), PO_TRIAL_DTYPE)
    for i, t in enumerate(trials):
        for key, val in t.items():
            tr[i][key] = val
    out["trials"] = tr
    out["rounds"] = np.array(rounds, PO_ROUND_DTYPE) if rounds else np.zeros(0, PO_ROUND_DTYPE)
    out["frames"] = np.array(frames, PO_FRAME_DTYPE) if frames else np.zeros(0, PO_FRAME_DTYPE)
    return out
