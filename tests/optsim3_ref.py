"""Per-pair fp64 restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:944-1100) on the orbba_sim3_batch
arrays, written from the reference's g2o:

  types/sim3.h:59-67 (constructors), :70-142 (Sim3(Vector7d)), :144-146 (map), :233-236 (inverse),
  :266-272 (operator*); types/types_seven_dof_expmap.h:60-88 (oplusImpl, cam_map1 / cam_map2), :138-145 and
  :160-167 (the two computeError; linearizeOplus is commented out at :147 / :169);
  core/base_binary_edge.hpp:143-200 (the numeric Jacobian, delta = 1e-9), :54-120 (constructQuadraticForm);
  core/robust_kernel_impl.cpp:65-91 (Huber); core/optimization_algorithm_levenberg.cpp:61-189;
  core/sparse_optimizer.cpp:354-419 (optimize); solvers/linear_solver_dense.h:65-115.

Every step is an IEEE double operation in the reference's evaluation order (Python floats for the estimate,
numpy's elementwise +, -, *, / and sqrt over the correspondences for the edges, which round one edge at a time
exactly as the scalar operations do; sums over edges run one addition at a time in insertion order); the camera-frame
points are np.float32 in the cv::Matx order and then widened (Optimizer.cc:1006-1012).  The dense LDL^T is
unpivoted, as the project restates Eigen::LDLT everywhere (oracle/orb_oracle.cpp, PoseOpt); H + lambda I is
positive definite whenever it is accepted.  Imports nothing from the package.

`jitter_seed`: every error evaluation is multiplied by 1 + k 2^-52, k in {-1, 0, 1} drawn from the seed, which
shows how far the reference's own result moves under the rounding that delta = 1e-9 magnifies."""
import math

import numpy as np

F32 = np.float32
EPS = 0.00001
DELTA = 1e-9
DBL_MAX = float(np.finfo(np.float64).max)


# ---------------------------------------------------------------- Eigen::Quaterniond pieces
def q_from_R(m):
    """Eigen::Quaterniond(Matrix3d), m row-major 9; returns (x, y, z, w), not normalised."""
    t = m[0] + m[4] + m[8]
    if t > 0:
        s = math.sqrt(t + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        return [(m[7] - m[5]) * s, (m[2] - m[6]) * s, (m[3] - m[1]) * s, w]
    i = (2 if m[8] > m[4] else 1) if m[4] > m[0] else (2 if m[8] > m[0] else 0)
    j, k = (i + 1) % 3, (i + 2) % 3
    M = lambda r, c: m[3 * r + c]   # noqa: E731
    s = math.sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0)
    q = [0.0] * 4
    q[i] = 0.5 * s
    s = 0.5 / s
    q[3] = (M(k, j) - M(j, k)) * s
    q[j] = (M(j, i) + M(i, j)) * s
    q[k] = (M(k, i) + M(i, k)) * s
    return q


def q_to_R(q):
    """toRotationMatrix(), row-major 9."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
            1 - (txx + tyy)]


def q_rotate(q, v):
    """Quaternion * vector (_transformVector): uv = 2 (vec x v); v + w uv + vec x uv."""
    qx, qy, qz, qw = q
    uv = [qy * v[2] - qz * v[1], qz * v[0] - qx * v[2], qx * v[1] - qy * v[0]]
    uv = [u + u for u in uv]
    c = [qy * uv[2] - qz * uv[1], qz * uv[0] - qx * uv[2], qx * uv[1] - qy * uv[0]]
    return [v[i] + qw * uv[i] + c[i] for i in range(3)]


def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz]


# ---------------------------------------------------------------- g2o::Sim3 as (q, t, s)
def sim3_exp(u):
    """Sim3(const Vector7d& update), sim3.h:70-142."""
    w0, w1, w2 = u[0], u[1], u[2]
    ups = u[3:6]
    sigma = u[6]
    theta = math.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
    O = [0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0]
    O2 = [(O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j]) + O[3 * i + 2] * O[6 + j] for i in range(3) for j in range(3)]
    I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    s = math.exp(sigma)
    if abs(sigma) < EPS:
        C = 1.0
        if theta < EPS:
            A, B = 1. / 2., 1. / 6.
            R = [(I[i] + O[i]) + O2[i] for i in range(9)]
        else:
            theta2 = theta * theta
            A = (1 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
            ra, rb = math.sin(theta) / theta, (1 - math.cos(theta)) / (theta * theta)
            R = [(I[i] + ra * O[i]) + rb * O2[i] for i in range(9)]
    else:
        C = (s - 1) / sigma
        if theta < EPS:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            R = [(I[i] + O[i]) + O2[i] for i in range(9)]
        else:
            ra, rb = math.sin(theta) / theta, (1 - math.cos(theta)) / (theta * theta)
            R = [(I[i] + ra * O[i]) + rb * O2[i] for i in range(9)]
            a = s * math.sin(theta)
            b = s * math.cos(theta)
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    W = [(A * O[i] + B * O2[i]) + C * I[i] for i in range(9)]
    t = [(W[3 * i] * ups[0] + W[3 * i + 1] * ups[1]) + W[3 * i + 2] * ups[2] for i in range(3)]
    return (q_from_R(R), t, s)


def sim3_mul(a, b):
    """operator*, sim3.h:266-272."""
    rt = q_rotate(a[0], b[1])
    return (q_mul(a[0], b[0]), [a[2] * rt[i] + a[1][i] for i in range(3)], a[2] * b[2])


def sim3_inverse(a):
    """inverse(), sim3.h:233-236."""
    qc = [-a[0][0], -a[0][1], -a[0][2], a[0][3]]
    m = -1. / a[2]
    return (qc, q_rotate(qc, [m * a[1][0], m * a[1][1], m * a[1][2]]), 1. / a[2])


def sim3_map(a, x):
    r = q_rotate(a[0], x)
    return [a[2] * r[i] + a[1][i] for i in range(3)]


def sim3_matrix(a):
    """The 4x4 [[s R, t], [0, 1]] (for the tests' matrix algebra)."""
    M = np.eye(4)
    M[:3, :3] = a[2] * np.array(q_to_R(a[0])).reshape(3, 3)
    M[:3, 3] = a[1]
    return M


def to_g2o(row):
    """ToG2OSim3 (Optimizer.cc:183-188) of the 13 floats R, t, s."""
    row = [float(F32(v)) for v in row]
    return (q_from_R(row[:9]), row[9:12], row[12])


def from_g2o(S):
    """FromG2OSim3 (Optimizer.cc:190-195): the 13 floats."""
    return np.array(q_to_R(S[0]) + list(S[1]) + [S[2]], np.float64).astype(np.float32)


def g2o_row(S):
    return np.array(list(S[0]) + list(S[1]) + [S[2]], np.float64)


# ---------------------------------------------------------------- the edges
def world_to_camera(P, X):
    """R * Xw + t in float, cv::Matx order (the helper tests/sim3_ref.py restates for SearchBySim3)."""
    P = [F32(v) for v in P]
    X = [F32(v) for v in X]
    return [float(((P[3 * i] * X[0] + P[3 * i + 1] * X[1]) + P[3 * i + 2] * X[2]) + P[9 + i]) for i in range(3)]


class _Jitter:
    def __init__(self, seed):
        self.rng = None if seed is None else np.random.default_rng(seed)

    def __call__(self, e):
        if self.rng is None:
            return e
        k = self.rng.integers(-1, 2, size=(2, len(e[0]))).astype(np.float64)
        return [e[0] * (1.0 + k[0] * 2.0 ** -52), e[1] * (1.0 + k[1] * 2.0 ** -52)]


def edge_error(S, X, f, c, z):
    """z - cam_map(project(S.map(X))).  X, z: lists of components, floats or arrays over the correspondences
    (numpy's elementwise +, -, *, / are the same IEEE operations as the scalar ones, one edge at a time)."""
    p = sim3_map(S, X)
    return [z[0] - ((p[0] / p[2]) * f[0] + c[0]), z[1] - ((p[1] / p[2]) * f[1] + c[1])]


def chi2_of(e, w):
    return e[0] * (w * e[0]) + e[1] * (w * e[1])


def huber(delta, c):
    """RobustKernelHuber::robustify: (rho, rho')."""
    dsqr = delta * delta
    c = np.asarray(c, np.float64)
    sq = np.sqrt(np.where(c <= dsqr, 1.0, c))
    return np.where(c <= dsqr, c, 2 * sq * delta - dsqr), np.where(c <= dsqr, 1.0, delta / sq)


def seq_sum(rows):
    """The sum of the rows in order, one addition at a time, as a loop over the edges adds them."""
    rows = np.asarray(rows, np.float64)
    if len(rows) == 0:
        return np.zeros(rows.shape[1:])
    return np.cumsum(rows, axis=0)[-1]


def interleave(a, b):
    """Rows a[0], b[0], a[1], b[1], ...: the edges in insertion order (e12 then e21 per correspondence)."""
    out = np.empty((2 * len(a),) + a.shape[1:])
    out[0::2], out[1::2] = a, b
    return out


def pk7(r, c):
    return r * 7 - r * (r - 1) // 2 + (c - r)


def solve7(H, b, lam):
    """LDL^T of the packed upper triangle + lambda I, unpivoted; (ok, x)."""
    A = [float(v) for v in H]
    b = [float(v) for v in b]
    for i in range(7):
        A[pk7(i, i)] += lam
    ok = True
    for j in range(7):
        v = A[pk7(j, j)]
        for k in range(j):
            v -= A[pk7(k, j)] * A[pk7(k, j)] * A[pk7(k, k)]
        ok = ok and v >= 0 and math.isfinite(v)
        A[pk7(j, j)] = v
        for i in range(j + 1, 7):
            s = A[pk7(j, i)]
            for k in range(j):
                s -= A[pk7(k, i)] * A[pk7(k, j)] * A[pk7(k, k)]
            A[pk7(j, i)] = s / v if v != 0 else 0.0
    y = [0.0] * 7
    for i in range(7):
        s = b[i]
        for k in range(i):
            s -= A[pk7(k, i)] * y[k]
        y[i] = s
    for i in range(7):
        y[i] = y[i] / A[pk7(i, i)] if A[pk7(i, i)] != 0 else 0.0
    x = [0.0] * 7
    for i in range(6, -1, -1):
        s = y[i]
        for k in range(i + 1, 7):
            s -= A[pk7(i, k)] * x[k]
        x[i] = s
    if not ok:
        x = [0.0] * 7
    return ok, x


class Pair:
    """The graph of one pair: correspondences (arrays over them), the estimate, the errors of the last
    computeActiveErrors."""

    def __init__(self, b, p, jitter_seed=None):
        k1, e1 = int(b["kp1_begin"][p]), int(b["kp1_begin"][p + 1])
        k2 = int(b["kp2_begin"][p])
        isig = np.array([float(F32(v)) for v in b["inv_level_sigma2"]])
        self.slots, j2 = [], []
        for i in range(k1, e1):   # Optimizer.cc:991-1001
            m = int(b["match12"][i])
            if b["mp1_valid"][i] and m >= 0 and b["mp2_valid"][k2 + m]:
                self.slots.append(i)
                j2.append(k2 + m)
        n = self.n = len(self.slots)
        X1 = np.array([world_to_camera(b["pose1"][p], b["mp1_xw"][i]) for i in self.slots]).reshape(n, 3)
        X2 = np.array([world_to_camera(b["pose2"][p], b["mp2_xw"][j]) for j in j2]).reshape(n, 3)
        self.X1, self.X2 = [X1[:, k] for k in range(3)], [X2[:, k] for k in range(3)]
        z1 = np.asarray(b["kp1_xy"], np.float32).reshape(-1, 2)[self.slots].astype(np.float64).reshape(n, 2)
        z2 = np.asarray(b["kp2_xy"], np.float32).reshape(-1, 2)[j2].astype(np.float64).reshape(n, 2)
        self.z1, self.z2 = [z1[:, 0], z1[:, 1]], [z2[:, 0], z2[:, 1]]
        self.w1 = isig[np.asarray(b["kp1_octave"])[self.slots].astype(int)] if n else np.zeros(0)
        self.w2 = isig[np.asarray(b["kp2_octave"])[j2].astype(int)] if n else np.zeros(0)
        K1, K2 = ([float(F32(v)) for v in b[k][p]] for k in ("camera1", "camera2"))
        self.f1, self.c1, self.f2, self.c2 = K1[:2], K1[2:], K2[:2], K2[2:]
        self.fix_scale = bool(b["fix_scale"])
        self.max_chi2 = float(F32(b["max_chi2"]))
        self.delta = math.sqrt(self.max_chi2)
        self.est = to_g2o(b["s12"][p])
        self.active = np.ones(n, bool)
        self.err = None   # (e12, e21), each [e0, e1] over the correspondences: the last computeActiveErrors
        self.jit = _Jitter(jitter_seed)
        self.rhos = []

    def errors_at(self, S):
        Si = sim3_inverse(S)
        return (self.jit(edge_error(S, self.X2, self.f1, self.c1, self.z1)),
                self.jit(edge_error(Si, self.X1, self.f2, self.c2, self.z2)))

    def edge_chi2(self):
        return chi2_of(self.err[0], self.w1), chi2_of(self.err[1], self.w2)

    def robust_chi2(self):
        c12, c21 = self.edge_chi2()
        r = interleave(huber(self.delta, c12)[0], huber(self.delta, c21)[0])
        return float(seq_sum(r[np.repeat(self.active, 2)]))

    def oplus(self, S, u):
        u = [float(v) for v in u]
        if self.fix_scale:
            u[6] = 0.0
        return sim3_mul(sim3_exp(u), S)

    def jacobians(self):
        """linearizeOplus of every edge (base_binary_edge.hpp:143-200): J[e][r][d], arrays over the
        correspondences, e = 0 for e12 and 1 for e21."""
        scalar = 1.0 / (2 * DELTA)
        J = [[[None] * 7 for _ in range(2)] for _ in range(2)]
        for d in range(7):
            u = [0.0] * 7
            u[d] = DELTA
            plus = self.errors_at(self.oplus(self.est, u))
            u[d] = -DELTA
            minus = self.errors_at(self.oplus(self.est, u))
            for e in range(2):
                for r in range(2):
                    J[e][r][d] = scalar * (plus[e][r] - minus[e][r])
        return J

    def build_system(self):
        """constructQuadraticForm over the active edges in insertion order: packed H (28), b (7)."""
        J = self.jacobians()
        parts = []
        for e, om in ((0, self.w1), (1, self.w2)):
            err, Je = self.err[e], J[e]
            _, r1 = huber(self.delta, chi2_of(err, om))
            or0, or1 = r1 * -(om * err[0]), r1 * -(om * err[1])
            w = r1 * om
            cols = []
            for r in range(7):
                for cc in range(r, 7):
                    cols.append(Je[0][r] * w * Je[0][cc] + Je[1][r] * w * Je[1][cc])
            for r in range(7):
                cols.append(Je[0][r] * or0 + Je[1][r] * or1)
            parts.append(np.stack([np.broadcast_to(c, (self.n,)) for c in cols], axis=1))
        tot = seq_sum(interleave(parts[0], parts[1])[np.repeat(self.active, 2)])
        return list(tot[:28]), list(tot[28:])

    def optimize(self, iterations):
        """SparseOptimizer::optimize over OptimizationAlgorithmLevenberg::solve; returns the iterations run."""
        if not self.active.any():
            return 0
        lam, ni, nbad, done = 0.0, 2.0, 0, 0
        for it in range(iterations):
            done += 1
            self.err = self.errors_at(self.est)
            cur = self.robust_chi2()
            ini = cur
            H, b = self.build_system()
            if it == 0:
                lam = 1e-5 * max(abs(H[pk7(j, j)]) for j in range(7))
                ni, nbad = 2.0, 0
            rho, qn = 0.0, 0
            while True:
                saved = self.est
                ok, x = solve7(H, b, lam)
                self.est = self.oplus(self.est, x)
                self.err = self.errors_at(self.est)
                tmp = self.robust_chi2()
                if not ok:
                    tmp = DBL_MAX
                rho = cur - tmp
                sc = 0.0
                for j in range(7):
                    sc += x[j] * (lam * x[j] + float(b[j]))
                rho /= sc + 1e-3
                self.rhos.append(rho)
                if rho > 0 and math.isfinite(tmp):
                    u = 2 * rho - 1
                    alpha = min(1. - u * u * u, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni = 2.0
                    cur = tmp
                else:
                    lam *= ni
                    ni *= 2
                    self.est = saved
                qn += 1
                if not (rho < 0 and qn < 10):
                    break
            if qn == 10 or rho == 0:
                break
            nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
            if nbad >= 3:
                break
        return done

    def classify(self):
        """chi2() of the last computed errors (Optimizer.cc:1051-1068 / :1079-1094); returns (removed,
        chi2 [n, 2] with nan rows for the edges already removed)."""
        c12, c21 = self.edge_chi2()
        chis = np.where(self.active[:, None], np.stack([c12, c21], axis=1), np.nan)
        bad = self.active & ((c12 > self.max_chi2) | (c21 > self.max_chi2))
        self.active = self.active & ~bad
        return list(np.nonzero(bad)[0]), chis


def optimize_pair(b, p, jitter_seed=None):
    """One pair: dict(s12 [13] f32, s12_g2o [8], removed slots, n_inliers, iterations (2), rho trace, chi2 at
    both classifications, last_trial_rejected of round 1)."""
    g = Pair(b, p, jitter_seed)
    out = dict(s12=np.array(b["s12"][p], np.float32).copy(), iterations=[0, 0], n_inliers=0, chi2=[[], []],
               removed=[], n_corr=g.n)
    if g.n:
        out["iterations"][0] = g.optimize(5)
        n_rho = len(g.rhos)
        out["last_trial_rejected"] = n_rho > 0 and not g.rhos[-1] > 0
        rem, out["chi2"][0] = g.classify()
        out["removed"] += [g.slots[n] for n in rem]
        nbad = len(rem)
        if g.n - nbad >= 10:
            out["iterations"][1] = g.optimize(10 if nbad > 0 else 5)
            rem, out["chi2"][1] = g.classify()
            out["removed"] += [g.slots[n] for n in rem]
            out["n_inliers"] = g.n - nbad - len(rem)
            out["s12"] = from_g2o(g.est)
    out["s12_g2o"] = g2o_row(g.est)
    out["rho"] = list(g.rhos)
    return out


def optimize_sim3(b, jitter_seed=None, pairs=None):
    """The batch: dict(s12 [F, 13] f32, s12_g2o [F, 8], match12 [K1], n_inliers [F], iterations [F, 2], trace =
    the per-pair dicts).  `pairs` restricts the work to those pairs (the others keep the input)."""
    F = len(b["kp1_begin"]) - 1
    res = dict(s12=np.array(b["s12"], np.float32).reshape(F, 13).copy(), s12_g2o=np.zeros((F, 8)),
               match12=np.array(b["match12"], np.int32).copy(), n_inliers=np.zeros(F, np.int32),
               iterations=np.zeros((F, 2), np.int32), trace=[None] * F)
    for p in (range(F) if pairs is None else pairs):
        o = optimize_pair(b, p, None if jitter_seed is None else jitter_seed * 1000 + p)
        res["s12"][p], res["s12_g2o"][p] = o["s12"], o["s12_g2o"]
        res["match12"][o["removed"]] = -1
        res["n_inliers"][p], res["iterations"][p] = o["n_inliers"], o["iterations"]
        res["trace"][p] = o
    return res


def spread(a, b):
    """Distance between two s12_g2o rows: (rotation angle, |dt| / |t|, |ds| / s)."""
    qa, qb = np.asarray(a[:4]), np.asarray(b[:4])
    qa, qb = qa / np.linalg.norm(qa), qb / np.linalg.norm(qb)
    # the angle of qa^-1 qb from its vector part (acos of the dot loses everything below 1e-8)
    rel = q_mul([-qa[0], -qa[1], -qa[2], qa[3]], list(qb))
    ang = 2 * math.atan2(math.sqrt(rel[0] ** 2 + rel[1] ** 2 + rel[2] ** 2), abs(rel[3]))
    ta, tb = np.asarray(a[4:7]), np.asarray(b[4:7])
    return np.array([ang, np.linalg.norm(ta - tb) / max(np.linalg.norm(ta), 1e-300), abs(a[7] - b[7]) / abs(a[7])])
