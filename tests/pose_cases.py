"""Hand-built PoseOptimization frames, one row per branch that synth.make_pose_batch cannot reach, shared by
tests/test_pose_cases_oracle.py (the oracle's trace witnesses each row's claim, far from a tie),
tests/test_pose_ref.py (the numpy restatement against the oracle) and tests/test_pose_cases_gpu.py (the device
against the oracle on every row).

A row is a small batch (1 .. 6 frames, 12 .. 1100 edges each) in the layout of make_pose_batch.  `iterations`
and `reasons` are the oracle's, per frame and round, as literals from a CPU run; None where the row's claim is
not about them (there a round may end on a rounding-level tie, which is nothing to pin).  Seeds were picked
on the oracle alone, for the conditions test_pose_cases_oracle.py asserts."""
from collections import namedtuple

import numpy as np

from orb_slam2_refactored_amd.synth import KITTI, make_pose_batch

F32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
KEYS = ("pose_R", "pose_t", "cam", "xw", "obs", "inv_sigma2")


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j, k = axis, (axis + 1) % 3, (axis + 2) % 3
    R = np.zeros((3, 3))
    R[i, i] = 1
    R[j, j] = R[k, k] = c
    R[j, k], R[k, j] = -s, s
    return R


def project(R, t, cam, X):
    """(u, v, u - bf / z) of world points X at pose (R, t), and the camera depth."""
    fx, fy, cx, cy, bf = cam
    Xc = X @ np.asarray(R).reshape(3, 3).T + t
    u = fx * Xc[:, 0] / Xc[:, 2] + cx
    v = fy * Xc[:, 1] / Xc[:, 2] + cy
    return np.stack([u, v, u - bf / Xc[:, 2]], axis=1), Xc[:, 2]


def concat(batches):
    """One batch of the frames of several."""
    out = {k: np.concatenate([np.asarray(b[k], np.float64) for b in batches]) for k in KEYS}
    counts = np.concatenate([np.diff(b["edge_begin"]) for b in batches])
    out["edge_begin"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return out


def take(batch, frames):
    """The batch of the given frames of `batch`, in the given order."""
    eb = batch["edge_begin"]
    out = {k: np.ascontiguousarray(batch[k][list(frames)]) for k in KEYS[:3]}
    idx = np.concatenate([np.arange(eb[f], eb[f + 1]) for f in frames] + [np.zeros(0, np.int64)]).astype(np.int64)
    for k in KEYS[3:]:
        out[k] = np.ascontiguousarray(batch[k][idx])
    out["edge_begin"] = np.concatenate([[0], np.cumsum([eb[f + 1] - eb[f] for f in frames])]).astype(np.int32)
    return out


def inputs(batch):
    """The batch without the generator's ground truth."""
    return {k: batch[k] for k in KEYS + ("edge_begin",)}


# --- the rows' constructions -------------------------------------------------------------------------------------

def cams(seed):
    """Four frames, each with its own intrinsics (every one of fx, fy, cx, cy, bf 1.3 x the previous frame's,
    rounded to float32) and observations generated with them."""
    frames = []
    for f in range(4):
        s = 1.3 ** f
        cam = {k: (float(np.float32(v * s)) if k in ("fx", "fy", "cx", "cy", "bf") else v * s)
               for k, v in KITTI.items()}
        frames.append(make_pose_batch(seed + f, n_frames=1, n_edges=60, cam=cam))
    return concat(frames)


def swap_cameras(batch):
    """The same frames, each run with the next frame's camera."""
    return dict(batch, cam=np.roll(batch["cam"], -1, axis=0))


QUAT_TARGETS = {   # the prediction's rotation after the change of world frame; expected (branch, flipped)
    "quat-t": (np.eye(3), ("t", 0)),
    "quat-i0": (rot(0, 179.0), ("i0", 0)),
    "quat-i1": (rot(1, 179.0), ("i1", 0)),
    "quat-i2": (rot(2, 179.0), ("i2", 0)),
    "quat-wneg": (rot(0, 181.0), ("i0", 1)),
}


def quat(seed, which):
    """One generator frame in a world re-expressed by W (R' = R W, X' = W^T X: the same camera points), W chosen so
    that the predicted rotation becomes QUAT_TARGETS[which] times a tilt of about half a degree."""
    b = make_pose_batch(seed, n_frames=1, n_edges=60)
    tilt = rot(0, -0.35) @ rot(1, -0.4) @ rot(2, -0.3)   # keeps 179 degrees below and 181 above 180
    R0 = b["pose_R"][0].reshape(3, 3)
    W = R0.T @ QUAT_TARGETS[which][0] @ tilt
    return dict(inputs(b), pose_R=F32((R0 @ W).reshape(1, 9)), xw=F32(b["xw"] @ W))


def near_plane(seed, edge_depth, rot_deg, trans_m, n=40):
    """A generator frame whose edge 0 sits `edge_depth` metres in front of the true camera centre, slightly off
    the axis, observed where it projects: the projection's curvature there keeps LM from converging fast."""
    b = make_pose_batch(seed, n_frames=1, n_edges=n, outlier_frac=0.0, rot_deg=rot_deg, trans_m=trans_m)
    R, t = b["gt_R"][0].reshape(3, 3), b["gt_t"][0]
    Xc = np.array([0.3 * edge_depth, -0.2 * edge_depth, edge_depth])
    xw = b["xw"].copy()
    xw[0] = R.T @ (Xc - t)   # kept in fp64: float32 cannot hold a micrometre at this distance from the origin
    obs = b["obs"].copy()
    obs[0] = F32(project(R, t, b["cam"][0], xw[:1])[0][0])
    obs[0, 2] = -1.0
    return dict(inputs(b), xw=xw, obs=obs)


def solve_fail(seed, kind):
    """Prediction R = I, t = 0 (se3_map is exact there), truth a 0.03 degree / 3 mm step away; edge 0 has
    Xw = (x, y, 0), so its camera depth is exactly 0 in round 0: infinite / NaN terms in H, every solve fails.
    kind "mono": chi2 = inf, flagged; "stereo": x < 0, chi2 = inf, flagged; "stereo-nan": x > 0, the disparity
    term is inf - inf, chi2 = NaN, which no comparison flags: the edge stays active and every round fails."""
    rng = np.random.default_rng(seed)
    n = 40
    cam = F32([KITTI[k] for k in ("fx", "fy", "cx", "cy", "bf")])
    Rt, tt = rot(1, 0.03) @ rot(0, -0.015), np.array([0.003, -0.0015, 0.002])
    u, v, z = rng.uniform(0, 1241, n), rng.uniform(0, 376, n), rng.uniform(3, 60, n)
    Xc = np.stack([(u - cam[2]) * z / cam[0], (v - cam[3]) * z / cam[1], z], axis=1)
    xw = F32((Xc - tt) @ Rt)
    o, _ = project(Rt, tt, cam, xw)
    o[:, :2] += rng.normal(0, 0.3, (n, 2))
    st = np.arange(n) % 3 == 0
    o[:, 2] = np.where(st, o[:, 2] + rng.normal(0, 0.3, n), -1.0)
    xw[0] = {"mono": (1.5, -0.75, 0.0), "stereo": (-1.5, 0.75, 0.0), "stereo-nan": (1.5, 0.75, 0.0)}[kind]
    o[0] = (300.0, 200.0, -1.0 if kind == "mono" else 250.0)
    return dict(edge_begin=np.array([0, n], np.int32), pose_R=np.eye(3).reshape(1, 9), pose_t=np.zeros((1, 3)),
                cam=cam.reshape(1, 5), xw=xw, obs=F32(o), inv_sigma2=np.ones(n))


BEHIND = (7, 23, 41)


def behind(seed):
    """60 edges; the BEHIND ones lie 4 .. 7 m behind the camera plane and are observed somewhere in the image."""
    b = make_pose_batch(seed, n_frames=1, n_edges=60, outlier_frac=0.0)
    rng = np.random.default_rng(seed + 1000)
    R, t = b["gt_R"][0].reshape(3, 3), b["gt_t"][0]
    xw = b["xw"].copy()
    for e in BEHIND:
        Xc = np.array([rng.uniform(-3, 3), rng.uniform(-1, 1), -rng.uniform(4, 7)])
        xw[e] = F32(R.T @ (Xc - t))
    return dict(inputs(b), xw=xw)


def exact_fit():
    """Every residual exactly 0.0 in fp64 (as ba_cases.exact_fit_problem): identity rotation, dyadic translation,
    points and intrinsics, so each projection is a short dyadic number; 1 / z is exact in float for the stereo
    edges.  b == 0, x == 0, rho == 0: one trial per round and nothing moves."""
    rng = np.random.default_rng(4321)
    n = 24
    fx = fy = 512.0
    cx, cy, bf = 320.0, 240.0, 64.0
    t = np.array([-1.0, 0.5, 0.0])
    X = np.stack([0.5 * rng.integers(2, 9, n), 0.5 * rng.integers(-3, 2, n), rng.choice([4.0, 8.0, 16.0], n)], axis=1)
    Xc = X + t
    u = fx * Xc[:, 0] / Xc[:, 2] + cx
    v = fy * Xc[:, 1] / Xc[:, 2] + cy
    ur = np.where(np.arange(n) % 3 == 0, u - bf / Xc[:, 2], -1.0)
    obs = np.stack([u, v, ur], axis=1)
    assert np.array_equal(F32(obs), obs) and (obs[:, :2] >= 0).all() and (ur[::3] >= 0).all()
    return dict(edge_begin=np.array([0, n], np.int32), pose_R=np.eye(3).reshape(1, 9), pose_t=t.reshape(1, 3),
                cam=np.array([[fx, fy, cx, cy, bf]]), xw=X, obs=obs,
                inv_sigma2=np.where(rng.integers(0, 2, n) == 1, 1.0, 0.25))


def few_active(seed, n_good):
    """12 edges, all but n_good of them moved by 60 .. 200 px: a later round runs on the n_good that are left."""
    b = make_pose_batch(seed, n_frames=1, n_edges=12, outlier_frac=0.0, rot_deg=0.02, trans_m=0.005)
    rng = np.random.default_rng(seed + 500)
    obs = b["obs"].copy()
    bad = np.arange(12) >= n_good
    d = rng.choice([-1.0, 1.0], (12, 2)) * rng.uniform(60, 200, (12, 2))
    obs[bad, :2] += d[bad]
    st = obs[:, 2] >= 0
    obs[bad & st, 2] += d[bad & st, 0]
    return dict(inputs(b), obs=F32(obs))


def all_outliers():
    """tests/test_pose_gpu.py::test_pose_all_outliers' scene."""
    b = make_pose_batch(seed=7, n_frames=2, n_edges=40, outlier_frac=1.0)
    obs = b["obs"].copy()
    obs[:, 0] += 400.0
    return dict(inputs(b), obs=obs)


EDGE_COUNTS = (255, 256, 257, 1023, 1024, 1025)   # beside 256 lanes x 1 edge and the 1024 staged edges
NAMED = (0, 254, 255, 256, 1022, 1023, 1024)


def planted(E):
    """(planted outliers, their unplanted neighbours) among a frame's E edges."""
    p = sorted({e for e in NAMED + (E - 1,) if e < E})
    nb = sorted({e + d for e in p for d in (-1, 1) if 0 <= e + d < E} - set(p))
    return p, nb


def edge_counts(seed):
    """One ragged batch of EDGE_COUNTS edges.  The planted edges are moved by 40 px (20 sigma at the coarsest
    octave); their neighbours are put on their exact projection, so they are clean whatever the noise drew."""
    b = make_pose_batch(seed, n_frames=len(EDGE_COUNTS), n_edges=list(EDGE_COUNTS), outlier_frac=0.0)
    obs = b["obs"].copy()
    for f, E in enumerate(EDGE_COUNTS):
        e0 = int(b["edge_begin"][f])
        p, nb = planted(E)
        st = obs[e0:e0 + E, 2] >= 0
        clean, _ = project(b["gt_R"][f], b["gt_t"][f], b["cam"][f], b["xw"][e0:e0 + E])
        for e in nb:
            obs[e0 + e, :2] = clean[e, :2]
            if st[e]:
                obs[e0 + e, 2] = clean[e, 2]
        for e in p:
            obs[e0 + e, :2] += 40.0
            if st[e]:
                obs[e0 + e, 2] += 40.0
    return dict(inputs(b), obs=F32(obs))


# id, what the trace must witness, constructor, its arguments; iterations / reasons: per frame, per round
Case = namedtuple("Case", "id claim make args iterations reasons")

CASES = [
    Case("cams", "cam is read per frame: another frame's camera changes n_inliers", cams, (100,), None, None),
    Case("quat-t", "q_from_R: trace > 0", quat, (21, "quat-t"), None, None),
    Case("quat-i0", "q_from_R: i == 0", quat, (21, "quat-i0"), None, None),
    Case("quat-i1", "q_from_R: i == 1", quat, (21, "quat-i1"), None, None),
    Case("quat-i2", "q_from_R: i == 2", quat, (21, "quat-i2"), None, None),
    Case("quat-wneg", "normalizeRotation flips a w < 0", quat, (21, "quat-wneg"), None, None),
    Case("budget", "optimize(10) runs all 10 iterations", near_plane, (4, 1e-6, 0.5, 0.1),
         ((10, 10, 10, 10),), (("budget",) * 4,)),
    Case("solve-fail-mono", "po_solve !ok, tmp = DBL_MAX, rho NaN", solve_fail, (1, "mono"),
         ((10, None, None, None),), (("budget", None, None, None),)),
    Case("solve-fail-stereo", "the same through the stereo edge", solve_fail, (2, "stereo"),
         ((10, None, None, None),), (("budget", None, None, None),)),
    Case("solve-fail-nan", "chi2 NaN is never flagged: every round fails", solve_fail, (3, "stereo-nan"),
         ((10, 10, 10, 10),), (("budget",) * 4,)),
    Case("behind", "points behind the camera plane: finite chi2, flagged", behind, (0,), None, None),
    Case("exact-fit", "rho == 0 on the first trial", exact_fit, (), ((1, 1, 1, 1),), (("rho0",) * 4,)),
    Case("active-2", "a round with 2 active edges: rank-deficient H", few_active, (21, 2),
         ((7, 7, 7, 7),), (("nbad",) * 4,)),
    Case("active-1", "a round with 1 active edge", few_active, (21, 1),
         ((7, 8, 8, 10),), (("nbad", "nbad", "nbad", "budget"),)),
    Case("all-out-then-none", "rounds without an active edge", all_outliers, (),
         (None, (8, 0, 0, 0)), (None, ("nbad", "none", "none", "none"))),
    Case("edges", "edge counts beside 256 and PO_LDS_EDGES", edge_counts, (30,), None, None),
]
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}

_built, _traced = {}, {}


def build_case(case):
    """The row's batch (built once per process and shared: treat it as read-only)."""
    if case.id not in _built:
        b = case.make(*case.args)
        _built[case.id] = {k: np.ascontiguousarray(b[k], np.int32 if k == "edge_begin" else np.float64)
                           for k in KEYS + ("edge_begin",)}
    return _built[case.id]


def oracle_result(oracle, case):
    """The oracle's traced result on the row (computed once per process and shared)."""
    if case.id not in _traced:
        _traced[case.id] = oracle.pose_optimization(build_case(case), trace=True)
    return _traced[case.id]
