"""Seeded synthetic inputs.  No datasets are available offline.

G(seed, W, H): background 128, 300 filled axis-aligned rectangles with uniform random
corners and uniform gray level 0..255 painted in order, plus i.i.d. integer noise U{-6..6},
clipped to u8.  Rectangle corners give FAST corners at every pyramid level.
"""
import numpy as np


def synth_image(seed: int, width: int, height: int, n_rects: int = 300) -> np.ndarray:
    rng = np.random.default_rng(seed)
    img = np.full((height, width), 128, np.int16)
    xs = np.sort(rng.integers(0, width, size=(n_rects, 2)), axis=1)
    ys = np.sort(rng.integers(0, height, size=(n_rects, 2)), axis=1)
    gray = rng.integers(0, 256, size=n_rects)
    for (x0, x1), (y0, y1), g in zip(xs, ys, gray):
        img[y0:y1 + 1, x0:x1 + 1] = g
    img += rng.integers(-6, 7, size=(height, width)).astype(np.int16)
    return np.clip(img, 0, 255).astype(np.uint8)


def shifted_pair(seed: int, width: int, height: int, dx: int = 3, dy: int = 2):
    """C2 pair: A = G(seed), B = A shifted by (dx, dy) with edge replicate + fresh noise."""
    a = synth_image(seed, width, height)
    base = np.pad(a.astype(np.int16), ((dy, 0), (dx, 0)), mode="edge")[:height, :width]
    rng = np.random.default_rng(seed + 1000)
    b = np.clip(base + rng.integers(-3, 4, size=(height, width)), 0, 255).astype(np.uint8)
    return a, b


def pan_sequence(seed: int, width: int, height: int, n: int, dx: int = 3, dy: int = 2) -> np.ndarray:
    """A camera-pan sequence for the C2 / C5 "frame i matched to i-1" workload: frame 0 = G(seed) and
    frame k = G(seed) shifted by k*(dx, dy) with edge replicate plus fresh noise U{-3..3} (frame k and
    k-1 are the shifted pair of SURVEY.md §8d C2; the noise does not accumulate along the chain).
    Returns [n, H, W] uint8."""
    out = np.empty((n, height, width), np.uint8)
    a = synth_image(seed, width, height).astype(np.int16)
    out[0] = a
    rng = np.random.default_rng(seed + 1000)
    for k in range(1, n):
        base = np.pad(a, ((k * dy, 0), (k * dx, 0)), mode="edge")[:height, :width]
        out[k] = np.clip(base + rng.integers(-3, 4, size=(height, width)), 0, 255).astype(np.uint8)
    return out


def textured_image(seed: int, width: int, height: int) -> np.ndarray:
    """Texture-rich frame (FAST fires almost everywhere, thousands of candidates per level):
    low-frequency value noise (1/8 resolution, bilinear) at +-40 grey levels plus per-pixel
    Gaussian noise sigma 12, around 128."""
    rng = np.random.default_rng(seed)
    gh, gw = height // 8 + 2, width // 8 + 2
    g = rng.normal(0, 40, (gh, gw))
    ys = np.arange(height) / 8.0
    xs = np.arange(width) / 8.0
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
    low = (g[y0][:, x0] * (1 - fy) * (1 - fx) + g[y0 + 1][:, x0] * fy * (1 - fx) +
           g[y0][:, x0 + 1] * (1 - fy) * fx + g[y0 + 1][:, x0 + 1] * fy * fx)
    img = 128 + low + rng.normal(0, 12, (height, width))
    return np.ascontiguousarray(np.clip(np.rint(img), 0, 255).astype(np.uint8))


# KITTI 00-02 intrinsics (Examples/Stereo/KITTI00-02.yaml:8-25)
KITTI = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, bf=386.1448, width=1241, height=376)


def _rot_y(deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _small_rot(rng, sigma_deg):
    w = rng.normal(0, np.deg2rad(sigma_deg), 3)
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_ba_problem(seed: int = 0, n_kf: int = 20, n_pts: int = 3000, n_fixed: int = 2, stereo_frac: float = 0.2,
                    outlier_frac: float = 0.03, cam=KITTI, yaw_per_kf: float = 0.5):
    """C4: a LocalBundleAdjustment problem in the flattened orbba_problem layout.

    n_kf local keyframes moving forward along +z (0.5 m apart, 0.5 deg yaw per KF); KF 0 is the
    fixed gauge (`localKF->id == 0`, Optimizer.cc:551) and `n_fixed` extra fixed cameras observe
    some points (the fixedCameras set, :524-537).  Each point is seen by a run of K ~ U{2..6}
    keyframes; 20 % of observations are stereo (ur >= 0), octaves U{0..7} with pixel noise
    N(0, 1.2^oct) and invSigma2 = 1/1.2^(2 oct); 3 % outliers get +-U(15,40) px.  Initial poses
    are perturbed by 0.2 deg / 2 cm and points by 2 % of depth.
    """
    rng = np.random.default_rng(seed)
    P = n_kf + n_fixed
    R_true, t_true, C = [], [], []
    for k in range(P):
        kk = k if k < n_kf else -(k - n_kf + 1)   # fixed cameras behind KF 0
        Rwc = _rot_y(yaw_per_kf * kk)   # long windows: a smaller yaw keeps points in front of every camera
        c = np.array([0.02 * np.sin(kk), 0.0, 0.5 * kk])
        Rcw = Rwc.T
        R_true.append(Rcw)
        t_true.append(-Rcw @ c)
        C.append(c)
    fixed = np.zeros(P, np.uint8)
    fixed[0] = 1
    fixed[n_kf:] = 1
    pts, ep, ek, obs, info, camv = [], [], [], [], [], []
    for p in range(n_pts):
        K = int(rng.integers(2, 7))
        s = int(rng.integers(-n_fixed, n_kf - K + 1))
        kfs = [(k if k >= 0 else n_kf + (-k - 1)) for k in range(s, s + K)]
        zc = max(C[k][2] for k in kfs)
        X = np.array([rng.uniform(-15, 15), rng.uniform(-3, 3), zc + rng.uniform(5, 40)])
        pid = len(pts)
        pts.append(X)
        for k in kfs:
            Xc = R_true[k] @ X + t_true[k]
            u = cam["fx"] * Xc[0] / Xc[2] + cam["cx"]
            v = cam["fy"] * Xc[1] / Xc[2] + cam["cy"]
            octv = int(rng.integers(0, 8))
            sig = 1.2 ** octv
            u += rng.normal(0, sig)
            v += rng.normal(0, sig)
            ur = -1.0
            if rng.random() < stereo_frac:
                ur = u - cam["bf"] / Xc[2] + rng.normal(0, sig)
            if rng.random() < outlier_frac:
                u += rng.choice([-1, 1]) * rng.uniform(15, 40)
                v += rng.choice([-1, 1]) * rng.uniform(15, 40)
                if ur >= 0:
                    ur = u - cam["bf"] / Xc[2]
            ep.append(pid)
            ek.append(k)
            # measurements are floats in the reference (cv::KeyPoint pt, uright)
            obs.append([np.float32(u), np.float32(v), np.float32(ur) if ur >= 0 else -1.0])
            info.append(np.float32(1.0 / (sig * sig)))
            camv.append([np.float32(cam[k2]) for k2 in ("fx", "fy", "cx", "cy", "bf")])
    pose_R = np.zeros((P, 9))
    pose_t = np.zeros((P, 3))
    for k in range(P):
        R, t = R_true[k], t_true[k]
        if not fixed[k]:
            R = _small_rot(rng, 0.2) @ R
            t = t + rng.normal(0, 0.02, 3)
        pose_R[k] = R.reshape(-1)
        pose_t[k] = t
    pts = np.array(pts)
    depth = np.abs(pts[:, 2] - np.mean([c[2] for c in C]))
    pts0 = pts + rng.normal(0, 1, pts.shape) * (0.02 * depth)[:, None]
    return dict(pose_R=pose_R.astype(np.float32).astype(np.float64), pose_t=pose_t.astype(np.float32).astype(np.float64),
                pose_fixed=fixed, points=pts0.astype(np.float32).astype(np.float64),
                edge_point=np.array(ep, np.int32), edge_pose=np.array(ek, np.int32),
                edge_obs=np.array(obs, np.float64), edge_inv_sigma2=np.array(info, np.float64),
                edge_cam=np.array(camv, np.float64), gt_R=np.array([r.reshape(-1) for r in R_true]),
                gt_t=np.array(t_true), gt_points=pts)


STEREO_Z = (5.0, 7.0, 10.0, 14.0, 20.0, 28.0, 40.0, 56.0)   # SURVEY.md §8d C3 band depths (m)


def stereo_pair(seed: int, width: int = 1242, height: int = 375, bf: float = KITTI["bf"]):
    """C3 pair: L = G(seed, W, H); R = L warped by 8 vertical bands at depths STEREO_Z with disparity
    round(bf / Z) (R[y, x] = L[y, x + d]); pixels with no source (x + d >= W) are noise-filled; fresh
    noise U{-3..3} on R.  Returns (L, R, band_depth_of_right_column)."""
    L = synth_image(seed, width, height)
    rng = np.random.default_rng(seed + 2000)
    R = np.empty_like(L, dtype=np.int16)
    zcol = np.empty(width, np.float32)
    edges = np.linspace(0, width, len(STEREO_Z) + 1).astype(int)
    for b, z in enumerate(STEREO_Z):
        d = int(round(bf / z))
        for x in range(edges[b], edges[b + 1]):
            zcol[x] = z
            R[:, x] = L[:, x + d] if x + d < width else rng.integers(0, 256, size=height)
    R += rng.integers(-3, 4, size=R.shape).astype(np.int16)
    return L, np.clip(R, 0, 255).astype(np.uint8), zcol


def stereo_tri_geometry(cam=KITTI):
    """SearchForTriangulation geometry of the C3 setup: KF1 = the left camera at
    [I|0], KF2 = the right camera at [I|(-bf/fx, 0, 0)].  Returns (F12, ep2) in float32 as the caller
    computes them: F12 = K1^-T [t12]x R12 K2^-1 (ComputeF12, LocalMapping.cc:55-71, with the closed
    -form inverse of the upper-triangular K) and ep2 = CameraProjection(pose2).WorldToImage(Ow1)
    (ORBmatcher.cc:772-773, CameraProjection.h:49-55).  KF1's centre lies on KF2's principal plane,
    so 1/Z = inf and ep2 = (-inf, NaN), exactly as the reference's float arithmetic gives it."""
    f32 = np.float32
    fx, fy, cx, cy = f32(cam["fx"]), f32(cam["fy"]), f32(cam["cx"]), f32(cam["cy"])
    b = f32(cam["bf"]) / fx
    t12 = np.array([b, 0, 0], f32)          # -R1w R2w^T t2w + t1w with t2w = (-b, 0, 0)
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]], f32)
    Kinv = np.array([[f32(1) / fx, 0, -cx / fx], [0, f32(1) / fy, -cy / fy], [0, 0, 1]], f32)
    F12 = (Kinv.T @ tx @ Kinv).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        Xc = np.array([-b, 0, 0], f32)      # Rcw * Ow1 + tcw with Ow1 = 0
        invz = f32(1) / Xc[2]
        ep2 = np.array([invz * fx * Xc[0] + cx, invz * fy * Xc[1] + cy], f32)
    return F12.reshape(9), ep2


def make_pose_batch(seed: int = 0, n_frames: int = 8, n_edges=600, stereo_frac: float = 0.4,
                    outlier_frac: float = 0.1, rot_deg: float = 0.5, trans_m: float = 0.1, cam=KITTI):
    """C5: a batch of PoseOptimization problems in the orbba_pose_batch layout.

    Per frame: a random camera pose (yaw U(-180,180) deg, position U(-50,50) m in x/z), map points
    back-projected from uniform pixels at depth U(3, 60) m, octaves U{0..7} with pixel noise
    N(0, 1.2^oct) and invSigma2 = 1/1.2^(2 oct) (float, like Frame::pyramid.invSigmaSq);
    `stereo_frac` of the observations carry ur = u - bf/z + noise; `outlier_frac` are moved by
    +-U(10, 60) px.  The initial pose (the motion-model prediction) is the true pose perturbed by
    N(0, rot_deg) rotation and N(0, trans_m) translation.  Measurements, map points and
    intrinsics are rounded to float32, as the reference stores them.  n_edges: int or per-frame list.
    """
    rng = np.random.default_rng(seed)
    counts = [int(n_edges)] * n_frames if np.isscalar(n_edges) else [int(n) for n in n_edges]
    assert len(counts) == n_frames
    eb = np.zeros(n_frames + 1, np.int32)
    eb[1:] = np.cumsum(counts)
    camv = np.array([cam[k] for k in ("fx", "fy", "cx", "cy", "bf")], np.float32).astype(np.float64)
    fx, fy, cx, cy, bf = camv
    pose_R, pose_t, gt_R, gt_t = [], [], [], []
    xw, obs, info = [], [], []
    for f, n in enumerate(counts):
        Rcw = _rot_y(rng.uniform(-180, 180)) @ _small_rot(rng, 3.0)
        C = np.array([rng.uniform(-50, 50), rng.uniform(-2, 2), rng.uniform(-50, 50)])
        tcw = -Rcw @ C
        gt_R.append(Rcw.reshape(-1))
        gt_t.append(tcw)
        u = rng.uniform(0, cam["width"], n)
        v = rng.uniform(0, cam["height"], n)
        z = rng.uniform(3, 60, n)
        Xc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
        Xw = (Xc - tcw) @ Rcw   # Rcw^T (Xc - t)
        octv = rng.integers(0, 8, n)
        sig = 1.2 ** octv
        uo = u + rng.normal(0, 1, n) * sig
        vo = v + rng.normal(0, 1, n) * sig
        st = rng.random(n) < stereo_frac
        ur = np.where(st, u - bf / z + rng.normal(0, 1, n) * sig, -1.0)
        out = rng.random(n) < outlier_frac
        du = rng.choice([-1, 1], n) * rng.uniform(10, 60, n)
        dv = rng.choice([-1, 1], n) * rng.uniform(10, 60, n)
        uo = np.where(out, uo + du, uo)
        vo = np.where(out, vo + dv, vo)
        ur = np.where(out & st, ur + du, ur)
        o = np.stack([uo, vo, ur], 1).astype(np.float32).astype(np.float64)
        o[~st, 2] = -1.0
        obs.append(o)
        xw.append(Xw.astype(np.float32).astype(np.float64))
        info.append((1.0 / (sig * sig)).astype(np.float32).astype(np.float64))
        R0 = _small_rot(rng, rot_deg) @ Rcw
        t0 = tcw + rng.normal(0, trans_m, 3)
        pose_R.append(R0.astype(np.float32).astype(np.float64).reshape(-1))
        pose_t.append(t0.astype(np.float32).astype(np.float64))
    cat = (lambda a, w: np.concatenate(a).reshape(-1, w) if sum(counts) else np.zeros((0, w)))
    return dict(edge_begin=eb, pose_R=np.array(pose_R).reshape(n_frames, 9), pose_t=np.array(pose_t).reshape(n_frames, 3),
                cam=np.tile(camv, (n_frames, 1)), xw=cat(xw, 3), obs=cat(obs, 3),
                inv_sigma2=np.concatenate(info) if sum(counts) else np.zeros(0),
                gt_R=np.array(gt_R).reshape(n_frames, 9), gt_t=np.array(gt_t).reshape(n_frames, 3))


ORB_QUOTA_2000 = (434, 362, 302, 251, 209, 175, 145, 122)


def make_proj_batch(seed: int = 0, n_frames: int = 4, n_kp=2000, n_mp=1500, width: float = 1241.0,
                    height: float = 376.0, th: float = 1.0, nnratio: float = 0.8, dup_frac: float = 0.15,
                    odd_bounds: bool = False):
    """C6: SearchByProjection(Frame, local map points) inputs in the orbm_proj_batch layout (§8f row 2).

    Per frame: n_kp keypoints uniform over the image with octaves drawn by the 2000-feature
    quotas, random descriptors, 40 % stereo (ur = x - U(5, 60)), 5 % already claimed.  Map points:
    70 % are re-observations of a keypoint (projection = keypoint + N(0, 1.5 * 1.2^oct) px,
    descriptor = the keypoint's with U{0..60} bits flipped, trackScaleLevel = octave or octave+1),
    `dup_frac` of those reuse an already used keypoint (claim conflicts) and some carry an exact copy
    of another candidate's descriptor (distance ties); the rest are random.  90 % trackInView,
    95 % with observations, viewCos U(0.5, 1) with a third above 0.998.  Bounds are (0, W, 0, H) or
    fractional undistortion-like bounds when `odd_bounds`.  n_kp / n_mp: int or per-frame list.
    """
    rng = np.random.default_rng(seed)
    kps = [int(n_kp)] * n_frames if np.isscalar(n_kp) else [int(v) for v in n_kp]
    mps = [int(n_mp)] * n_frames if np.isscalar(n_mp) else [int(v) for v in n_mp]
    q = np.array(ORB_QUOTA_2000, float)
    q /= q.sum()
    scale = (1.2 ** np.arange(8)).astype(np.float32)
    F = dict(kp_xy=[], kp_octave=[], kp_uright=[], kp_desc=[], kp_claimed=[], bounds=[], mp_valid=[], mp_proj=[],
             mp_view_cos=[], mp_level=[], mp_desc=[], mp_has_obs=[])
    for f in range(n_frames):
        n, m = kps[f], mps[f]
        if odd_bounds:
            b = np.array([rng.uniform(-8, 2), width + rng.uniform(-2, 8), rng.uniform(-6, 2), height + rng.uniform(-2, 6)])
        else:
            b = np.array([0.0, width, 0.0, height])
        x = rng.uniform(b[0] - 4, b[1] + 4, n)   # a few fall outside the grid (undistorted points)
        y = rng.uniform(b[2] - 4, b[3] + 4, n)
        octv = rng.choice(8, size=n, p=q)
        desc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        st = rng.random(n) < 0.4
        ur = np.where(st, x - rng.uniform(5, 60, n), -1.0)
        claimed = (rng.random(n) < 0.05).astype(np.uint8)
        F["kp_xy"].append(np.stack([x, y], 1).astype(np.float32))
        F["kp_octave"].append(octv.astype(np.int32))
        F["kp_uright"].append(ur.astype(np.float32))
        F["kp_desc"].append(desc)
        F["kp_claimed"].append(claimed)
        F["bounds"].append(b.astype(np.float32))
        proj = np.zeros((m, 3))
        lvl = np.zeros(m, np.int32)
        mdesc = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
        used = []
        for j in range(m):
            if n > 0 and rng.random() < 0.7:
                i = int(rng.choice(used)) if used and rng.random() < dup_frac else int(rng.integers(0, n))
                used.append(i)
                s = 1.5 * scale[octv[i]]
                u, v = x[i] + rng.normal(0, s), y[i] + rng.normal(0, s)
                d = desc[i].copy()
                if rng.random() < 0.1:
                    # an exact copy of a random keypoint's descriptor: ties with the true match
                    d = desc[int(rng.integers(0, n))].copy()
                flips = rng.choice(256, size=int(rng.integers(0, 61)), replace=False)
                for bit in flips:
                    d[bit >> 3] ^= np.uint8(1 << (bit & 7))
                mdesc[j] = d
                lvl[j] = min(int(octv[i]) + int(rng.integers(0, 2)), 7)
                uR = (u - (x[i] - ur[i]) + rng.normal(0, 1.0)) if st[i] else u - rng.uniform(5, 60)
                if rng.random() < 0.1:
                    uR += rng.uniform(-30, 30)
                proj[j] = (u, v, uR)
            else:
                proj[j] = (rng.uniform(b[0], b[1]), rng.uniform(b[2], b[3]), 0.0)
                proj[j, 2] = proj[j, 0] - rng.uniform(5, 60)
                lvl[j] = int(rng.integers(0, 8))
        F["mp_valid"].append((rng.random(m) < 0.9).astype(np.uint8))
        F["mp_proj"].append(proj.astype(np.float32))
        vc = rng.uniform(0.5, 1.0, m)
        vc = np.where(rng.random(m) < 0.33, rng.uniform(0.9975, 1.0, m), vc)
        F["mp_view_cos"].append(vc.astype(np.float32))
        F["mp_level"].append(lvl)
        F["mp_desc"].append(mdesc)
        F["mp_has_obs"].append((rng.random(m) < 0.95).astype(np.uint8))
    out = {}
    for k, v in F.items():
        out[k] = np.concatenate(v) if k != "bounds" else np.stack(v)
    out["kp_begin"] = np.concatenate([[0], np.cumsum(kps)]).astype(np.int32)
    out["mp_begin"] = np.concatenate([[0], np.cumsum(mps)]).astype(np.int32)
    out["scale_factors"] = scale
    out["th"] = float(th)
    out["nnratio"] = float(nnratio)
    return out


def tile_proj_batch(b: dict, reps: int) -> dict:
    """`reps` copies of a make_proj_batch batch back to back (a large batch without regenerating)."""
    out = dict(b)
    F = len(b["kp_begin"]) - 1
    for k in ("kp_xy", "kp_octave", "kp_uright", "kp_desc", "kp_claimed", "mp_valid", "mp_proj", "mp_view_cos",
              "mp_level", "mp_desc", "mp_has_obs"):
        if b.get(k) is not None:
            out[k] = np.concatenate([b[k]] * reps)
    out["bounds"] = np.concatenate([b["bounds"]] * reps)
    for k in ("kp_begin", "mp_begin"):
        per = np.diff(b[k])
        out[k] = np.concatenate([[0], np.cumsum(np.tile(per, reps))]).astype(np.int32)
    assert len(out["kp_begin"]) == F * reps + 1
    return out


def tile_ragged_batch(b: dict, reps: int) -> dict:
    """`reps` copies of a ragged batch back to back (a large batch without regenerating).  Every
    `*_begin` array (n + 1 prefix offsets) is re-prefixed; an array whose length equals the total of
    one prefix, or the number of batch entries, is repeated; other values (scalars, host tables such
    as scale_factors) are kept."""
    out = dict(b)
    begins = {k: v for k, v in b.items() if k.endswith("_begin")}
    n = len(next(iter(begins.values()))) - 1
    totals = {int(v[-1]) for v in begins.values()}
    for k, v in b.items():
        if k in begins:
            out[k] = np.concatenate([[0], np.cumsum(np.tile(np.diff(v), reps))]).astype(v.dtype)
        elif isinstance(v, np.ndarray) and v.ndim >= 1 and k != "scale_factors" and (len(v) in totals or len(v) == n):
            out[k] = np.concatenate([v] * reps)
    return out


def make_vocabulary(seed: int = 0, k: int = 10, L: int = 4, scoring: int = 0, weighting: int = 0,
                    early_leaf: float = 0.05, stop_frac: float = 0.03, order: str = "bfs"):
    """A synthetic DBoW2 ORB vocabulary (the real ORBvoc.txt is not available offline).

    A k-ary tree of depth L: children descriptors are the parent's with U{16..48} bits flipped (root
    children random), so descriptor distance follows the tree.  `early_leaf` of the internal nodes
    below level 2 stop early (leaves above level L, as k-means trees have), leaves get idf-like
    weights U(0.5, 8) and `stop_frac` of them weight 0 (stopped words); internal nodes weight 0.
    Nodes are numbered in `order` ("bfs" or "dfs"; the text format only needs parents first).
    Returns dict(k, L, scoring, weighting, parent, is_leaf, desc, weight) with node 0 = root."""
    rng = np.random.default_rng(seed)
    parent, is_leaf, desc, weight, depth = [0], [0], [np.zeros(32, np.uint8)], [0.0], [0]

    def new_node(p, d):
        i = len(parent)
        parent.append(p)
        depth.append(d)
        if p == 0:
            desc.append(rng.integers(0, 256, 32, dtype=np.uint8))
        else:
            x = desc[p].copy()
            for bit in rng.choice(256, size=int(rng.integers(16, 49)), replace=False):
                x[bit >> 3] ^= np.uint8(1 << (bit & 7))
            desc.append(x)
        leaf = d == L or (d >= 2 and rng.random() < early_leaf)
        is_leaf.append(1 if leaf else 0)
        weight.append(0.0 if not leaf else (0.0 if rng.random() < stop_frac else float(rng.uniform(0.5, 8.0))))
        return i

    if order == "bfs":
        frontier = [0]
        while frontier:
            nxt = []
            for p in frontier:
                if p != 0 and is_leaf[p]:
                    continue
                for _ in range(k):
                    nxt.append(new_node(p, depth[p] + 1))
            frontier = nxt
    else:
        def rec(p):
            for _ in range(k):
                c = new_node(p, depth[p] + 1)
                if not is_leaf[c]:
                    rec(c)
        rec(0)
    # text round trip precision: weights as the reference's ostream << double (6 significant digits)
    w = np.array([float(f"{x:g}") for x in weight])
    return dict(k=k, L=L, scoring=scoring, weighting=weighting, parent=np.array(parent, np.int32),
                is_leaf=np.array(is_leaf, np.uint8), desc=np.stack(desc).astype(np.uint8), weight=w)


def write_vocabulary_text(voc: dict, path) -> None:
    """saveToTextFile format (TemplatedVocabulary.h:1434-1450)."""
    lines = [f"{voc['k']} {voc['L']}  {voc['scoring']} {voc['weighting']}"]
    for i in range(1, len(voc["parent"])):
        d = " ".join(str(int(b)) for b in voc["desc"][i])
        lines.append(f"{voc['parent'][i]} {int(voc['is_leaf'][i])} {d}  {voc['weight'][i]:g}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def vocabulary_features(voc: dict, seed: int, n: int, near: float = 0.8) -> np.ndarray:
    """n descriptors: `near` of them a random leaf's descriptor with U{0..40} flips, the rest random,
    some repeated (same word several times)."""
    rng = np.random.default_rng(seed)
    leaves = np.nonzero(voc["is_leaf"])[0]
    out = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    for i in range(n):
        if rng.random() < near and len(leaves):
            x = voc["desc"][int(rng.choice(leaves))].copy()
            for bit in rng.choice(256, size=int(rng.integers(0, 41)), replace=False):
                x[bit >> 3] ^= np.uint8(1 << (bit & 7))
            out[i] = x
        if i > 0 and rng.random() < 0.05:
            out[i] = out[int(rng.integers(0, i))]
    return out


def make_full_vocabulary(seed: int = 0, k: int = 10, L: int = 6):
    """A full k-ary depth-L tree built level by level (ORBvoc.txt's shape: k = 10, L = 6, ~1.1 M nodes),
    BFS-numbered, children = parent with ~32 bits flipped, leaf weights U(0.5, 8), TF-IDF / L1."""
    rng = np.random.default_rng(seed)
    parents = [np.zeros(1, np.int64)]
    descs = [np.zeros((1, 32), np.uint8)]
    start = 0
    for d in range(1, L + 1):
        prev = descs[-1]
        pids = np.repeat(np.arange(start, start + len(prev)), k)
        base = np.repeat(prev, k, axis=0)
        if d == 1:
            base = rng.integers(0, 256, size=base.shape, dtype=np.uint8)
        else:
            flips = np.packbits(rng.integers(0, 256, size=(len(base), 256), dtype=np.uint8) < 32, axis=1)
            base = base ^ flips
        start += len(prev)
        parents.append(pids)
        descs.append(base)
    parent = np.concatenate(parents).astype(np.int32)
    desc = np.concatenate(descs)
    n = len(parent)
    is_leaf = np.zeros(n, np.uint8)
    is_leaf[n - k ** L:] = 1
    weight = np.zeros(n)
    weight[n - k ** L:] = rng.uniform(0.5, 8.0, k ** L)
    return dict(k=k, L=L, scoring=0, weighting=0, parent=parent, is_leaf=is_leaf, desc=desc, weight=weight)


def make_init_batch(seed: int = 0, n_pairs: int = 4, n1=4000, n2=4000, width: float = 1280.0, height: float = 720.0,
                    window: int = 100, nnratio: float = 0.9, check_orientation: bool = True, dup_frac: float = 0.25,
                    twin_frac: float = 0.15, dense: bool = False):
    """SearchForInitialization inputs (orbm_init_batch, host arrays) shaped like
    Tracking::MonocularInitialization (Tracking.cc:1050-1052: the initial extractor's 2x features,
    windowSize 100, ORBmatcher(0.9f, true)).

    F1 (initial frame): n1 keypoints over the image, octaves by the 2000-feature quotas, random
    descriptors, angles around a dominant value.  F2 (current frame): for 70 % of F1's keypoints a
    displaced copy (a common image motion + noise, 0-40 flipped bits, the same octave 75 % of the
    time), the rest random; a fraction `dup_frac` of F2's copies duplicate an F1 keypoint that already
    has one (several queries competing for one idx2, so later, closer queries take it from earlier
    ones), some with an exact descriptor copy (distance ties); `twin_frac` of F1's keypoints sit next
    to an earlier one with a similar descriptor (the later query takes the feature when it is closer).
    prevMatched = F1's positions.
    `dense`: a cluster of 300 octave-0 keypoints in a 150-px box puts more than PI_CAP candidates in
    the windows around it.  n1 / n2: int or per-pair list."""
    rng = np.random.default_rng(seed)
    n1s = [int(n1)] * n_pairs if np.isscalar(n1) else [int(v) for v in n1]
    n2s = [int(n2)] * n_pairs if np.isscalar(n2) else [int(v) for v in n2]
    q = np.array(ORB_QUOTA_2000, float)
    q /= q.sum()
    F = dict(kp_xy=[], kp_octave=[], kp_desc=[], kp_angle=[], bounds=[], q_octave=[], q_desc=[], q_angle=[],
             prev_matched=[])

    def flip(d, nbits):
        d = d.copy()
        for bit in rng.choice(256, size=nbits, replace=False):
            d[bit >> 3] ^= np.uint8(1 << (bit & 7))
        return d

    for p in range(n_pairs):
        a, b = n1s[p], n2s[p]
        x1 = rng.uniform(0, width, a)
        y1 = rng.uniform(0, height, a)
        o1 = rng.choice(8, size=a, p=q)
        if dense and a > 300:
            cx, cy = rng.uniform(200, width - 200), rng.uniform(200, height - 200)
            x1[:300] = cx + rng.uniform(-75, 75, 300)
            y1[:300] = cy + rng.uniform(-75, 75, 300)
            o1[:300] = 0
        d1 = rng.integers(0, 256, size=(a, 32), dtype=np.uint8)
        for i in range(1, a):   # twins: a later query near an earlier one with a similar descriptor
            if rng.random() < twin_frac:
                j = int(rng.integers(0, i))
                x1[i], y1[i], o1[i] = x1[j] + rng.normal(0, 2), y1[j] + rng.normal(0, 2), o1[j]
                d1[i] = flip(d1[j], int(rng.integers(0, 31)))
        rot = rng.uniform(0, 360)
        a1 = (rot + rng.normal(0, 20, a)) % 360
        mot = rng.normal(0, 15, 2)
        x2 = rng.uniform(0, width, b)
        y2 = rng.uniform(0, height, b)
        o2 = rng.choice(8, size=b, p=q)
        d2 = rng.integers(0, 256, size=(b, 32), dtype=np.uint8)
        a2 = rng.uniform(0, 360, b)
        used = []
        for k in range(b):
            if a == 0 or rng.random() >= 0.7:
                continue
            i = int(rng.choice(used)) if used and rng.random() < dup_frac else int(rng.integers(0, a))
            used.append(i)
            x2[k] = x1[i] + mot[0] + rng.normal(0, 3)
            y2[k] = y1[i] + mot[1] + rng.normal(0, 3)
            o2[k] = o1[i] if rng.random() < 0.75 else int(rng.integers(0, 8))
            d2[k] = flip(d1[i], int(rng.integers(0, 41)))
            if rng.random() < 0.08:
                d2[k] = d1[i].copy() if rng.random() < 0.5 else d2[int(rng.integers(0, b))].copy()
            a2[k] = (a1[i] + 25 + rng.normal(0, 8)) % 360
        F["kp_xy"].append(np.stack([x2, y2], 1).astype(np.float32))
        F["kp_octave"].append(o2.astype(np.int32))
        F["kp_desc"].append(d2)
        F["kp_angle"].append(np.clip(a2, 0, np.nextafter(np.float32(360), np.float32(0))).astype(np.float32))
        F["bounds"].append(np.array([0.0, width, 0.0, height], np.float32))
        F["q_octave"].append(o1.astype(np.int32))
        F["q_desc"].append(d1)
        F["q_angle"].append(np.clip(a1, 0, np.nextafter(np.float32(360), np.float32(0))).astype(np.float32))
        F["prev_matched"].append(np.stack([x1, y1], 1).astype(np.float32))
    shapes = dict(kp_xy=((0, 2), np.float32), kp_octave=((0,), np.int32), kp_desc=((0, 32), np.uint8),
                  kp_angle=((0,), np.float32), bounds=((0, 4), np.float32), q_octave=((0,), np.int32),
                  q_desc=((0, 32), np.uint8), q_angle=((0,), np.float32), prev_matched=((0, 2), np.float32))
    out = {}
    for k, (shape, dt) in shapes.items():
        v = F[k] if k != "bounds" else [x[None] for x in F[k]]
        out[k] = np.ascontiguousarray(np.concatenate(v).astype(dt) if v else np.zeros(shape, dt))
    out["kp_begin"] = np.concatenate([[0], np.cumsum(n2s)]).astype(np.int32)
    out["q_begin"] = np.concatenate([[0], np.cumsum(n1s)]).astype(np.int32)
    out.update(window=int(window), nnratio=float(nnratio), check_orientation=bool(check_orientation))
    return out


def make_reloc_batch(seed: int = 0, n_frames: int = 4, n_kp=2000, n_mp=600, th: float = 10.0, orb_dist: int = 100,
                     check_orientation: bool = True, dup_frac: float = 0.15, claimed_frac: float = 0.1):
    """SearchByProjection(Frame&, KeyFrame*, alreadyFound, th, ORBdist) inputs (orbm_reloc_batch, host arrays)
    shaped like Tracking::Relocalization (Tracking.cc:403,417: th 10 / ORBdist 100, then 3 / 64) on a
    KITTI camera.  Per frame: a pose (small rotation, a few metres of translation); the candidate
    keyframe's points in front of it (90 % valid), maxDistance_ = dist * 1.2^o * U(0.9, 1.1) for a random
    octave o and minDistance_ = maxDistance_ / 1.2^7 (MapPoint.cc:369-377), 5 % outside the invariance
    range; 70 % of the points observed by a keypoint near the projection (octave = the predicted scale
    +- 1 or off-window, 0-60 flipped bits), `dup_frac` of them sharing a keypoint with another point,
    plus random keypoints; `claimed_frac` of the keypoints already hold a map point.  Angles around a
    dominant rotation for CheckOrientation.  n_kp / n_mp: int or per-frame list."""
    rng = np.random.default_rng(seed)
    kps = [int(n_kp)] * n_frames if np.isscalar(n_kp) else [int(v) for v in n_kp]
    mps = [int(n_mp)] * n_frames if np.isscalar(n_mp) else [int(v) for v in n_mp]
    fx, fy, cx, cy = np.float32(KITTI["fx"]), np.float32(KITTI["fx"]), np.float32(607.1928), np.float32(185.2157)
    W, H = 1241.0, 376.0
    cum = np.ones(8, np.float32)
    for i in range(1, 8):
        cum[i] = np.float32(cum[i - 1] * np.float32(1.2))
    F = dict(kp_xy=[], kp_octave=[], kp_desc=[], kp_angle=[], kp_claimed=[], bounds=[], pose=[], camera=[],
             mp_valid=[], mp_xw=[], mp_max_min=[], mp_desc=[], mp_angle=[])
    for f in range(n_frames):
        n, m = kps[f], mps[f]
        Rcw = _small_rot(rng, 3.0).astype(np.float32)
        tcw = rng.normal(0, 2.0, 3).astype(np.float32)
        # points in the camera frame, then to the world: Xw = Rcw^T (Xc - tcw)
        z = rng.uniform(4, 40, m)
        u = rng.uniform(-20, W + 20, m)
        v = rng.uniform(-10, H + 10, m)
        Xc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
        Xw = ((Xc - tcw[None]) @ Rcw).astype(np.float32)
        Ow = -(Rcw.T @ tcw)
        dist = np.linalg.norm(Xw - Ow[None], axis=1)
        o = rng.integers(0, 8, m)
        maxd = dist * (1.2 ** o) * rng.uniform(0.9, 1.1, m)
        bad = rng.random(m) < 0.05
        maxd = np.where(bad, dist * rng.choice([0.5, 3.0], m), maxd)
        mind = maxd / cum[7]
        mdesc = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
        rot = rng.uniform(0, 360)
        mang = rng.uniform(0, 360, m)
        x = rng.uniform(0, W, n)
        y = rng.uniform(0, H, n)
        octv = rng.integers(0, 8, n)
        desc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        ang = rng.uniform(0, 360, n)
        used = []
        for j in range(m):
            if n == 0 or rng.random() >= 0.7:
                continue
            i = int(rng.choice(used)) if used and rng.random() < dup_frac else int(rng.integers(0, n))
            used.append(i)
            x[i] = u[j] + rng.normal(0, 1.5)
            y[i] = v[j] + rng.normal(0, 1.5)
            ratio = maxd[j] / max(dist[j], 1e-6)
            ps = int(min(7, max(0, np.ceil(np.log(ratio) / np.log(1.2)))))
            octv[i] = min(7, max(0, ps + int(rng.choice([-1, 0, 0, 1, 3]))))
            d = mdesc[j].copy()
            for bit in rng.choice(256, size=int(rng.integers(0, 61)), replace=False):
                d[bit >> 3] ^= np.uint8(1 << (bit & 7))
            desc[i] = d
            ang[i] = (mang[j] - rot + rng.normal(0, 6)) % 360
        F["kp_xy"].append(np.stack([x, y], 1).astype(np.float32))
        F["kp_octave"].append(octv.astype(np.int32))
        F["kp_desc"].append(desc)
        F["kp_angle"].append(np.minimum(ang, 359.99).astype(np.float32))
        F["kp_claimed"].append((rng.random(n) < claimed_frac).astype(np.uint8))
        F["bounds"].append(np.array([[0.0, W, 0.0, H]], np.float32))
        F["pose"].append(np.concatenate([Rcw.reshape(-1), tcw])[None].astype(np.float32))
        F["camera"].append(np.array([[fx, fy, cx, cy]], np.float32))
        F["mp_valid"].append((rng.random(m) < 0.9).astype(np.uint8))
        F["mp_xw"].append(Xw)
        F["mp_max_min"].append(np.stack([maxd, mind], 1).astype(np.float32))
        F["mp_desc"].append(mdesc)
        F["mp_angle"].append(np.minimum(mang, 359.99).astype(np.float32))
    shapes = dict(kp_xy=(0, 2), kp_octave=(0,), kp_desc=(0, 32), kp_angle=(0,), kp_claimed=(0,), bounds=(0, 4),
                  pose=(0, 12), camera=(0, 4), mp_valid=(0,), mp_xw=(0, 3), mp_max_min=(0, 2), mp_desc=(0, 32),
                  mp_angle=(0,))
    out = {}
    for k, shape in shapes.items():
        dt = np.uint8 if k in ("kp_desc", "mp_desc", "kp_claimed", "mp_valid") else (np.int32 if k == "kp_octave" else np.float32)
        out[k] = np.ascontiguousarray(np.concatenate(F[k]).astype(dt) if F[k] else np.zeros(shape, dt))
    out["kp_begin"] = np.concatenate([[0], np.cumsum(kps)]).astype(np.int32)
    out["mp_begin"] = np.concatenate([[0], np.cumsum(mps)]).astype(np.int32)
    out.update(scale_factors=cum, log_scale_factor=float(np.float32(np.log(np.float64(np.float32(1.2))))), th=float(th),
               orb_dist=int(orb_dist), check_orientation=bool(check_orientation))
    return out


def make_fuse_batch(seed: int = 0, n_items: int = 4, n_kp=2000, n_mp=1500, th: float = 3.0, chi2_gate: bool = True,
                    dup_frac: float = 0.0, claimed_frac: float = 0.0):
    """ORBmatcher::Fuse / Sim3 SearchByProjection inputs (orbm_fuse_batch, host arrays, plus kp_claimed for
    the Sim3 search) shaped like LocalMapping::SearchInNeighbors (LocalMapping.cc:606,624: th 3) and
    LoopClosing (th 4 / 10) on the KITTI stereo camera.  Per item a keyframe pose (small rotation, a few
    metres of translation) and n_mp candidate points (90 % valid):
      2 % behind the camera, ~4 % projecting outside the image, 2.5 % outside the invariance range
      (maxDistance_ = dist / 2 or dist * 6; else dist * 1.2^o * U(0.9, 1.1), minDistance_ = max / 1.2^7),
      normals 0-50 deg off the viewing ray (94 %), 65-120 deg (3 %) or around the 60 deg gate (3 %);
      ~70 % observed by a keypoint near the projection: octave = predicted scale + {-1, 0, 0, 1, 3}, 0-70
      flipped bits (92 % up to 45, the rest above: some best distances exceed TH_LOW), pixel noise
      N(0, s * 1.2^octave) with s = 0.8 (92 %) or 2.5 so the chi2 gates pass and fail at every octave,
      half stereo (uright near u - bf / z, also noisy) and half uright = -1; 3 % of the stereo ones have
      uright = 0 exactly (still stereo: the gate is uright >= 0);
      8 % of the observed points get a second keypoint with the identical descriptor in another grid cell
      of the window, the one earlier in scan order holding the higher index (a tie index order would
      decide the other way);
      `dup_frac` of the points copy an earlier observed point (position, a descriptor 0-10 bits away) and
      compete for its keypoint (the Sim3 search's claims).
    The other keypoints are random (half stereo); `claimed_frac` of all keypoints hold a match on entry.
    n_kp / n_mp: int or per-item list."""
    rng = np.random.default_rng(seed)
    kps = [int(n_kp)] * n_items if np.isscalar(n_kp) else [int(v) for v in n_kp]
    mps = [int(n_mp)] * n_items if np.isscalar(n_mp) else [int(v) for v in n_mp]
    fx, fy, cx, cy = np.float32(KITTI["fx"]), np.float32(KITTI["fy"]), np.float32(KITTI["cx"]), np.float32(KITTI["cy"])
    bf = np.float32(KITTI["bf"])
    W, H = np.float32(KITTI["width"]), np.float32(KITTI["height"])
    cum = np.ones(8, np.float32)
    for i in range(1, 8):
        cum[i] = np.float32(cum[i - 1] * np.float32(1.2))
    invW, invH = np.float32(64) / W, np.float32(48) / H

    def cell(px, py):   # FeaturesGrid::AssignFeatures' cell of a keypoint
        return (int(np.round(float(invW * np.float32(px)))), int(np.round(float(invH * np.float32(py)))))

    def flip(d, nbits):
        d = d.copy()
        for bit in rng.choice(256, size=nbits, replace=False):
            d[bit >> 3] ^= np.uint8(1 << (bit & 7))
        return d

    F = dict(kp_xy=[], kp_octave=[], kp_uright=[], kp_desc=[], kp_claimed=[], bounds=[], pose=[], camera=[],
             mp_valid=[], mp_xw=[], mp_max_min=[], mp_normal=[], mp_desc=[])
    for f in range(n_items):
        n, m = kps[f], mps[f]
        Rcw = _small_rot(rng, 3.0).astype(np.float32)
        tcw = rng.normal(0, 2.0, 3).astype(np.float32)
        z = rng.uniform(4, 40, m)
        z = np.where(rng.random(m) < 0.02, -rng.uniform(2, 30, m), z)
        u = rng.uniform(-10, float(W) + 10, m)
        v = rng.uniform(-4, float(H) + 4, m)
        o = rng.integers(0, 8, m)
        mscale = (1.2 ** o) * rng.uniform(0.9, 1.1, m)
        mscale = np.where(rng.random(m) < 0.025, rng.choice([0.5, 6.0], m), mscale)
        mdesc = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
        observed = rng.random(m) < 0.72
        src = np.full(m, -1)
        for j in range(1, m):   # copies of an earlier observed point
            if rng.random() < dup_frac:
                cand = np.nonzero(observed[:j] & (src[:j] < 0))[0]
                if len(cand):
                    j0 = int(rng.choice(cand))
                    src[j], observed[j] = j0, False
                    z[j], u[j], v[j], mscale[j] = z[j0], u[j0] + rng.normal(0, 0.3), v[j0] + rng.normal(0, 0.3), mscale[j0]
                    mdesc[j] = flip(mdesc[j0], int(rng.integers(0, 11)))
        Xc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
        Xw = ((Xc - tcw[None]) @ Rcw).astype(np.float32)   # Xw = Rcw^T (Xc - tcw)
        Ow = -(Rcw.T @ tcw)
        PO = Xw - Ow[None]
        dist = np.linalg.norm(PO, axis=1)
        maxd = dist * mscale
        mind = maxd / cum[7]
        # normals: the viewing ray turned by ang about a random axis perpendicular to it
        ray = PO / np.maximum(dist, 1e-9)[:, None]
        kind = rng.random(m)
        ang = np.deg2rad(np.where(kind < 0.94, rng.uniform(0, 50, m),
                                  np.where(kind < 0.97, rng.uniform(65, 120, m), rng.uniform(58, 62, m))))
        perp = np.cross(ray, rng.normal(0, 1, (m, 3)))
        perp /= np.maximum(np.linalg.norm(perp, axis=1), 1e-9)[:, None]
        normal = np.cos(ang)[:, None] * ray + np.sin(ang)[:, None] * perp
        for j in range(m):
            if src[j] >= 0:
                normal[j] = normal[src[j]]
        # keypoints: random ones, then the planted observations in free slots
        x = rng.uniform(0, float(W), n)
        y = rng.uniform(0, float(H), n)
        octv = rng.integers(0, 8, n)
        desc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        uright = np.where(rng.random(n) < 0.5, x - rng.uniform(5, 100, n), -1.0)
        free = list(rng.permutation(n))
        for j in range(m):
            if not observed[j] or not free:
                continue
            i = int(free.pop())
            ps = int(min(7, max(0, np.ceil(np.log(max(mscale[j], 1e-9)) / np.log(1.2)))))
            oc = min(7, max(0, ps + int(rng.choice([-1, 0, 0, 1, 3]))))
            s = (0.8 if rng.random() < 0.92 else 2.5) * 1.2 ** oc
            x[i], y[i], octv[i] = u[j] + rng.normal(0, s), v[j] + rng.normal(0, s), oc
            desc[i] = flip(mdesc[j], int(rng.integers(0, 46) if rng.random() < 0.92 else rng.integers(46, 71)))
            if rng.random() < 0.5:
                uright[i] = 0.0 if rng.random() < 0.03 else max(u[j] - float(bf) / max(z[j], 1e-3) + rng.normal(0, s), 0.0)
            else:
                uright[i] = -1.0
            if rng.random() < 0.08 and free:   # an identical descriptor in another cell of the window
                rad = 0.6 * th * 1.2 ** max(min(oc, ps), 0)
                for _ in range(20):
                    xb, yb = x[i] + rng.uniform(-rad, rad), y[i] + rng.uniform(-rad, rad)
                    if cell(xb, yb) != cell(x[i], y[i]) and 0 <= xb < float(W) and 0 <= yb < float(H):
                        k = int(free.pop())
                        x[k], y[k], octv[k], desc[k], uright[k] = xb, yb, oc, desc[i], uright[i]
                        if uright[i] > 0:
                            uright[k] = max(uright[i] + (xb - x[i]), 0.0)
                        first, second = (i, k) if cell(x[i], y[i]) < cell(xb, yb) else (k, i)
                        if first < second:   # the scan-first keypoint takes the higher index
                            for arr in (x, y, uright):
                                arr[first], arr[second] = arr[second], arr[first]
                        break
        F["kp_xy"].append(np.stack([x, y], 1).astype(np.float32))
        F["kp_octave"].append(octv.astype(np.int32))
        F["kp_uright"].append(uright.astype(np.float32))
        F["kp_desc"].append(desc)
        F["kp_claimed"].append((rng.random(n) < claimed_frac).astype(np.uint8))
        F["bounds"].append(np.array([[0.0, W, 0.0, H]], np.float32))
        F["pose"].append(np.concatenate([Rcw.reshape(-1), tcw])[None].astype(np.float32))
        F["camera"].append(np.array([[fx, fy, cx, cy, bf]], np.float32))
        F["mp_valid"].append((rng.random(m) < 0.9).astype(np.uint8))
        F["mp_xw"].append(Xw)
        F["mp_max_min"].append(np.stack([maxd, mind], 1).astype(np.float32))
        F["mp_normal"].append(normal.astype(np.float32))
        F["mp_desc"].append(mdesc)
    shapes = dict(kp_xy=(0, 2), kp_octave=(0,), kp_uright=(0,), kp_desc=(0, 32), kp_claimed=(0,), bounds=(0, 4),
                  pose=(0, 12), camera=(0, 5), mp_valid=(0,), mp_xw=(0, 3), mp_max_min=(0, 2), mp_normal=(0, 3),
                  mp_desc=(0, 32))
    out = {}
    for k, shape in shapes.items():
        dt = np.uint8 if k in ("kp_desc", "mp_desc", "kp_claimed", "mp_valid") else (np.int32 if k == "kp_octave" else np.float32)
        out[k] = np.ascontiguousarray(np.concatenate(F[k]).astype(dt) if F[k] else np.zeros(shape, dt))
    out["kp_begin"] = np.concatenate([[0], np.cumsum(kps)]).astype(np.int32)
    out["mp_begin"] = np.concatenate([[0], np.cumsum(mps)]).astype(np.int32)
    out.update(scale_factors=cum, inv_sigma2=(np.float32(1) / (cum * cum)).astype(np.float32),
               log_scale_factor=float(np.float32(np.log(np.float64(np.float32(1.2))))), th=float(th),
               chi2_gate=bool(chi2_gate))
    return out


def make_sim3_batch(seed: int = 0, n_pairs: int = 4, n_kp1=2000, n_kp2=2000, th: float = 7.5, scale=None):
    """ORBmatcher::SearchBySim3 inputs (orbm_sim3_batch, host arrays) shaped like
    LoopClosing::FindLoopInCandidateKFs (LoopClosing.cc:137, th 7.5) on the KITTI camera.  Per pair two
    keyframes with their own poses in two maps related by S12 (a few degrees, ~0.5 m, s = `scale`, or drawn
    from U(0.7, 0.95) / U(1.05, 1.4) when None: never 1), and a shared 3-D structure of min(n_kp1, n_kp2)
    / 2 points defined in camera 2 (z in 4..40 m, projections up to 10 px outside the image; 2 % behind the
    camera).  Every shared point holds a slot in both keyframes:
      the keypoint sits at the point's projection plus N(0, 1.2^octave) px of jitter (well under the
      radius th * 1.2^scale), octave = the scale predicted from the other side + {0, 0, 0, 0, -1, -1, 1, -2} (the
      last two fall outside the level window), its descriptor 0-40 bits off the shared one (90 %) or
      90-130 bits (best distances above TH_HIGH);
      the map point has maxDistance_ = dist * 1.2^o * U(0.9, 1.1) (3 %: dist / 2 or dist * 6, outside the
      invariance range), a descriptor 0-6 bits off the shared one, and is valid with probability 0.85
      (the rest: no map point, or matched on entry);
      6 % get a keypoint with the identical descriptor in another grid cell of the window of the other
      keyframe, the one earlier in scan order holding the higher index (a tie index order would decide
      the other way); 6 % get a decoy in keyframe 1 closer to keyframe 2's map point descriptor than the
      true keypoint (a 1 -> 2 match without its 2 -> 1 partner); 6 % a keypoint with the identical
      descriptor just outside the radius.
    The other slots are random keypoints, half of them holding a random map point in front of the camera.
    n_kp1 / n_kp2: int or per-pair list."""
    rng = np.random.default_rng(seed)
    kps = [[int(n)] * n_pairs if np.isscalar(n) else [int(v) for v in n] for n in (n_kp1, n_kp2)]
    fx, fy, cx, cy = (float(np.float32(KITTI[k])) for k in ("fx", "fy", "cx", "cy"))
    W, H = float(KITTI["width"]), float(KITTI["height"])
    cum = np.ones(8, np.float32)
    for i in range(1, 8):
        cum[i] = np.float32(cum[i - 1] * np.float32(1.2))
    invW, invH = np.float32(64) / np.float32(W), np.float32(48) / np.float32(H)

    def cell(px, py):   # FeaturesGrid::AssignFeatures' cell of a keypoint
        return (int(np.round(float(invW * np.float32(px)))), int(np.round(float(invH * np.float32(py)))))

    def flip(d, nbits):
        d = d.copy()
        for bit in rng.choice(256, size=int(nbits), replace=False):
            d[bit >> 3] ^= np.uint8(1 << (bit & 7))
        return d

    def proj(X):
        return fx * X[0] / X[2] + cx, fy * X[1] / X[2] + cy

    names = ("xy", "octave", "desc", "valid", "xw", "max_min", "mdesc")
    out = {f"{k}{s}": [] for s in "12" for k in names + ("bounds", "pose", "camera")}
    out["s12"] = []
    for p in range(n_pairs):
        n = [kps[0][p], kps[1][p]]
        R = [_small_rot(rng, 3.0), _small_rot(rng, 3.0)]
        t = [rng.normal(0, 2.0, 3), rng.normal(0, 2.0, 3)]
        R12, t12 = _small_rot(rng, 3.0), rng.normal(0, 0.5, 3)
        s12 = float(scale) if scale is not None else float(rng.uniform(0.7, 0.95) if rng.random() < 0.5 else rng.uniform(1.05, 1.4))
        side = []
        for s in range(2):   # random keypoints; half of the slots hold a random map point
            m = n[s]
            z = rng.uniform(4, 40, m)
            Xc = np.stack([(rng.uniform(0, W, m) - cx) * z / fx, (rng.uniform(0, H, m) - cy) * z / fy, z], 1)
            dist = np.linalg.norm(Xc, axis=1)
            maxd = dist * 1.2 ** rng.integers(0, 8, m) * rng.uniform(0.9, 1.1, m)
            side.append(dict(x=rng.uniform(0, W, m), y=rng.uniform(0, H, m), oct=rng.integers(0, 8, m),
                             desc=rng.integers(0, 256, size=(m, 32), dtype=np.uint8), valid=(rng.random(m) < 0.5).astype(np.uint8),
                             xw=(Xc - t[s][None]) @ R[s], maxd=maxd, mdesc=rng.integers(0, 256, size=(m, 32), dtype=np.uint8),
                             free=list(rng.permutation(m))))
        for _ in range(min(n) // 2):
            z = float(rng.uniform(4, 40)) * (-1.0 if rng.random() < 0.02 else 1.0)
            Xc2 = np.array([(rng.uniform(-10, W + 10) - cx) * z / fx, (rng.uniform(-4, H + 4) - cy) * z / fy, z])
            Xc = [s12 * (R12 @ Xc2) + t12, Xc2]   # the point in camera 1 and in camera 2
            D = rng.integers(0, 256, size=32, dtype=np.uint8)
            slot = [int(side[s]["free"].pop()) for s in range(2)]
            o = [int(rng.integers(0, 7)), int(rng.integers(0, 7))]
            for s in range(2):   # the map point of side s is searched in the other keyframe, at distance |Xc[1 - s]|
                S, i = side[s], slot[s]
                far = float(np.linalg.norm(Xc[1 - s]))
                kind = rng.random()
                mscale = 1.2 ** o[s] * rng.uniform(0.9, 1.1) if kind >= 0.03 else (0.5 if kind < 0.015 else 6.0)
                S["xw"][i] = R[s].T @ (Xc[s] - t[s])
                S["maxd"][i] = far * mscale
                S["mdesc"][i] = flip(D, rng.integers(0, 7))
                S["valid"][i] = 1 if rng.random() < 0.85 else 0
            for s in range(2):   # the keypoint of side s is what the other side's map point should find
                S, i = side[s], slot[s]
                if Xc[s][2] <= 0.1:
                    continue
                u, v = proj(Xc[s])
                ps = int(min(7, max(0, np.ceil(np.log(max(side[1 - s]["maxd"][slot[1 - s]] / np.linalg.norm(Xc[s]), 1e-9)) / np.log(1.2)))))
                oc = min(7, max(0, ps + int(rng.choice([0, 0, 0, 0, -1, -1, 1, -2]))))
                S["x"][i], S["y"][i], S["oct"][i] = u + rng.normal(0, 1.2 ** oc), v + rng.normal(0, 1.2 ** oc), oc
                S["desc"][i] = flip(D, rng.integers(0, 41) if rng.random() < 0.9 else rng.integers(90, 131))
                rad = th * 1.2 ** ps
                extra = rng.random()
                if extra < 0.06 and S["free"]:   # an identical descriptor in another cell of the window
                    for _try in range(20):
                        xb, yb = S["x"][i] + rng.uniform(-0.5, 0.5) * rad, S["y"][i] + rng.uniform(-0.5, 0.5) * rad
                        if cell(xb, yb) != cell(S["x"][i], S["y"][i]) and 0 <= xb < W and 0 <= yb < H:
                            k = int(S["free"].pop())
                            S["x"][k], S["y"][k], S["oct"][k], S["desc"][k] = xb, yb, oc, S["desc"][i]
                            first, second = (i, k) if cell(S["x"][i], S["y"][i]) < cell(xb, yb) else (k, i)
                            if first < second:   # the scan-first keypoint takes the higher index
                                for arr in (S["x"], S["y"]):
                                    arr[first], arr[second] = arr[second], arr[first]
                            break
                elif extra < 0.12 and s == 0 and S["free"]:   # a decoy for the 2 -> 1 search
                    k = int(S["free"].pop())
                    S["x"][k], S["y"][k], S["oct"][k] = u + rng.normal(0, 1.0), v + rng.normal(0, 1.0), max(0, min(ps, 7))
                    S["desc"][k] = side[1]["mdesc"][slot[1]]
                elif extra < 0.18 and S["free"]:   # the identical descriptor just outside the radius
                    k = int(S["free"].pop())
                    S["x"][k], S["y"][k], S["oct"][k], S["desc"][k] = u + rad * 1.05 + 1.0, v, oc, S["desc"][i]
        for s, tag in enumerate("12"):
            S = side[s]
            out["xy" + tag].append(np.stack([S["x"], S["y"]], 1).astype(np.float32).reshape(-1, 2))
            out["octave" + tag].append(S["oct"].astype(np.int32))
            out["desc" + tag].append(S["desc"])
            out["valid" + tag].append(S["valid"])
            out["xw" + tag].append(S["xw"].astype(np.float32).reshape(-1, 3))
            out["max_min" + tag].append(np.stack([S["maxd"], S["maxd"] / float(cum[7])], 1).astype(np.float32).reshape(-1, 2))
            out["mdesc" + tag].append(S["mdesc"])
            out["bounds" + tag].append(np.array([[0.0, W, 0.0, H]], np.float32))
            out["pose" + tag].append(np.concatenate([R[s].reshape(-1), t[s]])[None].astype(np.float32))
            out["camera" + tag].append(np.array([[fx, fy, cx, cy]], np.float32))
        out["s12"].append(np.concatenate([R12.reshape(-1), t12, [s12]])[None].astype(np.float32))
    cat = lambda xs, shape, dt: np.ascontiguousarray(np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt))   # noqa: E731
    b = {"s12": cat(out["s12"], (0, 13), np.float32)}
    for s, tag in enumerate("12"):
        b[f"kp{tag}_begin"] = np.concatenate([[0], np.cumsum(kps[s])]).astype(np.int32)
        b[f"kp{tag}_xy"] = cat(out["xy" + tag], (0, 2), np.float32)
        b[f"kp{tag}_octave"] = cat(out["octave" + tag], (0,), np.int32)
        b[f"kp{tag}_desc"] = cat(out["desc" + tag], (0, 32), np.uint8)
        b[f"mp{tag}_valid"] = cat(out["valid" + tag], (0,), np.uint8)
        b[f"mp{tag}_xw"] = cat(out["xw" + tag], (0, 3), np.float32)
        b[f"mp{tag}_max_min"] = cat(out["max_min" + tag], (0, 2), np.float32)
        b[f"mp{tag}_desc"] = cat(out["mdesc" + tag], (0, 32), np.uint8)
        for k, w in (("bounds", 4), ("pose", 12), ("camera", 4)):
            b[k + tag] = cat(out[k + tag], (0, w), np.float32)
    b.update(scale_factors=cum, log_scale_factor=float(np.float32(np.log(np.float64(np.float32(1.2))))), th=float(th))
    return b


def make_observation_sets(seed: int = 0, n_points: int = 1500, n_obs=8):
    """MapPoint::ComputeDistinctiveDescriptors inputs: point p holds n_obs (int, or one count per point)
    descriptor rows, each the point's own random descriptor with every bit flipped with a per-row
    probability from U(0, 0.2) (observations of one point from different views); one row in eight repeats
    an earlier row of its point, so equal medians (decided by the lower row) occur.  Returns
    {"desc": [total, 32] uint8, "begin": [n_points + 1] int32}."""
    rng = np.random.default_rng(seed)
    counts = np.full(n_points, int(n_obs), np.int64) if np.isscalar(n_obs) else np.asarray(n_obs, np.int64)
    assert len(counts) == n_points
    rows = []
    for c in counts:
        c = int(c)
        base = rng.integers(0, 256, size=32, dtype=np.uint8)
        mask = rng.random((c, 256)) < rng.uniform(0, 0.2, c)[:, None]
        d = base[None] ^ np.packbits(mask, axis=1, bitorder="little")
        for i in range(1, c):
            if rng.random() < 0.125:
                d[i] = d[int(rng.integers(0, i))]
        rows.append(d.astype(np.uint8).reshape(c, 32))
    desc = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 32), np.uint8))
    return {"desc": desc, "begin": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)}


def make_optsim3_batch(seed: int = 0, n_corr=(150,), n_outliers=0, noise: bool = True, rot_deg: float = 1.0,
                       trans: float = 0.03, dscale: float = 0.02, extras: int = 3, max_chi2: float = 10.0,
                       fix_scale: bool = False, cam=KITTI):
    """A batch of Optimizer::OptimizeSim3 problems in the orbba_sim3_batch layout (loop candidates).

    Pair p has n_corr[p] correspondences.  The ground truth S12 (rotation N(0, 3 deg), |t| ~ 0.3, s in
    U(0.8, 1.25), or 1 with fix_scale) takes camera-2 coordinates to camera-1 coordinates.  Points are
    back-projected from uniform pixels of camera 1 at depth U(4, 40) and kept when they also lie in front of
    camera 2 (depth > 1); both keyframes have random world poses, and the world positions, measurements and
    intrinsics are rounded to float32, as the reference stores them.  Octaves U{0..7}, pixel noise
    N(0, 1.2^oct) per axis on both measurements (`noise`), inv_level_sigma2 = 1 / 1.2^(2 level) in float.
    n_outliers (int or per-pair list): that many correspondences of the pair get +-U(15, 40) px on both
    axes of the keyframe-2 measurement, as the C4 generator's gross outliers.  The start s12 is the truth
    perturbed by N(0, rot_deg) rotation, N(0, trans) translation and a factor 1 + N(0, dscale) (none with
    fix_scale).  Keyframe 2's slots are a random permutation, and each keyframe carries `extras` slots of
    each kind the keep test must drop: no map point in keyframe 1, no match, a match whose map point in
    keyframe 2 is bad.  Returns the batch plus gt_s12 (F, 13), outlier (total_kp1, bool) and n_corr."""
    rng = np.random.default_rng(seed)
    counts = [int(n) for n in np.atleast_1d(n_corr)]
    F = len(counts)
    n_out = [int(n_outliers)] * F if np.isscalar(n_outliers) else [int(n) for n in n_outliers]
    camv = np.array([cam[k] for k in ("fx", "fy", "cx", "cy")], np.float32)
    fx, fy, cx, cy = camv.astype(np.float64)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)   # noqa: E731
    kp1_begin, kp2_begin = [0], [0]
    col = {k: [] for k in ("kp1_xy", "kp1_octave", "kp2_xy", "kp2_octave", "mp1_valid", "mp1_xw", "mp2_valid", "mp2_xw",
                           "match12", "outlier")}
    pose1, pose2, s12, gt = [], [], [], []
    for p, n in enumerate(counts):
        R12 = _small_rot(rng, 3.0)
        t12 = rng.normal(0, 0.2, 3)
        sc = 1.0 if fix_scale else rng.uniform(0.8, 1.25)
        Xc1 = np.zeros((0, 3))
        while len(Xc1) < n:   # points in front of both cameras
            m = 2 * (n - len(Xc1)) + 8
            u, v, z = rng.uniform(0, cam["width"], m), rng.uniform(0, cam["height"], m), rng.uniform(4, 40, m)
            X = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
            X2 = (X - t12) @ R12 / sc
            Xc1 = np.concatenate([Xc1, X[X2[:, 2] > 1.0]])
        Xc1 = Xc1[:n]
        Xc2 = (Xc1 - t12) @ R12 / sc   # S12^-1: R^T (x - t) / s
        poses = []
        for _ in range(2):
            Rcw = _rot_y(rng.uniform(-180, 180)) @ _small_rot(rng, 3.0)
            tcw = -Rcw @ np.array([rng.uniform(-50, 50), rng.uniform(-2, 2), rng.uniform(-50, 50)])
            poses.append((Rcw, tcw))
        Xw1 = (Xc1 - poses[0][1]) @ poses[0][0]
        Xw2 = (Xc2 - poses[1][1]) @ poses[1][0]
        oct1, oct2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
        z1 = np.stack([Xc1[:, 0] / Xc1[:, 2] * fx + cx, Xc1[:, 1] / Xc1[:, 2] * fy + cy], 1)
        z2 = np.stack([Xc2[:, 0] / Xc2[:, 2] * fx + cx, Xc2[:, 1] / Xc2[:, 2] * fy + cy], 1)
        if noise:
            z1 = z1 + rng.normal(0, 1, (n, 2)) * (1.2 ** oct1)[:, None]
            z2 = z2 + rng.normal(0, 1, (n, 2)) * (1.2 ** oct2)[:, None]
        out = np.zeros(n, bool)
        out[rng.permutation(n)[:n_out[p]]] = True
        z2 = z2 + out[:, None] * rng.choice([-1, 1], (n, 2)) * rng.uniform(15, 40, (n, 2))
        # keyframe 1: the n correspondences and 3 x extras dropped slots, shuffled; keyframe 2: permuted
        e = extras
        n1, n2 = n + 3 * e, n + 2 * e
        order1, perm2 = rng.permutation(n1), rng.permutation(n2)
        xy1 = np.concatenate([z1, rng.uniform(0, 300, (3 * e, 2))])
        xw1 = np.concatenate([Xw1, rng.uniform(-5, 5, (3 * e, 3))])
        o1 = np.concatenate([oct1, rng.integers(0, 8, 3 * e)])
        val1 = np.concatenate([np.ones(n, bool), np.zeros(e, bool), np.ones(2 * e, bool)])
        # slot of keyframe 2 before its permutation: i for the correspondences, a valid extra for the "no map
        # point in keyframe 1" kind, -1, and a bad map point of keyframe 2
        m12 = np.concatenate([np.arange(n), n + np.arange(e), -np.ones(e, int), n + e + np.arange(e)]).astype(int)
        xy2 = np.concatenate([z2, rng.uniform(0, 300, (2 * e, 2))])
        xw2 = np.concatenate([Xw2, rng.uniform(-5, 5, (2 * e, 3))])
        o2 = np.concatenate([oct2, rng.integers(0, 8, 2 * e)])
        val2 = np.concatenate([np.ones(n + e, bool), np.zeros(e, bool)])
        inv2 = np.empty(n2, int)
        inv2[perm2] = np.arange(n2)   # row r of keyframe 2 before the permutation sits at inv2[r]
        m12 = np.where(m12 >= 0, inv2[np.maximum(m12, 0)], -1)
        col["kp1_xy"].append(xy1[order1]); col["kp1_octave"].append(o1[order1]); col["mp1_valid"].append(val1[order1])
        col["mp1_xw"].append(xw1[order1]); col["match12"].append(m12[order1])
        col["outlier"].append(np.concatenate([out, np.zeros(3 * e, bool)])[order1])
        col["kp2_xy"].append(xy2[perm2]); col["kp2_octave"].append(o2[perm2]); col["mp2_valid"].append(val2[perm2])
        col["mp2_xw"].append(xw2[perm2])
        kp1_begin.append(kp1_begin[-1] + n1)
        kp2_begin.append(kp2_begin[-1] + n2)
        pose1.append(np.concatenate([poses[0][0].reshape(-1), poses[0][1]]))
        pose2.append(np.concatenate([poses[1][0].reshape(-1), poses[1][1]]))
        gt.append(np.concatenate([R12.reshape(-1), t12, [sc]]))
        R0 = _small_rot(rng, rot_deg) @ R12
        t0 = t12 + rng.normal(0, trans, 3)
        s0 = sc if fix_scale else sc * (1 + rng.normal(0, dscale))
        s12.append(np.concatenate([R0.reshape(-1), t0, [s0]]))
    cat = lambda k, w, dt: (np.concatenate(col[k]) if col[k] else np.zeros(0)).reshape((-1, w) if w > 1 else (-1,)).astype(dt)   # noqa: E731
    levels = np.arange(8)
    return dict(kp1_begin=np.array(kp1_begin, np.int32), kp2_begin=np.array(kp2_begin, np.int32),
                kp1_xy=cat("kp1_xy", 2, np.float32), kp1_octave=cat("kp1_octave", 1, np.int32),
                kp2_xy=cat("kp2_xy", 2, np.float32), kp2_octave=cat("kp2_octave", 1, np.int32),
                pose1=f32(pose1).reshape(F, 12), camera1=np.tile(camv, (F, 1)),
                pose2=f32(pose2).reshape(F, 12), camera2=np.tile(camv, (F, 1)),
                mp1_valid=cat("mp1_valid", 1, np.uint8), mp1_xw=cat("mp1_xw", 3, np.float32),
                mp2_valid=cat("mp2_valid", 1, np.uint8), mp2_xw=cat("mp2_xw", 3, np.float32),
                s12=f32(s12).reshape(F, 13), match12=cat("match12", 1, np.int32),
                inv_level_sigma2=(1.0 / (1.2 ** levels) ** 2).astype(np.float32), max_chi2=float(max_chi2),
                fix_scale=int(bool(fix_scale)), gt_s12=np.array(gt).reshape(F, 13), outlier=cat("outlier", 1, bool),
                n_corr=np.array(counts, np.int32))


def make_sim3solver_batch(seed: int = 0, n_corr=(150,), outlier_frac=0.2, noise_px: float = 0.3, fix_scale: bool = False,
                          max_iterations: int = 300, maxk: int = 300, min_inliers: int = 20, probability: float = 0.99,
                          extras: int = 3, cam=KITTI):
    """A batch of Sim3Solver problems in the orb_sim3solver_batch layout (loop candidates after SearchByBoW).

    make_optsim3_batch's noise-free geometry (ground truth S12, two world poses, shuffled slots and the
    `extras` slots the keep test must drop), with the error where the solver reads it: the solver never looks at
    the keypoints, it projects the matched map points, so keyframe 2's map points are moved in its camera frame,
    parallel to the image plane, by what shifts their projection by N(0, noise_px) pixels per axis, and a fraction
    outlier_frac (scalar or per pair) of the correspondences by +-U(30, 80) pixels per axis instead.  Adds
    level_sigma2 = 1.2^(2 level) in float, draws (make_draws with the same seed) and the RANSAC parameters.  Returns
    the batch plus gt_s12, outlier (total_kp1, bool) and n_corr."""
    from .sim3solver import make_draws
    b = make_optsim3_batch(seed, n_corr=n_corr, n_outliers=0, noise=False, extras=extras, fix_scale=fix_scale, cam=cam)
    rng = np.random.default_rng([seed, 77])
    F = len(b["kp1_begin"]) - 1
    frac = [float(outlier_frac)] * F if np.isscalar(outlier_frac) else [float(f) for f in outlier_frac]
    xw2 = b["mp2_xw"].astype(np.float64)
    outlier = np.zeros(len(b["match12"]), bool)
    for p in range(F):
        k1, k1e, k2 = int(b["kp1_begin"][p]), int(b["kp1_begin"][p + 1]), int(b["kp2_begin"][p])
        m = b["match12"][k1:k1e]
        keep = np.nonzero((b["mp1_valid"][k1:k1e] != 0) & (m >= 0) & (b["mp2_valid"][k2 + np.maximum(m, 0)] != 0))[0]
        n = len(keep)
        out = np.zeros(n, bool)
        out[rng.permutation(n)[:int(round(frac[p] * n))]] = True
        px = np.where(out[:, None], rng.choice([-1, 1], (n, 2)) * rng.uniform(30, 80, (n, 2)), rng.normal(0, noise_px, (n, 2)))
        R2, t2 = b["pose2"][p][:9].reshape(3, 3).astype(np.float64), b["pose2"][p][9:].astype(np.float64)
        rows = k2 + m[keep]
        Xc = xw2[rows] @ R2.T + t2
        dXc = np.stack([px[:, 0] * Xc[:, 2] / cam["fx"], px[:, 1] * Xc[:, 2] / cam["fy"], np.zeros(n)], 1)
        xw2[rows] = xw2[rows] + dXc @ R2
        outlier[k1 + keep] = out
    for k in ("s12", "inv_level_sigma2", "max_chi2"):
        del b[k]
    b.update(mp2_xw=xw2.astype(np.float32), outlier=outlier, level_sigma2=((1.2 ** np.arange(8)) ** 2).astype(np.float32),
             draws=np.ascontiguousarray(make_draws(F, max(max_iterations, 300), seed)[:, :max_iterations]), rand_max=2147483647, probability=float(probability),
             min_inliers=int(min_inliers), max_iterations=int(max_iterations), maxk=int(maxk), fix_scale=int(bool(fix_scale)))
    return b


def make_pnp_batch(seed: int = 0, n_corr=(150,), outlier_frac=0.2, noise_px: float = 0.3, extras_frac: float = 0.25,
                   n_draws: int = 300, probability: float = 0.99, min_inliers: int = 10, max_iterations: int = 300,
                   epsilon: float = 0.5, th2: float = 5.991, maxk: int = 5, cam=KITTI):
    """A batch of PnPsolver problems in the orb_pnpsolver_batch layout (relocalisation candidates after SearchByBoW).

    Per candidate a ground-truth Tcw (a rotation of up to 20 degrees about a random axis, a translation of a few
    metres) and n_corr[p] map points seen at a uniform pixel with a depth uniform in [4, 30] m: the depth spread is
    of the order of the depth, so no scene is planar.  The keypoint is the projection plus N(0, noise_px) per axis,
    or for a fraction outlier_frac (scalar or per candidate) of the correspondences plus +-U(30, 80) pixels per
    axis.  About extras_frac * n_corr unmatched slots (mp_valid = 0, arbitrary keypoint and point) are interleaved
    at random positions, so the compaction is exercised.  Octaves are uniform in 0 .. 7, level_sigma2 = 1.2^(2
    level).  Returns the batch (with draws from pnpsolver.make_draws and the RANSAC parameters) plus gt_tcw (F, 12),
    outlier (total_kp, bool) and n_corr."""
    from .pnpsolver import make_draws
    rng = np.random.default_rng([seed, 4177])
    counts = [int(n) for n in n_corr]
    F = len(counts)
    frac = [float(outlier_frac)] * F if np.isscalar(outlier_frac) else [float(f) for f in outlier_frac]
    begin, xy, octs, valid, xw, outl, gts = [0], [], [], [], [], [], []
    for p, n in enumerate(counts):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = np.deg2rad(rng.uniform(2, 20))
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
        t = rng.uniform(-3, 3, 3)
        n_extra = int(round(extras_frac * n)) + (1 if n == 0 else 0)
        tot = n + n_extra
        is_corr = np.zeros(tot, bool)
        is_corr[rng.permutation(tot)[:n]] = True
        px = np.stack([rng.uniform(20, cam["width"] - 20, tot), rng.uniform(20, cam["height"] - 20, tot)], 1)
        z = rng.uniform(4, 30, tot)
        Xc = np.stack([(px[:, 0] - cam["cx"]) * z / cam["fx"], (px[:, 1] - cam["cy"]) * z / cam["fy"], z], 1)
        Xw = (Xc - t) @ R   # R^T (Xc - t)
        out = np.zeros(tot, bool)
        ci = np.nonzero(is_corr)[0]
        out[ci[rng.permutation(n)[:int(round(frac[p] * n))]]] = True
        d = np.where(out[:, None], rng.choice([-1, 1], (tot, 2)) * rng.uniform(30, 80, (tot, 2)), rng.normal(0, noise_px, (tot, 2)))
        kp = px + d
        kp[~is_corr] = np.stack([rng.uniform(0, cam["width"], tot), rng.uniform(0, cam["height"], tot)], 1)[~is_corr]
        begin.append(begin[-1] + tot)
        xy.append(kp); octs.append(rng.integers(0, 8, tot)); valid.append(is_corr); xw.append(Xw); outl.append(out & is_corr)
        gts.append(np.concatenate([R.reshape(9), t]))
    cat = lambda parts, w, dt: (np.concatenate(parts) if parts else np.zeros((0, w))).astype(dt).reshape((-1, w) if w > 1 else (-1,))   # noqa: E731
    return dict(kp_begin=np.array(begin, np.int32), kp_xy=cat(xy, 2, np.float32), kp_octave=cat(octs, 1, np.int32),
                camera=np.tile(np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32), (F, 1)),
                mp_valid=cat(valid, 1, np.uint8), mp_xw=cat(xw, 3, np.float32),
                level_sigma2=((1.2 ** np.arange(8)) ** 2).astype(np.float32), draws=make_draws(F, n_draws, seed),
                rand_max=2147483647, probability=float(probability), min_inliers=int(min_inliers), max_iterations=int(max_iterations),
                min_set=4, epsilon=float(epsilon), th2=float(th2), maxk=int(maxk), gt_tcw=np.array(gts, np.float32).reshape(F, 12),
                outlier=cat(outl, 1, bool), n_corr=np.array(counts, np.int32))


def make_initializer_batch(seed: int = 0, n_corr=(150,), scene=("general",), outlier_frac=0.2, noise: float = 0.3,
                           max_iterations: int = 200, kp1_override=None):
    """Initializer inputs (orb_initializer_batch, host arrays) shaped like Tracking::MonocularInitialization: per pair
    N matched keypoints seen from two cameras (fx = fy = 500, a 640 x 480 image), `noise` px of Gaussian noise, a
    fraction `outlier_frac` (scalar or per pair) of the matches pointing at an unrelated keypoint, and int(1.3 N) + 5
    keypoints in either frame, so slots and compacted indices differ and Normalize sees unmatched points.  scene
    (per pair): "plane" (points on a tilted plane), "general" (depths 2 to 8) or "rotation" (no translation).
    kp1_override: {pair: keypoints in frame 1}, to build an oversized frame.  Also returns gt_r21t21 (F, 12)."""
    from .initializer import make_draws
    rng = np.random.default_rng(seed)
    F = len(n_corr)
    scenes = [scene[p % len(scene)] for p in range(F)]
    fracs = [float(outlier_frac)] * F if np.isscalar(outlier_frac) else [float(v) for v in outlier_frac]
    fx = fy = 500.0
    cx, cy = 320.0, 240.0
    b1, b2, xy1s, xy2s, m12s, gts = [0], [0], [], [], [], []
    for p in range(F):
        N = int(n_corr[p])
        n1 = int(1.3 * N) + 5
        if kp1_override and p in kp1_override:
            n1 = int(kp1_override[p])
        n2 = int(1.3 * N) + 5
        u = rng.uniform(40, 600, N)
        v = rng.uniform(40, 440, N)
        xn, yn = (u - cx) / fx, (v - cy) / fy
        if scenes[p] == "plane":
            z = 4.0 / (1.0 + 0.25 * xn + 0.15 * yn)
        else:
            z = rng.uniform(2.0, 8.0, N)
        X = np.stack([xn * z, yn * z, z], 1)
        w = rng.normal(0, 1, 3)
        w *= np.deg2rad(rng.uniform(2, 5)) / np.linalg.norm(w)
        th = np.linalg.norm(w)
        kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        R = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * (kx @ kx)
        t = np.zeros(3) if scenes[p] == "rotation" else np.array([0.45, 0.08, 0.05]) * rng.uniform(0.8, 1.2)
        X2 = X @ R.T + t
        p1 = np.stack([u, v], 1) + rng.normal(0, noise, (N, 2))
        p2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1) + rng.normal(0, noise, (N, 2))
        xy1 = np.stack([rng.uniform(0, 640, n1), rng.uniform(0, 480, n1)], 1)
        xy2 = np.stack([rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)], 1)
        s1 = np.sort(rng.choice(n1, N, replace=False))
        s2 = rng.permutation(n2)[:N]
        xy1[s1] = p1
        xy2[s2] = p2
        m12 = np.full(n1, -1, np.int32)
        m12[s1] = s2
        free = np.setdiff1d(np.arange(n2), s2)
        bad = rng.random(N) < fracs[p]
        if N and len(free):
            m12[s1[bad]] = rng.choice(free, int(bad.sum()))
        xy1s.append(xy1)
        xy2s.append(xy2)
        m12s.append(m12)
        nt = np.linalg.norm(t)
        gts.append(np.concatenate([R.reshape(9), t / nt if nt > 0 else t]))
        b1.append(b1[-1] + n1)
        b2.append(b2[-1] + n2)
    return dict(kp1_begin=np.array(b1, np.int32), kp2_begin=np.array(b2, np.int32),
                kp1_xy=np.concatenate(xy1s).astype(np.float32).reshape(-1, 2),
                kp2_xy=np.concatenate(xy2s).astype(np.float32).reshape(-1, 2), matches12=np.concatenate(m12s).astype(np.int32),
                camera=np.tile(np.array([fx, fy, cx, cy], np.float32), (F, 1)), draws=make_draws(F, max_iterations, seed),
                rand_max=2147483647, sigma=1.0, max_iterations=int(max_iterations), min_parallax=1.0, min_triangulated=50,
                rh_threshold=0.40, gt_r21t21=np.array(gts, np.float32).reshape(F, 12))


def make_new_points_batch(seed: int = 0, n_kf1: int = 2, n_rounds: int = 3, cap: int = 130, counts=None, mode: str = "mixed",
                          monocular=None, noise: float = 0.3, outlier_frac: float = 0.1, mp_frac: float = 0.15,
                          short_frac: float = 0.2, baseline=(0.4, 1.2), along=(1.0, 0.4, 0.3)):
    """CreateNewMapPoints inputs (orblm_batch, host arrays) shaped like LocalMapping's neighbour loop: n_kf1 current
    keyframes with n_rounds neighbours each, all in one slot set of F = n_kf1 (1 + n_rounds) keyframes x cap slots
    (keyframe k < n_kf1 is a current one, its neighbour of round r is n_kf1 + r n_kf1 + k).  Every keyframe sees the
    same world points (depths 4 to 14) from its own pose with its own intrinsics (K1 != K2), `noise` px of Gaussian
    noise, in its own slot order; a fraction outlier_frac of its keypoints lie 4 to 12 px off; descriptors are a world
    point's 256 bits with a few flipped per view, so SearchForTriangulation finds the correspondences by itself.
    mode: "mono" (uright = -1), "stereo" or "mixed" (half the keypoints carry uright / depth); monocular (the skip
    rule) defaults to mode == "mono".  A fraction short_frac of the neighbours sits closer than either skip rule
    allows, the others `baseline` away in a direction drawn with the per-axis weights `along`.  mp_frac of the slots already hold a MapPoint (has_mappoint, mp_xw).  counts: keypoints per keyframe
    (default: cap).  Returns the arrays of mapping.py's batch (sets 1 and 2 are the same arrays), desc, has_mappoint
    and the plan frame1 / frame2 [n_rounds, n_kf1]."""
    from ._lib import KP_DTYPE
    rng = np.random.default_rng(seed)
    F = n_kf1 * (1 + n_rounds)
    counts = np.full(F, cap, np.int32) if counts is None else np.asarray(counts, np.int32)
    assert len(counts) == F and counts.max(initial=0) <= cap
    mono = (mode == "mono") if monocular is None else bool(monocular)
    b = 0.1
    X = np.stack([rng.uniform(-4, 4, cap), rng.uniform(-3, 3, cap), rng.uniform(4, 14, cap)], 1)
    base = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
    scale = np.cumprod(np.concatenate([[np.float32(1)], np.full(7, np.float32(1.2), np.float32)])).astype(np.float32)
    kps = np.zeros((F, cap), KP_DTYPE)
    desc = rng.integers(0, 256, (F, cap, 32), dtype=np.uint8)
    ur = np.full((F, cap), -1, np.float32)
    depth = np.full((F, cap), -1, np.float32)
    mp = np.zeros((F, cap), np.uint8)
    xw = np.zeros((F, cap, 3), np.float32)
    pose = np.zeros((F, 12), np.float32)
    cam = np.zeros((F, 6), np.float32)
    for f in range(F):
        w = rng.normal(0, 1, 3)
        w *= np.deg2rad(rng.uniform(0.5, 4)) / np.linalg.norm(w)
        th = np.linalg.norm(w)
        kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        R = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * (kx @ kx)
        d = rng.normal(0, 1, 3) * np.asarray(along, np.float64)
        d /= np.linalg.norm(d)
        if f < n_kf1:
            t = d * 0.05
        else:
            t = d * (rng.uniform(0.02, 0.06) if rng.random() < short_frac else rng.uniform(*baseline))
        pose[f] = np.concatenate([R.astype(np.float32), t.astype(np.float32)[:, None]], 1).reshape(12)
        fx, fy = 500.0 + 7 * f, 505.0 - 3 * f
        cx, cy = 320.0 + 2 * f, 240.0 - f
        cam[f] = [fx, fy, cx, cy, b * fx, b]
        n = int(counts[f])
        order = rng.permutation(cap)[:n]
        Xc = X[order] @ R.T + t
        u = fx * Xc[:, 0] / Xc[:, 2] + cx + rng.normal(0, noise, n)
        v = fy * Xc[:, 1] / Xc[:, 2] + cy + rng.normal(0, noise, n)
        out = rng.random(n) < outlier_frac
        ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(4, 12, n)
        u = np.where(out, u + mag * np.cos(ang), u)
        v = np.where(out, v + mag * np.sin(ang), v)
        kps["x"][f, :n] = u
        kps["y"][f, :n] = v
        kps["size"][f, :n] = 31
        kps["octave"][f, :n] = rng.integers(0, 3, n)
        flips = np.zeros((n, 32), np.uint8)
        for _ in range(6):
            flips[np.arange(n), rng.integers(0, 32, n)] ^= (1 << rng.integers(0, 8, n)).astype(np.uint8)
        desc[f, :n] = base[order] ^ flips
        if mode != "mono":
            st = np.ones(n, bool) if mode == "stereo" else rng.random(n) < 0.5
            z = Xc[:, 2] + rng.normal(0, 0.02, n)
            depth[f, :n] = np.where(st, z, -1)
            ur[f, :n] = np.where(st, u - b * fx / z, -1)
        has = rng.random(n) < mp_frac
        mp[f, :n] = has
        xw[f, :n] = np.where(has[:, None], X[order], 0)
    k = np.arange(n_kf1, dtype=np.int32)
    frame1 = np.tile(k, (n_rounds, 1))
    frame2 = np.stack([n_kf1 + r * n_kf1 + k for r in range(n_rounds)]).astype(np.int32).reshape(n_rounds, n_kf1)
    return dict(kps1=kps, kps2=kps, counts1=counts, counts2=counts, uright1=None if mode == "mono" else ur,
                depth1=None if mode == "mono" else depth, uright2=None if mode == "mono" else ur,
                depth2=None if mode == "mono" else depth, has_mappoint2=mp.copy(), mp_xw2=xw, pose1=pose, pose2=pose,
                camera1=cam, camera2=cam, frame1=frame1, frame2=frame2, scale_factors2=scale, sigma2_2=(scale * scale).astype(np.float32),
                scale_factor=1.2, monocular=mono, desc=desc, has_mappoint=mp)


def make_keyframe_db_case(seed: int = 0, max_keyframes: int = 70, n_add: int = 68, n_erased: int = 3, word_cap: int = 200,
                          n_places: int = 5, n_queries: int = 5, counts=None, q_counts=None, vocab: int = 4000,
                          share: float = 0.85, q_cap: int = None):
    """A KeyFrameDatabase case (KeyFrameDatabase.cc:34-265): BowVectors built directly (word ids ascending, L1-normalised
    fp64 weights), a covisibility table, connected sets, covisible lists and queries.

    Keyframes are grouped into `n_places` places.  A place owns `word_cap` words; a keyframe of `counts[i]` words takes
    about `share` of them from its place and the rest from a small common pool, so keyframes of one place share most of
    their words, keyframes of different places a few, and the short ones of a place fall below 0.8 x the most shared.
    Each place has two visits: a query of the place (a further keyframe of it) is connected to the first visit only, the
    second is what a loop query should find.  Covisibility rows name keyframes of the same place first, then some of the
    next place, an erased slot and an unused one here and there, -1 padded.  Consecutive queries alternate between two
    neighbouring places, so a relocalisation query meets scores left by the one before.

    Returns dict(max_keyframes, word_cap, slot (n_add,), bow_word / bow_weight (n_add, word_cap), n_words (n_add,), erased,
    place (max_keyframes,; -1 unused), covis (max_keyframes, 10), n_queries, q_cap, q_bow_word / q_bow_weight (F, q_cap),
    q_n_words (F,), q_frame (Q,), q_place (Q,), conn_off / conn_idx, cov_off / cov_idx)."""
    rng = np.random.default_rng(seed)
    K, W = max_keyframes, word_cap
    q_cap = q_cap or W
    pool = rng.choice(vocab, size=max(W // 2, 8), replace=False)                      # words every place may use
    rest = np.setdiff1d(np.arange(vocab), pool)
    place_words = [rng.choice(rest, size=W, replace=False) for _ in range(n_places)]
    idf = rng.uniform(0.5, 8.0, vocab)

    def bow(place, n):
        n_own = min(int(round(share * n)), W)
        if n == 1:
            n_own = 1
        own = rng.choice(place_words[place], size=n_own, replace=False)
        other = rng.choice(pool, size=min(n - n_own, len(pool)), replace=False)
        w = np.unique(np.concatenate([own, other])).astype(np.uint32)
        v = idf[w] * rng.integers(1, 4, len(w))
        return w, (v / v.sum() if len(w) else v)

    if counts is None:
        counts = rng.integers(int(0.3 * W), W + 1, n_add)
        counts[rng.random(n_add) < 0.5] = rng.integers(int(0.85 * W), W + 1)
    counts = np.resize(np.asarray(counts, np.int64), n_add)
    slot = rng.permutation(K)[:n_add].astype(np.int32)
    place_of_add = np.arange(n_add) % n_places
    visit_of_add = (np.arange(n_add) // n_places) % 2
    bw, bv, nw = np.zeros((n_add, W), np.uint32), np.zeros((n_add, W)), np.zeros(n_add, np.int32)
    for i in range(n_add):
        w, v = bow(int(place_of_add[i]), int(counts[i]))
        nw[i] = len(w)
        bw[i, :len(w)], bv[i, :len(w)] = w, v
    erased = slot[rng.choice(n_add, size=n_erased, replace=False)] if n_erased else np.zeros(0, np.int32)
    place = np.full(K, -1, np.int32)
    visit = np.full(K, -1, np.int32)
    place[slot], visit[slot] = place_of_add, visit_of_add
    unused = np.setdiff1d(np.arange(K), slot)
    covis = np.full((K, 10), -1, np.int32)
    for k in slot:
        same = rng.permutation(np.flatnonzero((place == place[k]) & (np.arange(K) != k)))
        nxt = rng.permutation(np.flatnonzero(place == (place[k] + 1) % n_places))
        row = list(same[:int(rng.integers(0, 7))]) + list(nxt[:int(rng.integers(0, 4))])
        if len(unused) and rng.random() < 0.2:
            row.append(int(rng.choice(unused)))
        row = [int(x) for x in rng.permutation(row)][:10] if rng.random() < 0.5 else [int(x) for x in row][:10]
        covis[k, :len(row)] = row
    Q = n_queries
    F = Q + 1
    q_frame = rng.permutation(F)[:Q].astype(np.int32)
    if q_counts is None:
        q_counts = rng.integers(int(0.8 * W), min(W, q_cap) + 1, Q)
    q_counts = np.resize(np.asarray(q_counts, np.int64), Q)
    first = int(rng.integers(0, n_places))
    q_place = np.array([(first + (q % 2)) % n_places for q in range(Q)], np.int32)
    qw, qv, qn = np.zeros((F, q_cap), np.uint32), np.zeros((F, q_cap)), np.zeros(F, np.int32)
    conn_off, conn_idx, cov_off, cov_idx = [0], [], [0], []
    for q in range(Q):
        w, v = bow(int(q_place[q]), int(q_counts[q]))
        f = q_frame[q]
        qn[f] = len(w)
        qw[f, :len(w)], qv[f, :len(w)] = w, v
        conn = [int(k) for k in rng.permutation(np.flatnonzero((place == q_place[q]) & (visit == 0)))]
        if len(unused):
            conn.append(int(unused[q % len(unused)]))
        conn_idx += conn
        conn_off.append(len(conn_idx))
        cov = [k for k in conn if rng.random() < 0.7]
        cov_idx += cov
        cov_off.append(len(cov_idx))
    return dict(max_keyframes=K, word_cap=W, slot=slot, bow_word=bw, bow_weight=bv, n_words=nw, erased=np.asarray(erased, np.int32),
                place=place, covis=covis, n_queries=Q, q_cap=q_cap, q_bow_word=qw, q_bow_weight=qv, q_n_words=qn, q_frame=q_frame,
                q_place=q_place, conn_off=np.asarray(conn_off, np.int32), conn_idx=np.asarray(conn_idx, np.int32),
                cov_off=np.asarray(cov_off, np.int32), cov_idx=np.asarray(cov_idx, np.int32))


def local_map_tables(kf_mappoint, kf_n, n_mappoints: int, kf_bad=None, mp_bad=None, parent=None):
    """The dependent tables of a local map from kf_mappoint (K, kf_cap) / kf_n: observations that agree with it (mp_obs_off /
    mp_obs_kf ascending, mp_nobs), covisibility rows by shared-point count (descending, ties to the lower slot, at most 10,
    -1 padded), a spanning tree (parent = the earlier keyframe sharing most points, slot k - 1 when none does; `parent`
    overrides) and its children as a CSR with ascending lists."""
    kf_mappoint = np.ascontiguousarray(kf_mappoint, np.int32)
    K, M = kf_mappoint.shape[0], int(n_mappoints)
    sees = np.zeros((K, M), bool)
    for k in range(K):
        row = kf_mappoint[k, :kf_n[k]]
        sees[k, row[row >= 0]] = True
    obs = [np.flatnonzero(sees[:, p]) for p in range(M)]
    shared = sees.astype(np.int32) @ sees.astype(np.int32).T
    np.fill_diagonal(shared, 0)
    covis = np.full((K, 10), -1, np.int32)
    par = np.full(K, -1, np.int32)
    for k in range(K):
        order = sorted((j for j in range(K) if shared[k, j] > 0), key=lambda j: (-shared[k, j], j))[:10]
        covis[k, :len(order)] = order
        if k > 0:
            par[k] = int(np.argmax(shared[k, :k])) if shared[k, :k].max() > 0 else k - 1
    if parent is not None:
        par = np.asarray(parent, np.int32)
    kids = [np.flatnonzero(par == k) for k in range(K)]
    csr = lambda rows: (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32),  # noqa: E731
                        (np.concatenate(rows) if rows and sum(len(r) for r in rows) else np.zeros(0)).astype(np.int32))
    child_off, child_idx = csr(kids)
    obs_off, obs_kf = csr(obs)
    return dict(kf_bad=np.zeros(K, np.uint8) if kf_bad is None else np.asarray(kf_bad, np.uint8), kf_covis=covis, kf_parent=par,
                kf_child_off=child_off, kf_child_idx=child_idx, kf_n=np.asarray(kf_n, np.int32), kf_mappoint=kf_mappoint,
                mp_bad=np.zeros(M, np.uint8) if mp_bad is None else np.asarray(mp_bad, np.uint8),
                mp_nobs=np.array([len(r) for r in obs], np.int32), mp_obs_off=obs_off, mp_obs_kf=obs_kf)


def _lm_pose(x: float, yaw: float) -> np.ndarray:
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    return np.concatenate([R.reshape(-1), -R @ np.array([x, 0.0, 0.0])]).astype(np.float32)


def _lm_project(P, cam, xw):
    """float64 projection of points xw (n, 3): u, v, z, dist to the camera centre."""
    R, t = P[:9].astype(np.float64).reshape(3, 3), P[9:].astype(np.float64)
    xc = xw.astype(np.float64) @ R.T + t
    z = xc[:, 2]
    with np.errstate(all="ignore"):
        u, v = cam[0] * xc[:, 0] / z + cam[2], cam[1] * xc[:, 1] / z + cam[3]
    return u, v, z, np.linalg.norm(xw - (-R.T @ t), axis=1)


def make_local_map(seed: int = 0, n_keyframes: int = 70, kf_cap: int = 96, n_mappoints: int = 700, n_frames: int = 3,
                   kp_cap: int = 160, step: float = 0.35, bad_frac: float = 0.05, matched=(5, 60, 120), n_levels: int = 8,
                   scale_factor: float = 1.2, width: float = 640.0, height: float = 480.0):
    """A consistent map as orbtl_map's slot tables plus a batch of frames (orbtl_frames) with keypoint arrays of stride
    kp_cap for the projection search behind it.  Keyframes stand along the x axis `step` apart and look down +z at points
    in a slab; frame f stands among them with matched[f % len(matched)] of its keypoints holding map points (a few bad, a
    few without observations, one held twice, a few lying on another point's projection with its descriptor).  No (frame, point) pair has log(maxDistance / dist) / logScaleFactor within
    1e-4 of an integer.  Returns (tables, frames, keypoints)."""
    rng = np.random.default_rng(seed)
    K, M, F = n_keyframes, n_mappoints, n_frames
    cam = np.array([500.0, 500.0, width / 2, height / 2, 40.0], np.float32)
    span = step * (K - 1)
    xw = np.stack([rng.uniform(-3.0, span + 3.0, M), rng.uniform(-2.0, 2.0, M), rng.uniform(4.0, 12.0, M)], 1).astype(np.float32)
    kf_pose = [_lm_pose(step * k, rng.uniform(-0.1, 0.1)) for k in range(K)]
    kf_mappoint, kf_n = np.full((K, kf_cap), -1, np.int32), np.zeros(K, np.int32)
    for k in range(K):
        u, v, z, _ = _lm_project(kf_pose[k], cam, xw)
        vis = np.flatnonzero((z > 0) & (u >= 0) & (u < width) & (v >= 0) & (v < height))
        kf_n[k] = n = int(rng.integers(kf_cap // 2, kf_cap + 1))
        take = rng.permutation(vis)[:int(0.8 * n)]
        kf_mappoint[k, rng.permutation(n)[:len(take)]] = take
    t = local_map_tables(kf_mappoint, kf_n, M, kf_bad=rng.random(K) < bad_frac, mp_bad=rng.random(M) < bad_frac)
    log_sf = np.float32(np.log(scale_factor))
    first = np.array([t["mp_obs_kf"][t["mp_obs_off"][p]] if t["mp_nobs"][p] else rng.integers(K) for p in range(M)])
    centre = np.stack([[step * k, 0.0, 0.0] for k in first])
    d_ref = np.linalg.norm(xw - centre, axis=1)
    maxd = d_ref * scale_factor ** rng.integers(0, n_levels, M)
    normal = (xw - centre) / d_ref[:, None] + rng.normal(0, 0.35, (M, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    pose = np.stack([_lm_pose(rng.uniform(0.1, 0.9) * span, rng.uniform(-0.15, 0.15)) for _ in range(F)])
    for _ in range(50):   # keep every (frame, point) scale off the integers
        mm = np.stack([maxd, maxd / scale_factor ** (n_levels - 1)], 1).astype(np.float32)
        gap = np.inf
        for f in range(F):
            e = np.log(mm[:, 0].astype(np.float64) / _lm_project(pose[f], cam, xw)[3]) / float(log_sf)
            close = np.abs(e - np.round(e)) < 1e-4
            maxd[close] *= 1.003
            gap = min(gap, np.abs(e - np.round(e)).min())
        if gap >= 1e-4:
            break
    t.update(mp_xw=xw, mp_normal=normal.astype(np.float32), mp_max_min=mm,
             mp_desc=rng.integers(0, 256, (M, 32), dtype=np.uint8), mp_visible=rng.integers(0, 50, M).astype(np.int32))
    frame_n = rng.integers(kp_cap * 3 // 4, kp_cap + 1, F).astype(np.int32)
    frame_mp = np.full((F, kp_cap), -1, np.int32)
    kp_xy = np.stack([rng.uniform(0, width, (F, kp_cap)), rng.uniform(0, height, (F, kp_cap))], 2).astype(np.float32)
    kp_octave = rng.integers(0, n_levels, (F, kp_cap)).astype(np.int32)
    kp_desc = rng.integers(0, 256, (F, kp_cap, 32), dtype=np.uint8)
    for f in range(F):
        u, v, z, dist = _lm_project(pose[f], cam, xw)
        vis = rng.permutation(np.flatnonzero((z > 0) & (u >= 1) & (u < width - 1) & (v >= 1) & (v < height - 1)))
        n, nm = int(frame_n[f]), min(int(matched[f % len(matched)]), len(vis), int(frame_n[f]) - 1)
        slots = rng.permutation(n)
        frame_mp[f, slots[:nm]] = vis[:nm]
        if nm:
            frame_mp[f, slots[nm]] = vis[0]   # one point held by two keypoints
        src = np.concatenate([vis[:nm], vis[:1], rng.permutation(vis)[:max(n - nm - 1 - n // 5, 0)]])   # the rest stay random
        wrong = min(6, nm, max(len(vis) - nm, 0))
        src[:wrong] = vis[nm:nm + wrong]      # a few held points' keypoints lie on another point: that one finds them claimed
        who = slots[:len(src)]
        kp_xy[f, who] = np.stack([u[src], v[src]], 1) + rng.normal(0, 0.4, (len(src), 2))
        lvl = np.ceil(np.log(t["mp_max_min"][src, 0] / dist[src]) / float(log_sf))
        kp_octave[f, who] = np.clip(lvl - rng.integers(0, 2, len(src)), 0, n_levels - 1)
        flips = rng.random((len(src), 256)) < 0.04
        kp_desc[f, who] = t["mp_desc"][src] ^ np.packbits(flips, axis=1)
    kp_xy = np.clip(kp_xy, 0, [width - 1e-3, height - 1e-3]).astype(np.float32)
    with np.errstate(all="ignore"):
        kp_uright = np.where(rng.random((F, kp_cap)) < 0.5, -1.0, kp_xy[..., 0] - rng.uniform(1, 9, (F, kp_cap))).astype(np.float32)
    n_old = rng.integers(0, 4, F).astype(np.int32)
    cap = K + 8
    local_kf = np.full((F, cap), -1, np.int32)
    for f in range(F):
        local_kf[f, :n_old[f]] = rng.permutation(K)[:n_old[f]]
    frames = dict(frame_n=frame_n, frame_mappoint=frame_mp, pose=pose.astype(np.float32), camera=np.tile(cam, (F, 1)),
                  bounds=np.tile(np.array([0, width, 0, height], np.float32), (F, 1)), local_kf=local_kf, n_local_kf=n_old,
                  n_levels=n_levels, log_scale_factor=float(log_sf), min_view_cos=0.5)
    keypoints = dict(kp_xy=kp_xy, kp_octave=kp_octave, kp_uright=kp_uright, kp_desc=kp_desc, bounds=frames["bounds"],
                     scale_factors=(np.float32(scale_factor) ** np.arange(n_levels)).astype(np.float32))
    return t, frames, keypoints
