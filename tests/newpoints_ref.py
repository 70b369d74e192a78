"""numpy float32 restatement of csrc/lm_newpoint.h and of the neighbour loop of orblm.hip (LocalMapping::
CreateNewMapPoints, src/LocalMapping.cc:380-578): the same float32 operations in the same order, so F12, ep2, the
baseline and the median are bit-equal to the header's; the null vector of the 4 x 4 A comes from numpy.linalg (fp64),
the trig from numpy.  The search step is not restated: the loop takes it as a callable (the oracle's).

Beside every result stands each evaluated gate as (value, threshold, scale): margin = |value - threshold| / scale says
how far the decision is from flipping.  jitter=rng moves every entry of A and the stereo parallax cosines by one float
ulp (random signs): jitter_effect() measures what that does to Xw, the normal, the distances and the gated values."""
import numpy as np

f32 = np.float32
STATUS = dict(created=0, no_match=1, pair_skipped=2, low_parallax=3, w_zero=4, behind1=5, behind2=6, reproj1=7, reproj2=8,
              dist_zero=9, scale=10)
BRANCH = dict(none=0, triangulated=1, stereo1=2, stereo2=3)


def dot3(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def mul3(A, B):
    return np.array([[dot3(A[i], B[:, j]) for j in range(3)] for i in range(3)], f32)


def norm3(v):
    v = v.astype(np.float64)
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


class Frame:
    """lm_frame: Tcw (12) and camera (fx, fy, cx, cy, bf, baseline) of one keyframe."""

    def __init__(self, Tcw, cam):
        T = np.asarray(Tcw, f32).reshape(3, 4)
        cam = np.asarray(cam, f32)
        self.T, self.R, self.t = T, T[:, :3], T[:, 3]
        self.Rwc = self.R.T.copy()
        self.Ow = np.array([dot3(-self.Rwc[i], self.t) for i in range(3)], f32)
        self.fx, self.fy, self.cx, self.cy, self.bf, self.b = cam
        self.invfx, self.invfy = f32(1) / self.fx, f32(1) / self.fy

    def world_to_camera(self, X):
        return np.array([f32(dot3(self.R[i], X) + self.t[i]) for i in range(3)], f32)

    def camera_to_image(self, Xc):
        with np.errstate(all="ignore"):
            invZ = f32(1) / Xc[2]
            return f32(f32(f32(invZ * self.fx) * Xc[0]) + self.cx), f32(f32(f32(invZ * self.fy) * Xc[1]) + self.cy)

    def uvz_to_world(self, u, v, Z):
        x = f32(f32(self.invfx * f32(u - self.cx)) * Z)
        y = f32(f32(self.invfy * f32(v - self.cy)) * Z)
        c = np.array([x, y, Z], f32)
        return np.array([f32(dot3(self.Rwc[i], c) + self.Ow[i]) for i in range(3)], f32)

    def kinv(self):
        z, o = f32(0), f32(1)
        return np.array([[self.invfx, z, f32(-self.cx) / self.fx], [z, self.invfy, f32(-self.cy) / self.fy], [z, z, o]], f32)

    def depth(self, X):
        return f32(dot3(self.R[2], np.asarray(X, f32)) + self.t[2])


def pair(f1, f2):
    """lm_pair: F12 (9), ep2 (2), baseline."""
    R12 = mul3(f1.R, f2.Rwc)
    t12 = np.array([f32(dot3(-R12[i], f2.t) + f1.t[i]) for i in range(3)], f32)
    z = f32(0)
    tx = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], f32)
    F12 = mul3(mul3(mul3(f1.kinv().T.copy(), tx), R12), f2.kinv())
    ep2 = np.array(f2.camera_to_image(f2.world_to_camera(f1.Ow)), f32)
    return F12.reshape(9), ep2, f32(norm3(f2.Ow - f1.Ow))


def median_depth(f2, has_mappoint, mp_xw):
    """ComputeSceneMedianDepth(2): (n, depths[(n - 1) / 2]) over the slots with a MapPoint; (0, 0) without one."""
    d = np.array([f2.depth(mp_xw[j]) for j in np.nonzero(has_mappoint)[0]], f32)
    if len(d) == 0:
        return 0, f32(0)
    return len(d), np.sort(d)[(len(d) - 1) // 2]


def skip_rule(monocular, baseline, f2, n, median):
    if not monocular:
        return bool(baseline < f2.b)
    if n == 0:
        return True
    return bool(f32(baseline / median) < f32(0.01))


def _ulp_step(x, rng):
    x = np.asarray(x, f32)
    return np.where(rng.random(x.shape) < 0.5, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(-np.inf))).astype(f32)


def match(f1, f2, tab, kp1, kp2, jitter=None, null_vector=None):
    """lm_match.  kp = (u, v, uright, depth, octave); tab = dict(scale1, sigma1, scale2, sigma2, ratio_factor).
    null_vector(A), when given, stands for the SVD (to reach v(3) == 0, which needs exactly parallel rays that the
    float cosine still calls apart).  Returns dict(status, branch, xw, normal, min_distance, max_distance, gates)."""
    u1, v1, ur1, Z1, o1 = kp1
    u2, v2, ur2, Z2, o2 = kp2
    u1, v1, ur1, Z1, u2, v2, ur2, Z2 = (f32(x) for x in (u1, v1, ur1, Z1, u2, v2, ur2, Z2))
    L = len(tab["scale1"])
    o1, o2 = min(max(int(o1), 0), L - 1), min(max(int(o2), 0), L - 1)
    r = dict(status=STATUS["low_parallax"], branch=BRANCH["none"], xw=np.zeros(3, f32), normal=np.zeros(3, f32),
             min_distance=f32(0), max_distance=f32(0), gates=[])
    g = r["gates"]
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
    xn1 = np.array([f32(f1.invfx * f32(u1 - f1.cx)), f32(f1.invfy * f32(v1 - f1.cy)), 1], f32)
    xn2 = np.array([f32(f2.invfx * f32(u2 - f2.cx)), f32(f2.invfy * f32(v2 - f2.cy)), 1], f32)
    ray1 = np.array([dot3(f1.Rwc[i], xn1) for i in range(3)], f32)
    ray2 = np.array([dot3(f2.Rwc[i], xn2) for i in range(3)], f32)
    cos_rays = f32(np.float64(dot3(ray1, ray2)) / (norm3(ray1) * norm3(ray2)))
    cs1 = cs2 = f32(cos_rays + f32(1))
    if st1:
        cs1 = f32(np.cos(f32(f32(2) * np.arctan2(f32(f32(0.5) * f1.b), Z1))))
        if jitter is not None:
            cs1 = _ulp_step(cs1, jitter)[()]
    elif st2:
        cs2 = f32(np.cos(f32(f32(2) * np.arctan2(f32(f32(0.5) * f2.b), Z2))))
        if jitter is not None:
            cs2 = _ulp_step(cs2, jitter)[()]
    cs = min(cs1, cs2)
    g.append(("parallax", float(cos_rays), float(cs), 1.0))
    g.append(("cos_positive", float(cos_rays), 0.0, 1.0))
    if not (st1 or st2):
        g.append(("cos_0.9998", float(cos_rays), 0.9998, 1.0))
    if cos_rays < cs and cos_rays > 0 and (st1 or st2 or float(cos_rays) < 0.9998):
        r["branch"] = BRANCH["triangulated"]
        A = np.stack([xn1[0] * f1.T[2] - f1.T[0], xn1[1] * f1.T[2] - f1.T[1], xn2[0] * f2.T[2] - f2.T[0],
                      xn2[1] * f2.T[2] - f2.T[1]]).astype(f32)
        if jitter is not None:
            A = _ulp_step(A, jitter)
        r["A"] = A
        w, V = np.linalg.eigh(A.astype(np.float64).T @ A.astype(np.float64))
        v = V[:, 0].astype(f32) if null_vector is None else np.asarray(null_vector(A), f32)
        if v[3] == 0:
            r["status"] = STATUS["w_zero"]
            return r
        denom = 1.0 / np.float64(v[3])
        X = (v[:3].astype(np.float64) * denom).astype(f32)
    elif st1 and cs1 < cs2:
        g.append(("stereo_order", float(cs1), float(cs2), 1.0))
        r["branch"] = BRANCH["stereo1"]
        X = f1.uvz_to_world(u1, v1, Z1)
    elif st2 and cs2 < cs1:
        g.append(("stereo_order", float(cs2), float(cs1), 1.0))
        r["branch"] = BRANCH["stereo2"]
        X = f2.uvz_to_world(u2, v2, Z2)
    else:
        return r
    r["xw"] = X
    Xc1, Xc2 = f1.world_to_camera(X), f2.world_to_camera(X)
    g.append(("z1", float(Xc1[2]), 0.0, float(norm3(Xc1))))
    if Xc1[2] <= 0:
        r["status"] = STATUS["behind1"]
        return r
    g.append(("z2", float(Xc2[2]), 0.0, float(norm3(Xc2))))
    if Xc2[2] <= 0:
        r["status"] = STATUS["behind2"]
        return r
    for k, (f, Xc, u, v, ur, st, sig) in enumerate(((f1, Xc1, u1, v1, ur1, st1, tab["sigma1"][o1]),
                                                     (f2, Xc2, u2, v2, ur2, st2, tab["sigma2"][o2]))):
        pu, pv = f.camera_to_image(Xc)
        dx, dy = f32(pu - u), f32(pv - v)
        ns = f32(f32(dx * dx) + f32(dy * dy))
        th = 5.991 * np.float64(sig)
        if st:
            dz = f32(f32(pu - f32(f.bf / Xc[2])) - ur)
            ns = f32(ns + f32(dz * dz))
            th = 7.8 * np.float64(sig)
        g.append((f"reproj{k + 1}", float(ns), float(th), float(th)))
        if np.float64(ns) > th:
            r["status"] = STATUS["reproj1"] if k == 0 else STATUS["reproj2"]
            return r
    nA, nB = (X - f1.Ow).astype(f32), (X - f2.Ow).astype(f32)
    d1, d2 = norm3(nA), norm3(nB)
    dist1, dist2 = f32(d1), f32(d2)
    if dist1 == 0 or dist2 == 0:
        r["status"] = STATUS["dist_zero"]
        return r
    ratio_dist = f32(dist2 / dist1)
    ratio_octave = f32(tab["scale1"][o1] / tab["scale2"][o2])
    rf = f32(tab["ratio_factor"])
    g.append(("scale_low", float(f32(ratio_dist * rf)), float(ratio_octave), float(ratio_octave)))
    g.append(("scale_high", float(ratio_dist), float(f32(ratio_octave * rf)), float(f32(ratio_octave * rf))))
    if f32(ratio_dist * rf) < ratio_octave or ratio_dist > f32(ratio_octave * rf):
        r["status"] = STATUS["scale"]
        return r
    r["status"] = STATUS["created"]
    i1, i2 = 1.0 / d1, 1.0 / d2
    s = (i1 * nA.astype(np.float64)).astype(f32) + (i2 * nB.astype(np.float64)).astype(f32)
    r["normal"] = (s.astype(np.float64) * 0.5).astype(f32)
    r["max_distance"] = f32(tab["scale1"][o1] * dist1)
    r["min_distance"] = f32(r["max_distance"] / tab["scale1"][L - 1])
    return r


def margin(gates):
    """Smallest |value - threshold| / scale over the evaluated gates (inf without one)."""
    return min((abs(v - t) / s for _, v, t, s in gates if s > 0 and np.isfinite(v)), default=np.inf)


def margins(gates, into=None):
    """The same per kind of gate: {name: smallest margin}, merged into `into`."""
    into = {} if into is None else into
    for n, v, t, s in gates:
        if s > 0 and np.isfinite(v):
            into[n] = min(into.get(n, np.inf), abs(v - t) / s)
    return into


def tables(batch):
    s2, g2 = np.asarray(batch["scale_factors2"], f32), np.asarray(batch["sigma2_2"], f32)
    s1 = np.asarray(batch["scale_factors1"], f32) if batch.get("scale_factors1") is not None else s2
    g1 = np.asarray(batch["sigma2_1"], f32) if batch.get("sigma2_1") is not None else g2
    sf = batch.get("scale_factor")
    sf = f32(s1[min(1, len(s1) - 1)]) if sf is None else f32(sf)
    return dict(scale1=s1, sigma1=g1, scale2=s2, sigma2=g2, ratio_factor=f32(f32(1.5) * sf))


def _kp(batch, s, f, i):
    k = batch["kps" + s][f, i]
    ur, z = batch.get("uright" + s), batch.get("depth" + s)
    return (k["x"], k["y"], f32(-1) if ur is None else ur[f, i], f32(-1) if z is None else z[f, i], int(k["octave"]))


def prepare(batch, frame1=None, frame2=None):
    """orblm_prepare_pairs on a mapping.py host batch: dict of F12, ep2, baseline, median, skip, frame1, frame2."""
    f1s = np.asarray(batch["frame1"] if frame1 is None else frame1).reshape(-1)
    f2s = np.asarray(batch["frame2"] if frame2 is None else frame2).reshape(-1)
    P = len(f1s)
    out = dict(F12=np.zeros((P, 9), f32), ep2=np.zeros((P, 2), f32), baseline=np.zeros(P, f32), median=np.zeros(P, f32),
               skip=np.zeros(P, np.int32), frame1=np.zeros(P, np.int32), frame2=np.zeros(P, np.int32), frames=[None] * P)
    F1, F2 = len(batch["counts1"]), len(batch["counts2"])
    for p, (a, c) in enumerate(zip(f1s, f2s)):
        if a < 0 or c < 0 or a >= F1 or c >= F2:
            out["skip"][p] = 2
            continue
        k1, k2 = Frame(batch["pose1"][a], batch["camera1"][a]), Frame(batch["pose2"][c], batch["camera2"][c])
        out["F12"][p], out["ep2"][p], out["baseline"][p] = pair(k1, k2)
        n, med = 0, f32(0)
        if batch.get("monocular"):
            n2 = int(batch["counts2"][c])
            n, med = median_depth(k2, batch["has_mappoint2"][c][:n2], batch["mp_xw2"][c][:n2])
        out["median"][p] = med
        with np.errstate(all="ignore"):
            out["skip"][p] = int(skip_rule(bool(batch.get("monocular")), out["baseline"][p], k2, n, med))
        out["frame1"][p], out["frame2"][p] = a, c
        out["frames"][p] = (k1, k2)
    return out


def triangulate(batch, pairs, match12, flags1=None, flags2=None, jitter=None):
    """orblm_triangulate: match12 [P, cap1]; flags are updated in place.  Also returns the gates per (pair, idx1)."""
    P, cap1 = match12.shape
    tab = tables(batch)
    out = dict(status=np.full((P, cap1), STATUS["no_match"], np.int32), branch=np.zeros((P, cap1), np.int32),
               xw=np.zeros((P, cap1, 3), f32), normal=np.zeros((P, cap1, 3), f32), min_distance=np.zeros((P, cap1), f32),
               max_distance=np.zeros((P, cap1), f32), new_idx1=np.full((P, cap1), -1, np.int32),
               new_idx2=np.full((P, cap1), -1, np.int32), n_created=np.zeros(P, np.int32), gates={}, A={})
    for p in range(P):
        if pairs["skip"][p] == 2:
            continue
        a, c = int(pairs["frame1"][p]), int(pairs["frame2"][p])
        k1, k2 = pairs["frames"][p]
        n1, n2 = int(batch["counts1"][a]), int(batch["counts2"][c])
        k = 0
        for i in range(n1):
            m = int(match12[p, i])
            if m < 0 or m >= n2:
                continue
            if pairs["skip"][p]:
                out["status"][p, i] = STATUS["pair_skipped"]
                continue
            r = match(k1, k2, tab, _kp(batch, "1", a, i), _kp(batch, "2", c, m), jitter)
            for key in ("status", "branch", "xw", "normal", "min_distance", "max_distance"):
                out[key][p, i] = r[key]
            out["gates"][(p, i)] = r["gates"]
            if "A" in r:
                out["A"][(p, i)] = r["A"]
            if r["status"] == STATUS["created"]:
                out["new_idx1"][p, k], out["new_idx2"][p, k] = i, m
                k += 1
                if flags1 is not None:
                    flags1[a, i] = 1
                if flags2 is not None:
                    flags2[c, m] = 1
        out["n_created"][p] = k
    return out


def loop(batch, search, flags1, flags2, update_flags=True):
    """The neighbour loop: search(round pairs, flags1, flags2) -> match12 [P, cap1] is the oracle's
    SearchForTriangulation on round r's pairs with the current flags.  Returns (pairs, [per-round triangulate results],
    [per-round match12]).  update_flags=False is the loop without the flag update (what one launch over all
    neighbours would compute)."""
    R, P = np.asarray(batch["frame1"]).shape
    pairs = prepare(batch)
    rounds, matches = [], []
    for r in range(R):
        sl = slice(r * P, (r + 1) * P)
        pr = {k: v[sl] for k, v in pairs.items()}
        m12 = search(pr, flags1, flags2)
        matches.append(m12)
        rounds.append(triangulate(batch, pr, m12, flags1 if update_flags else None, flags2 if update_flags else None))
    return pairs, rounds, matches


def jitter_effect(batch, pairs, match12, seed=0):
    """(spread, gate_jitter) of one triangulate call when every entry of A and the stereo cosines move one float ulp
    (signs drawn from `seed`): spread = the largest of |dXw| / |Xw|, |d normal| and |d distance| / distance over the
    triangulated matches, gate_jitter = per kind of gate the largest |d value| / scale over the gates that both runs
    evaluated."""
    base = triangulate(batch, pairs, match12)
    jit = triangulate(batch, pairs, match12, jitter=np.random.default_rng(seed))
    spread, gj = 0.0, {}
    for key, g0 in base["gates"].items():
        p, i = key
        if key in base["A"] and np.all(np.isfinite(base["xw"][p, i])):
            nrm = float(np.linalg.norm(base["xw"][p, i].astype(np.float64)))
            if nrm > 0:
                spread = max(spread, float(np.linalg.norm(jit["xw"][p, i].astype(np.float64) - base["xw"][p, i])) / nrm)
            if base["status"][p, i] == STATUS["created"] and jit["status"][p, i] == STATUS["created"]:
                spread = max(spread, float(np.abs(jit["normal"][p, i].astype(np.float64) - base["normal"][p, i]).max()))
                for k in ("min_distance", "max_distance"):
                    spread = max(spread, abs(float(jit[k][p, i]) - float(base[k][p, i])) / float(base[k][p, i]))
        for (n0, v0, t0, s0), (n1, v1, t1, s1) in zip(g0, jit["gates"][key]):
            if n0 == n1 and s0 > 0 and np.isfinite(v0) and np.isfinite(v1):
                gj[n0] = max(gj.get(n0, 0.0), abs(v1 - v0) / s0, abs(t1 - t0) / s0)
    return spread, gj
