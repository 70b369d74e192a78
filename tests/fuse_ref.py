"""Literal per-point restatement of ORBmatcher::Fuse (src/ORBmatcher.cc:868-980 and :982-1088) and of
SearchByProjection(const KeyFrame*, const Sim3&, points, matched, th) (:518-612) on the orbm_fuse_batch
arrays, with the FeaturesGrid of src/Frame.cc:71-145.  Imports nothing from the package.

Every arithmetic step is an np.float32 scalar operation in the reference's evaluation order; double
where the reference promotes (cv::norm's accumulator, the chi2 compares against 7.8 / 5.99, 0.5 * dist3D)
and math.log on a double for PredictScale.  Constants are wrapped in np.float32 so no step is silently
done in double."""
import math

import numpy as np

F32 = np.float32
COLS, ROWS = 64, 48
TH_LOW = 50
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)

# why a point produced no candidate search, or why a candidate / a best distance was refused
CAUSES = ("invalid", "depth", "image", "distance", "angle", "level", "chi2_mono", "chi2_stereo", "th_low")


def hamming(a, b) -> int:
    return int(_POP[np.bitwise_xor(a, b)].sum())


def _round(v) -> int:   # std::round: halves away from zero
    v = float(v)
    return int(math.floor(v + 0.5)) if v >= 0 else -int(math.floor(-v + 0.5))


def project(P, K, bounds, X, max_min, N, n_levels, log_sf):
    """The gates of :879-910 for one point.  Returns (cause or None, u, v, ur, predictedScale)."""
    P = [F32(x) for x in P]
    K = [F32(x) for x in K]
    X0, X1, X2 = (F32(x) for x in X)
    minx, maxx, miny, maxy = (F32(x) for x in bounds)
    # WorldToCamera: cv::Matx product (s = 0; s += a(i, k) * b(k)), then + tcw
    c0 = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[9]
    c1 = ((P[3] * X0 + P[4] * X1) + P[5] * X2) + P[10]
    c2 = ((P[6] * X0 + P[7] * X1) + P[8] * X2) + P[11]
    if c2 < F32(0):
        return "depth", None, None, None, None
    with np.errstate(all="ignore"):   # z == 0 goes on with inf / nan, as the reference does
        invZ = F32(1) / c2
        u = invZ * K[0] * c0 + K[2]
        v = invZ * K[1] * c1 + K[3]
    if not (u >= minx and u < maxx and v >= miny and v < maxy):
        return "image", None, None, None, None
    ur = u - K[4] / c2
    # Ow = -Rcw^T * tcw
    o0 = -((P[0] * P[9] + P[3] * P[10]) + P[6] * P[11])
    o1 = -((P[1] * P[9] + P[4] * P[10]) + P[7] * P[11])
    o2 = -((P[2] * P[9] + P[5] * P[10]) + P[8] * P[11])
    p0, p1, p2 = X0 - o0, X1 - o1, X2 - o2
    d0, d1, d2 = float(p0), float(p1), float(p2)
    dist3D = F32(math.sqrt((d0 * d0 + d1 * d1) + d2 * d2))   # cv::norm: double accumulator
    maxD, minD = F32(max_min[0]), F32(max_min[1])
    if dist3D < F32(0.8) * minD or dist3D > F32(1.2) * maxD:
        return "distance", None, None, None, None
    dot = ((F32(0) + p0 * F32(N[0])) + p1 * F32(N[1])) + p2 * F32(N[2])   # float Matx::dot
    if float(dot) < 0.5 * float(dist3D):
        return "angle", None, None, None, None
    ratio = maxD / dist3D
    sc = math.ceil(math.log(float(ratio)) / float(F32(log_sf)))
    return None, u, v, ur, max(0, min(int(sc), n_levels - 1))


class Grid:
    """FeaturesGrid::AssignFeatures / GetFeaturesInArea without a level filter."""

    def __init__(self, xy, bounds):
        self.xy = np.asarray(xy, F32).reshape(-1, 2)
        self.minx, maxx, self.miny, maxy = (F32(x) for x in bounds)
        self.invW = F32(COLS) / (maxx - self.minx)
        self.invH = F32(ROWS) / (maxy - self.miny)
        self.cells = {}
        for i, (x, y) in enumerate(self.xy):
            cx = _round(self.invW * (x - self.minx))
            cy = _round(self.invH * (y - self.miny))
            if cx < 0 or cx >= COLS or cy < 0 or cy >= ROWS:
                continue
            self.cells.setdefault((cx, cy), []).append(i)

    def area(self, u, v, r):
        """Indices in scan order (columns, then rows, then insertion order) and each one's cell."""
        mincx = max(math.floor(float(self.invW * (u - r - self.minx))), 0)
        maxcx = min(math.ceil(float(self.invW * (u + r - self.minx))), COLS - 1)
        mincy = max(math.floor(float(self.invH * (v - r - self.miny))), 0)
        maxcy = min(math.ceil(float(self.invH * (v + r - self.miny))), ROWS - 1)
        out = []
        if mincx >= COLS or maxcx < 0 or mincy >= ROWS or maxcy < 0:
            return out
        for cx in range(mincx, maxcx + 1):
            for cy in range(mincy, maxcy + 1):
                for idx in self.cells.get((cx, cy), ()):
                    distx = self.xy[idx, 0] - u
                    disty = self.xy[idx, 1] - v
                    if abs(distx) < r and abs(disty) < r:
                        out.append((idx, (cx, cy)))
        return out


def _items(b):
    kb, mb = np.asarray(b["kp_begin"]), np.asarray(b["mp_begin"])
    for i in range(len(kb) - 1):
        yield i, int(kb[i]), int(kb[i + 1]), int(mb[i]), int(mb[i + 1])


def fuse(b, stats=None):
    """Both Fuse overloads (chi2_gate: the first).  Returns (best_idx, best_dist, n_fused); `stats`, when
    a dict, receives per-cause counts, the per-item (mp_valid, searched = passed every projection gate,
    fused) counts and the ties decided by scan order."""
    M = int(np.asarray(b["mp_begin"])[-1])
    n_items = len(b["kp_begin"]) - 1
    best_idx = np.full(M, -1, np.int32)
    best_dist = np.full(M, 256, np.int32)
    n_fused = np.zeros(n_items, np.int32)
    sf = [F32(x) for x in b["scale_factors"]]
    chi2 = bool(b["chi2_gate"])
    inv_s2 = [F32(x) for x in b["inv_sigma2"]] if chi2 else None
    th = F32(b["th"])
    cnt = dict.fromkeys(CAUSES, 0)
    per_item, ties = [], 0
    for i, k0, k1, m0, m1 in _items(b):
        grid = Grid(b["kp_xy"][k0:k1], b["bounds"][i])
        xy, octv, desc = grid.xy, b["kp_octave"][k0:k1], b["kp_desc"][k0:k1]
        uright = b["kp_uright"][k0:k1] if chi2 else None
        valid = searched = fused = 0
        for m in range(m0, m1):
            if not b["mp_valid"][m]:
                cnt["invalid"] += 1
                continue
            valid += 1
            cause, u, v, ur, ps = project(b["pose"][i], b["camera"][i], b["bounds"][i], b["mp_xw"][m], b["mp_max_min"][m],
                                          b["mp_normal"][m], len(sf), b["log_scale_factor"])
            if cause:
                cnt[cause] += 1
                continue
            searched += 1
            radius = th * sf[ps]
            bestDist, bestIdx, tied = 256, -1, []
            for idx, cell in grid.area(u, v, radius):
                scale = int(octv[idx])
                if scale < ps - 1 or scale > ps:
                    cnt["level"] += 1
                    continue
                if chi2:
                    dx, dy = u - xy[idx, 0], v - xy[idx, 1]
                    if uright[idx] >= 0:
                        dz = ur - F32(uright[idx])
                        if float(((dx * dx + dy * dy) + dz * dz) * inv_s2[scale]) > 7.8:
                            cnt["chi2_stereo"] += 1
                            continue
                    elif float((dx * dx + dy * dy) * inv_s2[scale]) > 5.99:
                        cnt["chi2_mono"] += 1
                        continue
                dist = hamming(b["mp_desc"][m], desc[idx])
                if dist < bestDist:
                    bestDist, bestIdx, tied = dist, idx, [(idx, cell)]
                elif dist == bestDist:
                    tied.append((idx, cell))
            best_dist[m] = bestDist
            if bestDist <= TH_LOW:
                best_idx[m] = bestIdx
                n_fused[i] += 1
                fused += 1
                # a tie that index order would have decided differently
                if any(j < bestIdx and c != tied[0][1] for j, c in tied[1:]):
                    ties += 1
            elif bestIdx >= 0:
                cnt["th_low"] += 1
        per_item.append((valid, searched, fused))
    if stats is not None:
        stats.update(causes=cnt, per_item=per_item, scan_order_ties=ties)
    return best_idx, best_dist, n_fused


def search_by_projection_sim3(b):
    """:518-612.  kp_claimed = matched[k] != nullptr on entry.  Returns (kp_match, n_matches)."""
    K = int(np.asarray(b["kp_begin"])[-1])
    n_items = len(b["kp_begin"]) - 1
    kp_match = np.full(K, -1, np.int32)
    n_matches = np.zeros(n_items, np.int32)
    sf = [F32(x) for x in b["scale_factors"]]
    th = F32(b["th"])
    claimed = b.get("kp_claimed")
    for i, k0, k1, m0, m1 in _items(b):
        grid = Grid(b["kp_xy"][k0:k1], b["bounds"][i])
        octv, desc = b["kp_octave"][k0:k1], b["kp_desc"][k0:k1]
        matched = [bool(claimed[k0 + k]) if claimed is not None else False for k in range(k1 - k0)]
        for m in range(m0, m1):
            if not b["mp_valid"][m]:
                continue
            cause, u, v, _ur, ps = project(b["pose"][i], b["camera"][i], b["bounds"][i], b["mp_xw"][m], b["mp_max_min"][m],
                                           b["mp_normal"][m], len(sf), b["log_scale_factor"])
            if cause:
                continue
            bestDist, bestIdx = 256, -1
            for idx, _cell in grid.area(u, v, th * sf[ps]):
                if matched[idx]:
                    continue
                scale = int(octv[idx])
                if scale < ps - 1 or scale > ps:
                    continue
                dist = hamming(b["mp_desc"][m], desc[idx])
                if dist < bestDist:
                    bestDist, bestIdx = dist, idx
            if bestDist <= TH_LOW:
                matched[bestIdx] = True
                kp_match[k0 + bestIdx] = m - m0
                n_matches[i] += 1
    return kp_match, n_matches
