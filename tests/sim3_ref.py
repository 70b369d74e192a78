"""Literal per-point restatement of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1090-1277, with Sim3::Map /
Inverse of include/Sim3.h:40-47) on the orbm_sim3_batch arrays, and of
MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:285-319) on (desc, begin).  Imports the
FeaturesGrid and the Hamming distance of tests/fuse_ref.py and nothing from the package.

Every arithmetic step is an np.float32 scalar operation in the reference's evaluation order; double where
the reference promotes (cv::norm's accumulator) and math.log on a double for PredictScale.  Constants are
wrapped in np.float32 so no step is silently done in double."""
import math

import numpy as np

from fuse_ref import Grid, hamming

F32 = np.float32
TH_HIGH = 100
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)

# why a slot produced no candidate search, or why a candidate / a best distance was refused
CAUSES = ("invalid", "depth", "image", "distance", "level", "th_high")


def _matvec(m, x, t):
    """cv::Matx product (s = 0; s += a(i, k) * b(k)) then + t."""
    return [((m[3 * i] * x[0] + m[3 * i + 1] * x[1]) + m[3 * i + 2] * x[2]) + t[i] for i in range(3)]


def sim3_inverse(S):
    """Sim3::Inverse (Sim3.h:43-47): (R^T, ((-(1 / s)) * R^T) * t, 1 / s) as the 13 floats R, t, s."""
    S = [F32(x) for x in S]
    inv_s = F32(1) / S[12]
    neg = -inv_s
    Rt = [S[3 * c + r] for r in range(3) for c in range(3)]
    m = [neg * e for e in Rt]   # Matx scaled elementwise, then the product
    t = [(m[3 * i] * S[9] + m[3 * i + 1] * S[10]) + m[3 * i + 2] * S[11] for i in range(3)]
    return Rt + t + [inv_s]


def sim3_map(S, x):
    """Sim3::Map (Sim3.h:40): (s * R) * x + t, the matrix scaled elementwise first."""
    S = [F32(v) for v in S]
    return _matvec([S[12] * e for e in S[:9]], [F32(v) for v in x], S[9:12])


def project(P_src, S, K_dst, bounds_dst, X, max_min, n_levels, log_sf):
    """:1133-1158 for one slot: camera of its own keyframe, S.Map, the other keyframe's intrinsics and
    bounds.  Returns (cause or None, u, v, predictedScale)."""
    P = [F32(x) for x in P_src]
    K = [F32(x) for x in K_dst]
    minx, maxx, miny, maxy = (F32(x) for x in bounds_dst)
    c = _matvec(P[:9], [F32(x) for x in X], P[9:12])   # WorldToCamera
    y0, y1, y2 = sim3_map(S, c)
    if y2 < F32(0):
        return "depth", None, None, None
    with np.errstate(all="ignore"):   # z == 0 goes on with inf / nan, as the reference does
        invZ = F32(1) / y2
        u = invZ * K[0] * y0 + K[2]
        v = invZ * K[1] * y1 + K[3]
    if not (u >= minx and u < maxx and v >= miny and v < maxy):
        return "image", None, None, None
    d0, d1, d2 = float(y0), float(y1), float(y2)
    dist3D = F32(math.sqrt((d0 * d0 + d1 * d1) + d2 * d2))   # cv::norm: double accumulator
    maxD, minD = F32(max_min[0]), F32(max_min[1])
    if dist3D < F32(0.8) * minD or dist3D > F32(1.2) * maxD:
        return "distance", None, None, None
    ratio = maxD / dist3D
    sc = math.ceil(math.log(float(ratio)) / float(F32(log_sf)))
    return None, u, v, max(0, min(int(sc), n_levels - 1))


def _one_way(b, p, src, dst, S, sf, cnt, ties):
    """One search loop (:1127-1191 with src = 1, :1194-1258 with src = 2) of pair p."""
    s0, s1 = int(b[f"kp{src}_begin"][p]), int(b[f"kp{src}_begin"][p + 1])
    k0, k1 = int(b[f"kp{dst}_begin"][p]), int(b[f"kp{dst}_begin"][p + 1])
    grid = Grid(b[f"kp{dst}_xy"][k0:k1], b[f"bounds{dst}"][p])
    octv, desc = b[f"kp{dst}_octave"][k0:k1], b[f"kp{dst}_desc"][k0:k1]
    th = F32(b["th"])
    match = np.full(s1 - s0, -1, np.int32)
    for i in range(s0, s1):
        if not b[f"mp{src}_valid"][i]:
            cnt["invalid"] += 1
            continue
        cause, u, v, ps = project(b[f"pose{src}"][p], S, b[f"camera{dst}"][p], b[f"bounds{dst}"][p], b[f"mp{src}_xw"][i],
                                  b[f"mp{src}_max_min"][i], len(sf), b["log_scale_factor"])
        if cause:
            cnt[cause] += 1
            continue
        bestDist, bestIdx, tied = 2 ** 31 - 1, -1, []
        for idx, cell in grid.area(u, v, th * sf[ps]):
            scale = int(octv[idx])
            if scale < ps - 1 or scale > ps:
                cnt["level"] += 1
                continue
            dist = hamming(b[f"mp{src}_desc"][i], desc[idx])
            if dist < bestDist:
                bestDist, bestIdx, tied = dist, idx, [(idx, cell)]
            elif dist == bestDist:
                tied.append((idx, cell))
        if bestDist <= TH_HIGH:
            match[i - s0] = bestIdx
            # a tie that index order would have decided differently
            if any(j < bestIdx and c != tied[0][1] for j, c in tied[1:]):
                ties[0] += 1
        elif bestIdx >= 0:
            cnt["th_high"] += 1
    return match


def search_by_sim3(b, stats=None):
    """Returns (match12 [total_kp1], match1 [total_kp1], match2 [total_kp2], n_found [n_pairs]); `stats`,
    when a dict, receives per-cause counts over both directions, the one-way-only matches (match1 >= 0
    with match12 == -1) and the ties decided by scan order."""
    n_pairs = len(b["kp1_begin"]) - 1
    sf = [F32(x) for x in b["scale_factors"]]
    cnt = dict.fromkeys(CAUSES, 0)
    ties = [0]
    m12, m1, m2 = [], [], []
    n_found = np.zeros(n_pairs, np.int32)
    for p in range(n_pairs):
        S12 = b["s12"][p]
        a = _one_way(b, p, 1, 2, sim3_inverse(S12), sf, cnt, ties)
        c = _one_way(b, p, 2, 1, S12, sf, cnt, ties)
        agreed = np.full(len(a), -1, np.int32)
        for i1, idx2 in enumerate(a):
            if idx2 >= 0 and c[idx2] == i1:
                agreed[i1] = idx2
                n_found[p] += 1
        m12.append(agreed)
        m1.append(a)
        m2.append(c)
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)   # noqa: E731
    m12, m1, m2 = cat(m12), cat(m1), cat(m2)
    if stats is not None:
        stats.update(causes=cnt, one_way_only=int(((m1 >= 0) & (m12 < 0)).sum()), scan_order_ties=ties[0])
    return m12, m1, m2, n_found


def distinctive_descriptors(desc, begin):
    """:285-319 per point.  Returns (best, best_median), both -1 for an empty point."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    begin = np.asarray(begin)
    P = len(begin) - 1
    best = np.full(P, -1, np.int32)
    best_median = np.full(P, -1, np.int32)
    for p in range(P):
        rows = desc[int(begin[p]):int(begin[p + 1])]
        N = len(rows)
        if N == 0:
            continue
        # distances[i][j] = DescriptorDistance(row i, row j), zero diagonal (a row at a time: N = 1024 stays quick)
        distances = [_POP[np.bitwise_xor(rows, rows[i])].sum(axis=1) for i in range(N)]
        bestMedian, bestIdx = 2 ** 31 - 1, 0
        for i in range(N):
            median = int(np.sort(distances[i])[(N - 1) // 2])
            if median < bestMedian:
                bestMedian, bestIdx = median, i
        best[p], best_median[p] = bestIdx, bestMedian
    return best, best_median
