"""ComputeStereoMatches (src/ORBmatcher.cc:72-247, PatchDistance :60-68) restated in plain Python / numpy with a trace: the
operation oracle/orb_oracle.cpp's oracle_compute_stereo_matches restates, float32 arithmetic in the same expression order
(every float step is rounded to float32 on its own, as -ffp-contract=off leaves it), integers exact.

compute(...) -> dict(uright, depth, trace, median, n_matched)
  trace      one TRACE_DTYPE record per left keypoint: where it ended (`reason`) and what it had found by then
  median     the SAD at the median rank of the call (-1 with no match)
  n_matched  matches before the median filter

Reasons, in the order the operation can end:
  ROW_OUT       (int)y outside [0, rows)
  NO_CAND       no right keypoint passes the row band, octave and window gates (an empty row list included)
  MAXU_NEG      x < 0 on a row whose list is not empty (on an empty one the operation ends earlier: NO_CAND)
  NO_HAMMING    best distance >= TH_HIGH (100)
  HAMMING_HIGH  best distance in 75 .. 99
  BORDER        suR < 0 or suR + 11 >= cols of the left octave's level
  DX_EDGE       the first SAD minimum sits at dx = -5 or +5
  DISP_NEG      refined disparity < 0
  DISP_BIG      refined disparity >= maxd
  MATCH         a match that the median filter keeps
  MATCH_EPS     the same with disparity <= 0 replaced by 0.01
  FILTERED      a match (either kind) with SAD >= 1.5f * 1.4f * median
deltaR outside [-1, 1] has no code: the first strict minimum gives d1 > d2 <= d3, so with a = d1 - d2 > 0 and
b = d3 - d2 >= 0, |deltaR| = |a - b| / (2 (a + b)) <= 0.5 and the reference's test can never fire.

Reads outside a level raise IndexError: neither the reference nor the kernel checks the left patch or the left end of the
right window (suR - 10), so such inputs are out of contract."""
import math

import numpy as np

F32 = np.float32
TH_HIGH, TH_LOW, PR, PS, SR = 100, 50, 5, 11, 5
TH_ORB_DIST = (TH_HIGH + TH_LOW) // 2
REASONS = ("ROW_OUT", "NO_CAND", "MAXU_NEG", "NO_HAMMING", "HAMMING_HIGH", "BORDER", "DX_EDGE", "DISP_NEG", "DISP_BIG",
           "MATCH", "MATCH_EPS", "FILTERED")
(ROW_OUT, NO_CAND, MAXU_NEG, NO_HAMMING, HAMMING_HIGH, BORDER, DX_EDGE, DISP_NEG, DISP_BIG, MATCH, MATCH_EPS,
 FILTERED) = range(len(REASONS))
# best_ham: the smallest distance over the gated candidates (may be >= 100); n_row: length of the row list; sads: the 11
# SAD sums, dx = -5 .. 5; matched: a match before the filter
TRACE_DTYPE = np.dtype([("reason", "i4"), ("n_row", "i4"), ("n_cand", "i4"), ("best_ham", "i4"), ("bestIdxR", "i4"),
                        ("suL", "i4"), ("svL", "i4"), ("suR", "i4"), ("bestdx", "i4"), ("deltaR", "f4"), ("sad", "i4"),
                        ("sads", "i4", (2 * SR + 1,)), ("matched", "?")])
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def round_half_away(x):
    """std::round on a float32 value."""
    x = float(x)
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def scale_tables(nlevels, factor=1.2):
    """ORBextractor's mvScaleFactor / mvInvScaleFactor (ORBextractor.cc:418-432): float32 products, 1.0f / scale."""
    s = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        s[i] = F32(s[i - 1] * F32(factor))
    return s, (F32(1) / s).astype(F32)


def row_band(y, octave, scale):
    """floor(y - r) .. ceil(y + r), r = 2 scale[octave], before the clamp to the image."""
    r = F32(F32(2) * scale[octave])
    return math.floor(F32(F32(y) - r)), math.ceil(F32(F32(y) + r))


def _window(img, y0, y1, x0, x1):
    if y0 < 0 or x0 < 0 or y1 > img.shape[0] or x1 > img.shape[1]:
        raise IndexError(f"patch rows {y0}:{y1} cols {x0}:{x1} outside a {img.shape[0]} x {img.shape[1]} level")
    return img[y0:y1, x0:x1].astype(np.int32)


def compute(kpsL, descL, pyrL, kpsR, descR, pyrR, scale, inv_scale, bf, baseline):
    scale, inv_scale = np.asarray(scale, F32), np.asarray(inv_scale, F32)
    bf, baseline = F32(bf), F32(baseline)
    nL, nR = len(kpsL), len(kpsR)
    uright, depth = np.full(nL, -1, F32), np.full(nL, -1, F32)
    trace = np.zeros(nL, TRACE_DTYPE)
    for f in ("n_row", "n_cand", "best_ham", "bestIdxR", "suL", "svL", "suR", "bestdx", "sad"):
        trace[f] = -1
    trace["sads"] = -1
    trace["deltaR"] = np.nan
    nrows = pyrL[0].shape[0]
    rows = [[] for _ in range(nrows)]
    for iR in range(nR):
        y0, y1 = row_band(kpsR["y"][iR], int(kpsR["octave"][iR]), scale)
        for y in range(max(y0, 0), min(y1, nrows - 1) + 1):
            rows[y].append(iR)
    mind, maxd = F32(0), F32(bf / baseline)
    dist = []
    for iL in range(nL):
        t = trace[iL]
        octL, uL, vL = int(kpsL["octave"][iL]), F32(kpsL["x"][iL]), F32(kpsL["y"][iL])
        row = int(vL)   # truncation, as the C cast
        if row < 0 or row >= nrows:
            t["reason"] = ROW_OUT
            continue
        t["n_row"] = len(rows[row])
        if not rows[row]:
            t["reason"] = NO_CAND
            continue
        minu, maxu = F32(uL - maxd), F32(uL - mind)
        if maxu < 0:
            t["reason"] = MAXU_NEG
            continue
        best, bestIdxR, n_cand = 1 << 30, -1, 0
        for iR in rows[row]:
            o, uR = int(kpsR["octave"][iR]), F32(kpsR["x"][iR])
            if o < octL - 1 or o > octL + 1 or not (uR >= minu and uR <= maxu):
                continue
            n_cand += 1
            d = hamming(descL[iL], descR[iR])
            if d < best:
                best, bestIdxR = d, iR
        t["n_cand"] = n_cand
        if n_cand == 0:
            t["reason"] = NO_CAND
            continue
        t["best_ham"], t["bestIdxR"] = best, bestIdxR
        if best >= TH_ORB_DIST:
            t["reason"] = NO_HAMMING if best >= TH_HIGH else HAMMING_HIGH
            continue
        sf = inv_scale[octL]
        suL = round_half_away(F32(sf * uL))
        svL = round_half_away(F32(sf * vL))
        suR = round_half_away(F32(sf * F32(kpsR["x"][bestIdxR])))
        t["suL"], t["svL"], t["suR"] = suL, svL, suR
        if suR + SR - PR < 0 or suR + SR + PR + 1 >= pyrR[octL].shape[1]:
            t["reason"] = BORDER
            continue
        IL = _window(pyrL[octL], svL - PR, svL + PR + 1, suL - PR, suL + PR + 1)
        W = _window(pyrR[octL], svL - PR, svL + PR + 1, suR - SR - PR, suR + SR + PR + 1)
        sads = []
        for dx in range(-SR, SR + 1):
            IR = W[:, SR + dx:SR + dx + PS]
            sub = IL[PR, PR] - IR[PR, PR]
            sads.append(int(np.abs(IL - IR - sub).sum()))
        t["sads"] = sads
        bi = int(np.argmin(sads))   # the first minimum
        bestdx, sad = bi - SR, sads[bi]
        t["bestdx"], t["sad"] = bestdx, sad
        if bestdx == -SR or bestdx == SR:
            t["reason"] = DX_EDGE
            continue
        d1, d2, d3 = sads[bi - 1], sads[bi], sads[bi + 1]
        deltaR = F32(F32(d1 - d3) / F32(F32(2) * F32(F32(d1 + d3) - F32(F32(2) * F32(d2)))))
        t["deltaR"] = deltaR
        bestuR = F32(scale[octL] * F32(F32(suR + bestdx) + deltaR))
        disparity = F32(uL - bestuR)
        if not disparity >= mind:
            t["reason"] = DISP_NEG
            continue
        if not disparity < maxd:
            t["reason"] = DISP_BIG
            continue
        t["reason"] = MATCH
        if disparity <= 0:
            disparity = F32(0.01)
            bestuR = F32(uL - F32(0.01))
            t["reason"] = MATCH_EPS
        depth[iL] = F32(bf / disparity)
        uright[iL] = bestuR
        t["matched"] = True
        dist.append((sad, iL))
    median = -1
    if dist:
        dist.sort(reverse=True)
        median = dist[max(len(dist) // 2 - 1, 0)][0]
        th = F32(F32(F32(1.5) * F32(1.4)) * F32(median))
        for sad, iL in dist:
            if F32(sad) < th:
                break
            uright[iL] = depth[iL] = -1
            trace["reason"][iL] = FILTERED
    return dict(uright=uright, depth=depth, trace=trace, median=median, n_matched=len(dist))
