"""References of the evaluation ledger (include/pbd_c.h "evaluation ledger").

1. eval_pck_m, eval_apk_m, vocap_m: matlab/evaluation/eval_pck.m, eval_apk.m and VOCap.m restated line by line, with their 1-based
   logic and their quirks as written (the `nargin < 4` test on three-argument functions; gt(n) read after the loop in eval_pck.m:13).
2. The numpy form of the header's definitions: keypoints, dist, pck, match_frame, ap — what the C host functions and the device kernels are
   held to in bits.
3. random_frames: test data with true positives, misses by distance, double detections, empty frames and tied scores.
"""
import numpy as np

HEAD_DTYPE = np.dtype([("score", np.float32), ("component", np.int32), ("level", np.int32), ("nparts", np.int32)])
SCALE_LAST, SCALE_OWN = 0, 1


# ---- 1. the MATLAB files ------------------------------------------------------------------------------------------------------------
def eval_pck_m(ca, gt, thresh=0.5, literal_nargin=True):
    """eval_pck.m.  ca[n]["point"], gt[n]["point"]: [P, 2]; gt[n]["scale"].  Returns pck [P].  As written the file overwrites the caller's
    thresh with 0.5 (a three-argument function never has nargin >= 4); literal_nargin=False reads the test as the `nargin < 3` it was
    meant to be, so that other thresholds can be compared."""
    nargin = 3
    if nargin < (4 if literal_nargin else 3):                          # :3-5
        thresh = 0.5
    assert len(ca) == len(gt)                                          # :7
    P = np.asarray(gt[0]["point"]).shape[0]
    dist = np.zeros((P, len(gt)), np.float64)
    n = 0
    for n in range(1, len(gt) + 1):                                    # :9
        d = np.asarray(ca[n - 1]["point"], np.float64) - np.asarray(gt[n - 1]["point"], np.float64)
        sq = d ** 2
        dist[:, n - 1] = np.sqrt(sq[:, 0] + sq[:, 1])                  # :10  sqrt(sum((..).^2, 2))
    hit = dist < thresh * gt[n - 1]["scale"]                           # :13  gt(n): n is the loop's last value
    return hit.sum(axis=1) / hit.shape[1]                              #      mean(.., 2)'


def vocap_m(rec, prec):
    """VOCap.m"""
    mrec = np.concatenate([[0.0], rec, [1.0]])                         # :3
    mpre = np.concatenate([[0.0], prec, [0.0]])                        # :4
    for i in range(len(mpre) - 1, 0, -1):                              # :5  i = numel(mpre)-1:-1:1 (1-based)
        mpre[i - 1] = max(mpre[i - 1], mpre[i])                        # :6
    i = np.nonzero(mrec[1:] != mrec[:-1])[0] + 1                       # :8  (0-based index of the later element)
    return float(np.sum((mrec[i] - mrec[i - 1]) * mpre[i]))            # :9


def eval_apk_m(ca, gt, thresh=0.5, literal_nargin=True):
    """eval_apk.m for ONE keypoint.  ca[k]: dict(score, fr (1-based frame), point [2]); gt[i]: dict(numgt, point [numgt, 2],
    scale [numgt]).  Returns (apk, prec, rec, tp flags in the caller's order of ca, tp cumulative, fp cumulative, sort order).
    literal_nargin: as eval_pck_m."""
    nargin = 3
    if nargin < (4 if literal_nargin else 3):                          # :3-5
        thresh = 0.5
    sc = np.array([c["score"] for c in ca], np.float64)
    si = np.argsort(-sc, kind="stable")                                # :7  sort(.., 'descend') is stable
    cas = [ca[k] for k in si]                                          # :8
    numca = len(cas)                                                   # :10
    tp = np.zeros(numca)
    fp = np.zeros(numca)
    det = [np.zeros(g["numgt"], bool) for g in gt]
    for n in range(1, numca + 1):                                      # :14
        i = cas[n - 1]["fr"]                                           # :15
        if gt[i - 1]["numgt"] == 0:                                    # :16
            fp[n - 1] = 1
            continue
        d = np.asarray(cas[n - 1]["point"], np.float64)[None, :] - np.asarray(gt[i - 1]["point"], np.float64)
        sq = d ** 2
        dist = np.sqrt(sq[:, 0] + sq[:, 1])                            # :21
        dist = dist / np.asarray(gt[i - 1]["scale"], np.float64)       # :22
        jmin = int(np.argmin(dist)) + 1                                # :24  the first minimum
        distmin = dist[jmin - 1]
        if distmin <= thresh:                                          # :26
            if not det[i - 1][jmin - 1]:                               # :27
                tp[n - 1] = 1
                det[i - 1][jmin - 1] = True
            else:
                fp[n - 1] = 1                                          # :31
        else:
            fp[n - 1] = 1                                              # :34
    flags = np.zeros(numca, np.uint8)
    flags[si] = tp.astype(np.uint8)
    fpc = np.cumsum(fp)                                                # :38
    tpc = np.cumsum(tp)                                                # :39
    with np.errstate(invalid="ignore", divide="ignore"):
        rec = tpc / sum(g["numgt"] for g in gt)                        # :40
        prec = tpc / (fpc + tpc)                                       # :41
    return vocap_m(rec, prec), prec, rec, flags, tpc, fpc, si          # :43


# ---- 2. the header's definitions ------------------------------------------------------------------------------------------------------
def keypoints(boxes):
    """[..., 4] int (x, y, w, h) -> [..., 2] float64 centres: x2 = x + w - 1, cx = .5 x + .5 x2 (exact)"""
    b = np.asarray(boxes, np.int32).astype(np.float64)
    x2 = b[..., 0] + b[..., 2] - 1.0
    y2 = b[..., 1] + b[..., 3] - 1.0
    return np.stack([.5 * b[..., 0] + .5 * x2, .5 * b[..., 1] + .5 * y2], -1)


def dist(c, g):
    """dx = cx - gx, dy = cy - gy, s = dx*dx + dy*dy (x term first), sqrt(s)"""
    c, g = np.asarray(c, np.float64), np.asarray(g, np.float64)
    dx, dy = c[..., 0] - g[..., 0], c[..., 1] - g[..., 1]
    with np.errstate(over="ignore"):
        return np.sqrt(dx * dx + dy * dy)


def pck(d, scale, thresh, rule):
    """d [N, P] (+Inf: no pose), scale [N] -> pck [P]; N == 0: NaN"""
    d = np.asarray(d, np.float64)
    scale = np.asarray(scale, np.float64)
    N = len(scale)
    s = (np.full(N, scale[N - 1]) if rule == SCALE_LAST else scale) if N else scale
    hits = (d < (thresh * s)[:, None]).sum(axis=0).astype(np.float64) if N else np.zeros(d.shape[1])
    with np.errstate(invalid="ignore"):
        return hits / np.float64(N)


def score_order(score):
    """positions by (score descending as float32 with -0.0 == +0.0, position ascending)"""
    return np.argsort(-np.asarray(score, np.float32).astype(np.float64), kind="stable")


def match_frame(heads, boxes, points, scale, P, thresh):
    """one frame: heads [count], boxes [count, mp, 4], points [ngt, P, 2], scale [ngt] -> tp [count, P] uint8 by given position"""
    count, ngt = len(heads), len(scale)
    tp = np.zeros((count, P), np.uint8)
    if ngt == 0 or count == 0:
        return tp
    kp = keypoints(np.asarray(boxes)[:, :P])                           # [count, P, 2]
    points = np.asarray(points, np.float64).reshape(ngt, P, 2)
    scale = np.asarray(scale, np.float64)
    order = score_order(heads["score"])
    for p in range(P):
        taken = np.zeros(ngt, bool)
        for i in order:
            q = dist(kp[i, p][None, :], points[:, p]) / scale
            j = int(np.argmin(q))                                      # the first index of the minimum
            if q[j] <= thresh and not taken[j]:
                tp[i, p] = 1
                taken[j] = True
    return tp


def block_sum(terms):
    """64 lane-strided partials starting at +0.0 (term k to partial k % 64, k ascending), folded s[t] += s[t + h], h = 32 .. 1"""
    s = np.zeros(64, np.float64)
    with np.errstate(invalid="ignore"):
        for k, t in enumerate(terms):
            s[k % 64] = s[k % 64] + t
        h = 32
        while h >= 1:
            s[:h] = s[:h] + s[h:2 * h]
            h //= 2
    return s[0]


def ap(score, tp, npos):
    """score [M], tp [M, P], npos -> (apk [P], prec [P, M], rec [P, M], tpc [P, M] int, order [M])"""
    score = np.asarray(score, np.float32)
    tp = np.asarray(tp, np.uint8)
    M, P = tp.shape
    order = score_order(score)
    apk = np.zeros(P, np.float64)
    prec, rec, tpcs = np.zeros((P, M)), np.zeros((P, M)), np.zeros((P, M), np.int64)
    for p in range(P):
        tpc = np.cumsum(tp[order, p] != 0).astype(np.int64)
        fpc = np.arange(1, M + 1, dtype=np.int64) - tpc
        with np.errstate(invalid="ignore", divide="ignore"):
            r = tpc.astype(np.float64) / np.float64(npos)
            pr = tpc.astype(np.float64) / (fpc + tpc).astype(np.float64)
        mrec = np.concatenate([[0.0], r, [1.0]])
        mpre = np.concatenate([[0.0], pr, [0.0]])
        for i in range(len(mpre) - 2, -1, -1):
            mpre[i] = max(mpre[i], mpre[i + 1])
        with np.errstate(invalid="ignore"):
            terms = (mrec[1:] - mrec[:-1]) * mpre[1:]                  # M + 1 terms, every i
        apk[p] = block_sum(terms)
        prec[p], rec[p], tpcs[p] = pr, r, tpc
    return apk, prec, rec, tpcs, order


# ---- 3. test data ---------------------------------------------------------------------------------------------------------------------
def box_around(c, w, h):
    """an int box (x, y, w, h) whose centre is within half a pixel of c"""
    return [int(np.floor(c[0] - .5 * (w - 1) + .5)), int(np.floor(c[1] - .5 * (h - 1) + .5)), int(w), int(h)]


def random_frames(seed, P, mp, counts, ngts, span=300.0):
    """frames of detections and persons.  A detection is a copy of a person's points with small noise (mostly inside .5 * scale), a repeat
    of an earlier detection of the frame (a double detection), or a pose placed at random (a miss).  Scores are multiples of 1/4 in
    [-1, 1] (with -0.0 for 0 now and then), so they tie inside and across frames.  -> list of dict(heads, boxes, points, scale)"""
    rng = np.random.default_rng(seed)
    frames = []
    for count, ngt in zip(counts, ngts):
        points = rng.uniform(20.0, span, (ngt, P, 2)).round(2)
        scale = rng.integers(6, 30, ngt).astype(np.float64)
        heads = np.zeros(count, HEAD_DTYPE)
        boxes = np.zeros((count, mp, 4), np.int32)
        heads["nparts"] = P
        heads["component"] = rng.integers(0, 2, count)
        heads["level"] = rng.integers(0, 9, count)
        sc = (rng.integers(-4, 5, count) / 4.0).astype(np.float32)
        sc[(sc == 0) & (rng.random(count) < .5)] = np.float32(-0.0)
        heads["score"] = sc
        for i in range(count):
            kind = rng.random()
            if ngt and kind < .55:
                g = int(rng.integers(0, ngt))
                c = points[g] + rng.normal(0.0, .2 * scale[g], (P, 2))
            elif i and kind < .75:
                boxes[i] = boxes[int(rng.integers(0, i))]
                continue
            else:
                c = rng.uniform(0.0, span + 100.0, (P, 2))
            for p in range(P):
                boxes[i, p] = box_around(c[p], rng.integers(1, 13), rng.integers(1, 13))
        frames.append(dict(heads=heads, boxes=boxes, points=points, scale=scale))
    return frames
