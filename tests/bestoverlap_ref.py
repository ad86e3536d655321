"""Two references for the best pose per ground-truth box (include/pbd_c.h: pbd_candidates_best_overlap), in float64.

bestoverlap_m:    matlab/detection/bestoverlap.m restated line by line on its own input, a matrix of rows [x1 y1 x2 y2 ... c score]
                  with inclusive pixel corners, one gt box (x1, y1, x2, y2) and an overlap; returns the picked row index or None.
best_overlap_def: the library's definition on records (heads, boxes [n, mp, 4] as (x, y, w, h)) in their given order, for a list of gt
                  boxes; returns (best[ngt], o[ngt])."""
import numpy as np


def bestoverlap_m(boxes, gtbox, overlap):
    boxes = np.asarray(boxes, np.float64)
    gtbox = np.asarray(gtbox, np.float64)
    if boxes.size == 0 or gtbox.size == 0:                           # :3-6
        return None
    x1, y1, x2, y2 = gtbox                                           # :8
    area = (x2 - x1 + 1) * (y2 - y1 + 1)                             # :9
    b = boxes[:, :boxes.shape[1] // 4 * 4]                           # :11
    b = b.reshape(b.shape[0], b.shape[1] // 4, 4)                    # :12 (MATLAB's reshape is column-major: (row, 4, part); here (row, part, 4))
    bx = .5 * b[:, :, 0] + .5 * b[:, :, 2]                           # :13
    by = .5 * b[:, :, 1] + .5 * b[:, :, 3]                           # :14
    bx1, bx2 = bx.min(1), bx.max(1)                                  # :15-16
    by1, by2 = by.min(1), by.max(1)                                  # :17-18
    xx1, yy1 = np.maximum(x1, bx1), np.maximum(y1, by1)              # :20-21
    xx2, yy2 = np.minimum(x2, bx2), np.minimum(y2, by2)              # :22-23
    w = xx2 - xx1 + 1                                                # :25
    w[w < 0] = 0
    h = yy2 - yy1 + 1                                                # :26
    h[h < 0] = 0
    inter = w * h                                                    # :27
    with np.errstate(divide="ignore", invalid="ignore"):
        o = inter / area                                             # :28
    I = np.flatnonzero(o > overlap)                                  # :29
    if len(I) == 0:                                                  # :31
        return None
    return int(I[int(np.argmax(boxes[I, -1]))])                      # :32-33 (max: the first of equal values)


def to_matrix(heads, boxes, P):
    """records of P parts each -> bestoverlap.m's matrix: corners x2 = x + w - 1, y2 = y + h - 1, then component and score"""
    n = len(heads)
    m = np.zeros((n, 4 * P + 2), np.float64)
    b = np.asarray(boxes, np.float64)[:, :P]
    m[:, 0:4 * P:4] = b[..., 0]
    m[:, 1:4 * P:4] = b[..., 1]
    m[:, 2:4 * P:4] = b[..., 0] + b[..., 2] - 1
    m[:, 3:4 * P:4] = b[..., 1] + b[..., 3] - 1
    m[:, -2] = heads["component"]
    m[:, -1] = heads["score"].astype(np.float64)
    return m


def best_overlap_def(heads, boxes, gt, overlap):
    gt = np.asarray(gt, np.float64).reshape(-1, 4)
    overlap = np.float64(overlap)
    n = len(heads)
    cb = np.zeros((n, 4), np.float64)
    has = np.zeros(n, bool)
    for i in range(n):
        P = int(heads["nparts"][i])
        if P == 0:                                                   # rule 2
            continue
        b = boxes[i, :P].astype(np.float64)
        x2 = b[:, 0] + b[:, 2] - 1.0                                 # rule 1
        y2 = b[:, 1] + b[:, 3] - 1.0
        cx = .5 * b[:, 0] + .5 * x2
        cy = .5 * b[:, 1] + .5 * y2
        cb[i] = (cx.min(), cy.min(), cx.max(), cy.max())
        has[i] = True
    best = np.full(len(gt), -1, np.int32)
    o = np.zeros(len(gt), np.float64)
    score = heads["score"]                                           # rule 5: compared as the stored float32
    for g, (x1, y1, x2, y2) in enumerate(gt):
        area = (x2 - x1 + np.float64(1)) * (y2 - y1 + np.float64(1))  # rule 3, elementwise over the records: the same IEEE operations
        w = np.minimum(x2, cb[:, 2]) - np.maximum(x1, cb[:, 0]) + np.float64(1)
        h = np.minimum(y2, cb[:, 3]) - np.maximum(y1, cb[:, 1]) + np.float64(1)
        w = np.where(w < 0, np.float64(0), w)
        h = np.where(h < 0, np.float64(0), h)
        with np.errstate(divide="ignore", invalid="ignore"):
            ov = (w * h) / area
        for i in np.flatnonzero(has & (ov > overlap)):               # rule 4; in the given order: the first of equal scores stays
            if best[g] < 0 or score[i] > score[best[g]]:
                best[g], o[g] = i, ov[i]
    return best, o


def records(seed, n, mp, w=640, hgt=480, distinct=True, nparts=None, tie_run=0):
    """Seeded records: boxes with even and odd w and h (half-integer and integer centres), a few with negative sizes, junk in the slots
    beyond nparts.  distinct: all scores differ; tie_run > 0: runs of that many consecutive records share one exact score, the runs'
    scores ascending with the position, so that the best matching record tends to sit in the last run."""
    from partsbaseddetector_amd import capi
    rng = np.random.default_rng(seed)
    heads = np.zeros(n, capi.HEAD_DTYPE)
    if tie_run:
        sc = ((np.arange(n) // tie_run).astype(np.float32) - 3.0) * np.float32(0.25)
    else:
        sc = rng.permutation(n).astype(np.float32) * np.float32(0.125) - np.float32(n / 16.0) if distinct else rng.integers(-3, 4, n).astype(np.float32) * np.float32(0.5)
    heads["score"] = sc
    heads["component"] = rng.integers(0, 3, n)
    heads["level"] = rng.integers(0, 40, n)
    heads["nparts"] = mp if nparts is None else nparts
    boxes = np.zeros((n, mp, 4), np.int32)
    cx = rng.integers(0, w, n)[:, None]
    cy = rng.integers(0, hgt, n)[:, None]
    boxes[..., 0] = cx + rng.integers(-40, 40, (n, mp))
    boxes[..., 1] = cy + rng.integers(-60, 60, (n, mp))
    boxes[..., 2] = rng.integers(1, 50, (n, mp))
    boxes[..., 3] = rng.integers(1, 50, (n, mp))
    neg = rng.random(n) < 0.03
    boxes[neg, 0, 2] = -7
    junk = np.arange(mp)[None, :] >= heads["nparts"][:, None]
    boxes[junk] = rng.integers(-2**30, 2**30, (int(junk.sum()), 4))
    return heads, boxes


def gt_boxes(seed, ngt, w=640, hgt=480):
    """Seeded gt boxes of person size, with fractional corners"""
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(-20, w - 60, ngt)
    y1 = rng.uniform(-20, hgt - 80, ngt)
    return np.stack([x1, y1, x1 + rng.uniform(30, 160, ngt), y1 + rng.uniform(40, 220, ngt)], 1)
