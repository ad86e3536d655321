"""Two references for the part-wise overlap NMS (include/pbd_c.h: pbd_candidates_nms_parts), in float64 / exact integers.

nms_m:          matlab/detection/nms.m restated line by line on its own input, a matrix of rows [x1 y1 x2 y2 ... c score] with
                inclusive pixel corners; returns the picked row indices in pick order.
nms_parts_def:  the library's definition on records (heads, boxes [n, mp, 4] as (x, y, w, h)) in their given order; returns the kept
                indices.  `slip` switches on one deliberate mistake, for the tests that show each clause matters."""
import numpy as np

SLIPS = ("later_area", "ge", "no_cover", "area_minus_one", "cap_after")


def nms_m(boxes, overlap=0.5, numpart=None):
    boxes = np.asarray(boxes, np.float64)
    if boxes.size == 0:                                              # :14-16
        return []
    if numpart is None:
        numpart = boxes.shape[1] // 4                                # :10
    rows = np.arange(len(boxes))
    if len(boxes) > 1000:                                            # :19-22 (stable descending sort: scores are distinct where it matters)
        I = np.argsort(-boxes[:, -1], kind="stable")
        rows = I[:1000]
        boxes = boxes[rows]
    x1 = boxes[:, 0:4 * numpart:4]                                   # :30-36
    y1 = boxes[:, 1:4 * numpart:4]
    x2 = boxes[:, 2:4 * numpart:4]
    y2 = boxes[:, 3:4 * numpart:4]
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    rx1, ry1 = x1.min(1, keepdims=True), y1.min(1, keepdims=True)    # :38-42
    rx2, ry2 = x2.max(1, keepdims=True), y2.max(1, keepdims=True)
    rarea = (rx2 - rx1 + 1) * (ry2 - ry1 + 1)
    x1, y1 = np.hstack([x1, rx1]), np.hstack([y1, ry1])              # :44-48
    x2, y2 = np.hstack([x2, rx2]), np.hstack([y2, ry2])
    area = np.hstack([area, rarea])
    s = boxes[:, -1]                                                 # :50-52
    I = list(np.argsort(s, kind="stable"))
    pick = []
    while I:                                                         # :53-70
        i = I[-1]
        pick.append(i)
        J = np.array(I)
        w = np.minimum(x2[i], x2[J]) - np.maximum(x1[i], x1[J]) + 1
        h = np.minimum(y2[i], y2[J]) - np.maximum(y1[i], y1[J]) + 1
        w[w < 0] = 0
        h[h < 0] = 0
        with np.errstate(divide="ignore", invalid="ignore"):
            o = (w * h) / area[i][None, :]
        o = np.fmax.reduce(o, axis=1)                                # MATLAB's max skips NaN
        keep = ~(o > overlap)
        if keep[-1]:                                                 # overlap >= 1: nms.m never drops i and loops forever
            raise RuntimeError("nms.m does not terminate for this overlap")
        I = [j for j, k in zip(I, keep) if k]
    return [int(rows[i]) for i in pick]


def _rect(b):   # (x, y, w, h) -> corners in exact integers; None: empty
    x, y, w, h = (int(v) for v in b)
    return None if w <= 0 or h <= 0 else (x, y, x + w, y + h)


def _area(r, slip):
    if r is None:
        return 0
    if slip == "area_minus_one":
        return (r[2] - r[0] - 1) * (r[3] - r[1] - 1)
    return (r[2] - r[0]) * (r[3] - r[1])


def _inter(a, b):
    if a is None or b is None:
        return 0
    return max(0, min(a[2], b[2]) - max(a[0], b[0])) * max(0, min(a[3], b[3]) - max(a[1], b[1]))


def _rejects(inter, area, overlap, slip):
    if area == 0:
        if inter == 0:
            return False                   # 0 / 0 = NaN rejects nothing
        q = float("inf")
    else:
        q = float(inter) / float(area)     # both exact integers, each rounded once to double, as (double)inter / (double)area
    return q >= overlap if slip == "ge" else q > overlap


def nms_parts_def(heads, boxes, overlap, top, slip=None):
    assert slip is None or slip in SLIPS
    overlap = float(np.float32(overlap))   # the library takes a float and compares in double
    count = len(heads)
    n = count if slip == "cap_after" or not (top > 0 and count > top) else top
    rects = []
    for i in range(n):
        P = int(heads["nparts"][i])
        r = [_rect(boxes[i, p]) for p in range(P)]
        ne = [q for q in r if q is not None]
        cover = None if not ne else (min(q[0] for q in ne), min(q[1] for q in ne), max(q[2] for q in ne), max(q[3] for q in ne))
        rects.append((r, cover))
    gone = [False] * n
    kept = []
    for i in range(n):
        if gone[i]:
            continue
        kept.append(i)
        ri, ci = rects[i]
        for j in range(i + 1, n):
            if gone[j]:
                continue
            rj, cj = rects[j]
            pairs = [(ri[p], rj[p]) for p in range(min(len(ri), len(rj)))]
            if slip != "no_cover":
                pairs.append((ci, cj))
            for a, b in pairs:
                if _rejects(_inter(a, b), _area(b if slip == "later_area" else a, slip), overlap, slip):
                    gone[j] = True
                    break
    if slip == "cap_after" and top > 0:
        kept = kept[:top]
    return kept


def records(seed, n, mp, w=640, hgt=480, ties=True):
    """Adversarial record sets, built like records() of tests/test_gpu_candidate_filter.py: exact score ties (signed zeros among
    them), part counts 0 .. mp, junk in the slots beyond nparts, 5 % of the records with empty boxes, boxes large enough to meet."""
    from partsbaseddetector_amd import capi
    rng = np.random.default_rng(seed)
    heads = np.zeros(n, capi.HEAD_DTYPE)
    sc = rng.normal(0, 2, n).astype(np.float32)
    if ties:
        tie = np.array([0.0, -0.0, 1.5, -2.25, 0.5], np.float32)
        pick = rng.random(n) < 0.4
        sc[pick] = tie[rng.integers(0, len(tie), pick.sum())]
    heads["score"] = sc
    heads["component"] = rng.integers(0, 3, n)
    heads["level"] = rng.integers(0, 40, n)
    heads["nparts"] = rng.integers(0, mp + 1, n)
    big = 200 if n <= 4096 else 48
    boxes = np.zeros((n, mp, 4), np.int32)
    boxes[..., 0] = rng.integers(-big, w + big // 2, (n, mp))
    boxes[..., 1] = rng.integers(-big, hgt + big // 2, (n, mp))
    boxes[..., 2] = rng.integers(-3, big, (n, mp))
    boxes[..., 3] = rng.integers(-3, big, (n, mp))
    junk = np.arange(mp)[None, :] >= np.maximum(heads["nparts"], 1)[:, None]
    boxes[junk] = rng.integers(-2**30, 2**30, (int(junk.sum()), 4))
    empty = rng.random(n) < 0.05
    boxes[empty, :, 2] = 0
    locs = rng.integers(-1000, 1000, (n, mp, 3)).astype(np.int32)
    return heads, boxes, locs
