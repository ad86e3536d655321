"""Numpy restatement of SearchSpacePruning<T>::filterCandidatesByDepth (src/SearchSpacePruning.cpp:73-94) as this project
specifies it (include/pbd_c.h, pbd_set_depth_filter): the reference's loop with its boxes clipped to the depth image.

keep(cand) := nparts(c) >= 2 and for every p in 1 .. nparts(c) - 1:
    not (mc > 0 and mp > 0 and (double)|mc - mp|_T > sqrt((double)ax*ax + (double)ay*ay) * (double)zfactor)
mc / mp = Math::median<T> (element of rank n // 2 in ascending order) over box p / box parentid[c][p], clipped to the image
(empty: "no data", 0); (ax, ay) = anchors[defid[c][p][0]] (anchor(0)).  NaN orders above +inf (np.partition puts NaN last)."""
import math

import numpy as np


def median(depth, box):
    """Math::median<T> over the box clipped to the image; 0 (of T) for an empty intersection."""
    x, y, w, h = (int(v) for v in box)
    dh, dw = depth.shape[:2] if depth is not None else (0, 0)
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, dw), min(y + h, dh)
    if w <= 0 or h <= 0 or x1 <= x0 or y1 <= y0:
        return depth.dtype.type(0) if depth is not None else np.float32(0)
    v = depth[y0:y1, x0:x1].ravel()
    k = v.size // 2
    return np.partition(v, k)[k]


def thresholds(model, zfactor):
    """[c][p]: norm(anchor(0)) * zfactor in double (p >= 1)."""
    z = float(np.float32(zfactor))
    out = []
    for c in range(model.ncomponents):
        row = [0.0]
        for p in range(1, model.nparts(c)):
            ax, ay = (int(v) for v in np.asarray(model.anchors).reshape(-1, 2)[model.defid[c][p][0]])
            row.append(math.sqrt(float(ax) * ax + float(ay) * ay) * z)
        out.append(row)
    return out


def keep_mask(model, heads, boxes, depth, zfactor, dtype=np.float32):
    """Boolean keep flag per record.  depth: HxW array of T (None: every box is "no data")."""
    T = np.dtype(dtype).type
    if depth is not None:
        depth = np.asarray(depth, dtype)
    thr = thresholds(model, zfactor)
    keep = np.zeros(len(heads), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(heads)):
            c = int(heads["component"][i])
            np_ = model.nparts(c)
            if np_ < 2:
                continue
            meds = [T(median(depth, boxes[i, p])) for p in range(np_)]
            ok = True
            for p in range(1, np_):
                mc, mq = meds[p], meds[model.parentid[c][p]]
                if mc > 0 and mq > 0 and float(abs(T(mc - mq))) > thr[c][p]:
                    ok = False
                    break
            keep[i] = ok
    return keep


def depth_filter(model, heads, boxes, locs, depth, zfactor, dtype=np.float32):
    """The kept records, order preserved."""
    k = keep_mask(model, heads, boxes, depth, zfactor, dtype)
    return heads[k], boxes[k], None if locs is None else locs[k]
