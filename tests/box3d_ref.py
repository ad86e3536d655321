"""numpy restatement of Candidate::boundingBox3D (include/Candidate.hpp:140-215) and PointCloudClusterer::computeBoundingBoxes
(include/PointCloudClusterer.hpp:53-150): the rule the GPU's k_box3d must reproduce bit for bit (include/pbd_c.h).

float32 arithmetic op for op where the reference computes in float (the resample, the derivative of Gaussian), double where it
computes in double.  Vectorised within a record; one record at a time.
"""
import math

import numpy as np

from partsbaseddetector_amd import capi

ROWS = 400
F32 = np.float32


def dog_taps():
    """(offsets from the centre, float32 values) of dog = filter2D(getGaussianKernel(35, 4, CV_32F), (-1, 0, 1)) — its nonzero
    taps in raster order (OpenCV 2.4: t = exp(-0.5 / 16 * x * x) stored as float, summed in double, times 1. / sum)"""
    n = 35
    g = np.zeros(n, F32)
    s = 0.0
    for i in range(n):
        x = i - (n - 1) * 0.5
        g[i] = F32(math.exp(-0.5 / (4.0 * 4.0) * x * x))
        s += float(g[i])
    s = 1.0 / s
    g = np.array([F32(float(v) * s) for v in g], F32)
    ref = lambda i: -i if i < 0 else (2 * (n - 1) - i if i >= n else i)   # BORDER_REFLECT_101
    dog = np.array([(F32(0) + F32(-1) * g[ref(i - 1)]) + F32(1) * g[ref(i + 1)] for i in range(n)], F32)
    nz = np.flatnonzero(dog != 0)
    return nz - (n - 1) // 2, dog[nz]


OFFS, TAPS = dog_taps()


def reflect101(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def bounding_box(parts):
    """Candidate::boundingBox: the union of the unclipped part rects (x, y, w, h)"""
    p = np.asarray(parts, np.int64)
    x0, y0 = p[:, 0].min(), p[:, 1].min()
    return int(x0), int(y0), int((p[:, 0] + p[:, 2]).max() - x0), int((p[:, 1] + p[:, 3]).max() - y0)


def bounding_box_norm(parts):
    """Candidate::boundingBoxNorm: cvRound centroids, cv::meanStdDev (sums times 1. / n), Rect of truncated doubles"""
    p = np.asarray(parts, np.int64)
    cx = np.rint((2 * p[:, 0] + p[:, 2]).astype(np.float64) * 0.5)
    cy = np.rint((2 * p[:, 1] + p[:, 3]).astype(np.float64) * 0.5)
    sc = 1.0 / len(p)
    out = []
    for c in (cx, cy):
        s, q = 0.0, 0.0
        for v in c:                       # (integer values: every order of the double sums is exact)
            s += v
            q += v * v
        m = s * sc
        out.append((m, math.sqrt(max(q * sc - m * m, 0.0))))
    (mx, sx), (my, sy) = out
    return int(mx - 1.5 * sx), int(my - 1.5 * sy), int(3 * sx), int(3 * sy)


def clip(r, w, h):
    """cv::Rect & Rect(0, 0, w, h): an empty intersection is Rect()"""
    x, y = max(r[0], 0), max(r[1], 0)
    cw, ch = min(r[0] + r[2], w) - x, min(r[1] + r[3], h) - y
    return (0, 0, 0, 0) if cw <= 0 or ch <= 0 else (x, y, cw, ch)


def scaled_boxes(parts, im_w, im_h, dw, dh):
    sx, sy = dw / float(im_w), dh / float(im_h)
    out = []
    for r in list(map(tuple, np.asarray(parts).tolist())) + [bounding_box_norm(parts)]:
        x, y, w, h = clip(r, im_w, im_h)
        out.append((int(x * sx), int(y * sy), int(w * sx), int(h * sy)))
    return out


def points_of(parts, depth, im_w, im_h):
    """the valid depth values under the boxes (with multiplicity), or None when the record is invalid"""
    dh, dw = depth.shape
    got, first = [], True
    for x, y, w, h in scaled_boxes(parts, im_w, im_h, dw, dh):
        if w <= 0 or h <= 0:
            continue
        v = depth[y:y + h, x:x + w].ravel()
        v = v[(v != 0) & ~np.isnan(v)]
        if first and v.size == 0:
            return None
        first = False
        got.append(v)
    if first:
        return None                        # no box with a non-empty ROI (the reference asserts in cv::resize)
    return np.concatenate(got)


def resample(sorted_pts):
    """cv::resize(points, Size(1, 400)), INTER_LINEAR, OpenCV 2.4 resizeGeneric_ for a float column"""
    n = len(sorted_pts)
    if n == ROWS:
        return sorted_pts.astype(F32).copy()
    scale = 1.0 / (ROWS / float(n))
    fy = ((np.arange(ROWS, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    sy = np.floor(fy).astype(np.int64)
    fy = (fy - sy.astype(F32)).astype(F32)
    s0 = sorted_pts[np.clip(sy, 0, n - 1)].astype(F32)
    s1 = sorted_pts[np.clip(sy + 1, 0, n - 1)].astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (s0 * (F32(1) - fy)).astype(F32) + (s1 * fy).astype(F32)


def dog_filter(pts):
    """filter2D(points, dog): float accumulator from 0, one product then one add per nonzero tap, BORDER_REFLECT_101"""
    m = np.arange(ROWS)
    s = np.zeros(ROWS, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for o, t in zip(OFFS, TAPS):
            s = (s + (t * pts[reflect101(m + o, ROWS)]).astype(F32)).astype(F32)
    return s


def walk(dp):
    midx = ROWS // 2
    bad = np.abs(dp).astype(np.float64) > 0.035
    up = np.flatnonzero(bad[midx:])
    dmax = midx if len(up) and up[0] == 0 else (midx + up[0] - 1 if len(up) else ROWS - 1)
    dn = np.flatnonzero(bad[:midx + 1][::-1])
    dmin = midx if len(dn) and dn[0] == 0 else (midx - dn[0] + 1 if len(dn) else 0)
    return dmin, dmax


def ray(cam, u, v):
    fx, fy, cx, cy, tx, ty = cam
    return (u - cx - tx) / fx, (v - cy - ty) / fy, 1.0


def centres_of(parts, depth, im_w, im_h, cam):
    """the part centres (PointCloudClusterer.hpp:97-141): the reference's transposed window, out-of-image pixels read as 0"""
    dh, dw = depth.shape
    out = []
    for r in np.asarray(parts).tolist():
        x, y, w, h = clip(r, im_w, im_h)
        win = np.zeros((h, w), np.float64)
        rs, cs = min(h, max(dh - x, 0)), min(w, max(dw - y, 0))
        win[:rs, :cs] = depth[x:x + rs, y:y + cs]
        avg = float(win.sum())
        if w * h != 0:
            avg /= w * h
        rx, ry, rz = ray(cam, float(x + w // 2), float(y + h // 2))
        out.append((rx * avg, ry * avg, rz * avg))
    return out


def box3d_one(parts, depth, im_w, im_h, cam):
    """(pbd_box3d as a BOX3D_DTYPE record, centres [nparts, 3]) of one record; depth: float32 (64F rounded first)"""
    o = np.zeros((), capi.BOX3D_DTYPE)
    o["x"], o["y"], o["width"], o["height"] = bounding_box(parts)
    cen = np.zeros((len(parts), 3))
    pts = points_of(parts, depth, im_w, im_h)
    if pts is None:
        o["zmin"] = o["zmax"] = np.nan
        return o, cen
    p = resample(np.sort(pts))
    dmin, dmax = walk(dog_filter(p))
    zmin, zmax = p[dmin], p[dmax]
    o["zmin"], o["zmax"] = zmin, zmax
    cz = float(zmin)
    with np.errstate(invalid="ignore", over="ignore"):
        cd = float(zmax) - float(zmin)
        if math.isnan(cd):
            return o, cen
        o["valid"] = 1
        bx, by, bw, bh = bounding_box(parts)
        t = ray(cam, float(bx), float(by))
        zb = cz + cd
        b = ray(cam, bx + float(bw), by + float(bh))
        tl = (t[0] * cz, t[1] * cz, t[2] * cz)
        br = (b[0] * zb, b[1] * zb, b[2] * zb)
        o["x3d"], o["y3d"], o["z3d"] = tl
        o["width3d"], o["height3d"], o["depth3d"] = br[0] - tl[0], br[1] - tl[1], br[2] - tl[2]
        cen[:] = centres_of(parts, depth, im_w, im_h, cam)
    return o, cen


def as_float_depth(depth):
    """Mat_<float> = depth(r): a 64F depth rounded to float"""
    return np.asarray(depth).astype(F32)


def box3d(heads, boxes, depth, im_w, im_h, cam, max_parts=None):
    """every record: (BOX3D_DTYPE array, centres [n, max_parts, 3]); cam = (fx, fy, cx, cy, tx, ty)"""
    cam = tuple(float(v) for v in cam) + (0.0,) * (6 - len(cam))
    d = as_float_depth(depth) if depth is not None else np.zeros((0, 0), F32)
    boxes = np.asarray(boxes)
    mp = boxes.shape[1] if max_parts is None else max_parts
    out = np.zeros(len(heads), capi.BOX3D_DTYPE)
    cen = np.zeros((len(heads), mp, 3))
    for i in range(len(heads)):
        n = int(heads["nparts"][i])
        out[i], c = box3d_one(boxes[i, :n], d, im_w, im_h, cam)
        cen[i, :n] = c
    return out, cen
