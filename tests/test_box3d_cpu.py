"""3-D bounding boxes (pbd_set_box3d / pbd_get_box3d / pbd_candidates_box3d): the numpy restatement against a literal
per-pixel transcription of Candidate::boundingBox3D and PointCloudClusterer::computeBoundingBoxes, known answers, and the C ABI
surface that needs no GPU."""
import ctypes as C
import math
import os
import re

import numpy as np

from partsbaseddetector_amd import capi
from tests import box3d_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbd_set_box3d", "pbd_get_box3d", "pbd_candidates_box3d")
F32 = np.float32


def literal(parts, depth, im_w, im_h, cam):
    """include/Candidate.hpp:105-215 and include/PointCloudClusterer.hpp:76-147 as written, one pixel at a time: push_back,
    sorted(), cv::resize's row loop, getGaussianKernel / filter2D loops and the walk.  Returns (valid, bb, zmin, zmax, rect3d,
    centres)."""
    parts = [tuple(int(v) for v in p) for p in parts]
    depth = np.asarray(depth).astype(F32)       # Mat_<float>: a 64F depth rounded (the centres too: pbd_c.h's deviation)
    # boundingBox
    hx, hy, hw, hh = parts[0]
    for p in parts:
        x1, y1 = min(hx, p[0]), min(hy, p[1])
        hw, hh = max(hx + hw, p[0] + p[2]) - x1, max(hy + hh, p[1] + p[3]) - y1
        hx, hy = x1, y1
    bb = (hx, hy, hw, hh)
    # boundingBoxNorm: Point((tl + br) * 0.5) = saturate_cast<int>: Python's round() is half to even, as cvRound
    xs = [round((p[0] + p[0] + p[2]) * 0.5) for p in parts]
    ys = [round((p[1] + p[1] + p[3]) * 0.5) for p in parts]

    def msd(v):
        s = sq = 0.0
        for a in v:
            s += a
            sq += float(a) * a
        scale = 1.0 / len(v)
        s *= scale
        return s, math.sqrt(max(sq * scale - s * s, 0.0))
    (xm, xsd), (ym, ysd) = msd(xs), msd(ys)
    bbn = (int(xm - 1.5 * xsd), int(ym - 1.5 * ysd), int(3 * xsd), int(3 * ysd))

    def clip(r):
        x1, y1 = max(r[0], 0), max(r[1], 0)
        w, h = min(r[0] + r[2], im_w) - x1, min(r[1] + r[3], im_h) - y1
        return (0, 0, 0, 0) if w <= 0 or h <= 0 else (x1, y1, w, h)
    dh, dw = depth.shape
    sx, sy = dw / float(im_w), dh / float(im_h)
    points = []
    nan = (False, bb, None, None, None, None)
    for r in [clip(p) for p in parts] + [clip(bbn)]:
        x, y, w, h = int(r[0] * sx), int(r[1] * sy), int(r[2] * sx), int(r[3] * sy)
        if w == 0 or h == 0:                    # part.empty()
            continue
        for row in range(y, y + h):
            for col in range(x, x + w):
                v = F32(depth[row, col])
                if v != 0 and not np.isnan(v):
                    points.append(v)
        if not points:
            return nan
    if not points:
        return nan                              # (the reference asserts inside cv::resize here)
    points = sorted(points)
    N = len(points)
    # cv::resize(points, points, Size(1, 400)): resizeGeneric_, INTER_LINEAR, one column
    if N == 400:
        pts = [F32(v) for v in points]
    else:
        scale_y = 1.0 / (400.0 / N)
        pts = []
        for dy in range(400):
            fy = F32((dy + 0.5) * scale_y - 0.5)
            s0 = int(math.floor(fy))
            fy = F32(fy - F32(s0))
            r0, r1 = min(max(s0, 0), N - 1), min(max(s0 + 1, 0), N - 1)
            with np.errstate(invalid="ignore", over="ignore"):
                pts.append(F32(F32(points[r0] * F32(F32(1) - fy)) + F32(points[r1] * fy)))
    # getGaussianKernel(35, 4, CV_32F)
    g = []
    ssum = 0.0
    for i in range(35):
        x = i - 34 * 0.5
        g.append(F32(math.exp(-0.5 / 16.0 * x * x)))
        ssum += float(g[-1])
    ssum = 1.0 / ssum
    g = [F32(float(c) * ssum) for c in g]

    def r101(i, n):
        return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)
    diff = [F32(-1), F32(0), F32(1)]
    dog = []
    for i in range(35):
        s = F32(0)
        for k in range(3):
            if diff[k] != 0:
                s = F32(s + F32(diff[k] * g[r101(i + k - 1, 35)]))
        dog.append(s)
    dpoints = []
    for m in range(400):
        s = F32(0)
        for k in range(35):
            if dog[k] != 0:
                with np.errstate(invalid="ignore", over="ignore"):
                    s = F32(s + F32(dog[k] * pts[r101(m + k - 17, 400)]))
        dpoints.append(s)
    midx = 200
    dmin = dmax = midx
    for m in range(midx, 400):
        if abs(float(dpoints[m])) > 0.035:
            break
        dmax = m
    for m in range(midx, -1, -1):
        if abs(float(dpoints[m])) > 0.035:
            break
        dmin = m
    zmin, zmax = pts[dmin], pts[dmax]
    cube = (bb[0], bb[1], float(zmin), bb[2], bb[3], float(zmax) - float(zmin))
    if any(math.isnan(v) for v in cube):
        return (False, bb, zmin, zmax, None, None)
    fx, fy_, cx, cy, tx, ty = cam

    def ray(u, v):
        return ((u - cx - tx) / fx, (v - cy - ty) / fy_, 1.0)
    centres = []
    for p in parts:
        x, y, w, h = clip(p)
        cu, cv = x + w // 2, y + h // 2
        avg = 0.0
        for row in range(x, x + h):
            for col in range(y, y + w):
                avg += float(depth[row, col]) if row < dh and col < dw else 0.0
        if w * h != 0:
            avg /= w * h
        r = ray(float(cu), float(cv))
        centres.append((r[0] * avg, r[1] * avg, r[2] * avg))
    t = ray(float(cube[0]), float(cube[1]))
    b = ray(cube[0] + float(cube[3]), cube[1] + float(cube[4]))
    tl = tuple(c * cube[2] for c in t)
    br = tuple(c * (cube[2] + cube[5]) for c in b)
    return (True, bb, zmin, zmax, (tl[0], tl[1], tl[2], br[0] - tl[0], br[1] - tl[1], br[2] - tl[2]), centres)


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)) or \
        (a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)))))


def check(parts, depth, im_w, im_h, cam):
    want = literal(parts, depth, im_w, im_h, cam)
    o, cen = box3d_ref.box3d_one(np.asarray(parts), box3d_ref.as_float_depth(depth), im_w, im_h, tuple(cam))
    assert bool(o["valid"]) == want[0]
    assert (int(o["x"]), int(o["y"]), int(o["width"]), int(o["height"])) == want[1]
    if want[2] is None:
        assert np.isnan(o["zmin"]) and np.isnan(o["zmax"])
    else:
        assert same(o["zmin"], want[2]) and same(o["zmax"], want[3])
    if want[0]:
        got = [float(o[k]) for k in ("x3d", "y3d", "z3d", "width3d", "height3d", "depth3d")]
        assert same(got, want[4])
        np.testing.assert_allclose(cen, np.array(want[5]), rtol=1e-12, atol=0)
    else:
        assert not np.any(cen)
    return o


def random_parts(rng, n, im_w, im_h):
    x = rng.integers(-8, im_w, n)
    y = rng.integers(-8, im_h, n)
    w = rng.integers(1, 14, n)
    h = rng.integers(1, 14, n)
    return np.stack([x, y, w, h], 1)


def scene(rng, dh, dw, kind):
    d = rng.uniform(0.5, 4.0, (dh, dw)).astype(F32)
    if kind >= 1:
        d[rng.random((dh, dw)) < 0.2] = 0
    if kind >= 2:
        d[rng.random((dh, dw)) < 0.05] = np.nan
        d[rng.random((dh, dw)) < 0.03] = np.inf
        d[rng.random((dh, dw)) < 0.03] = -np.inf
        d[rng.random((dh, dw)) < 0.05] = -rng.uniform(0.1, 2.0)
    if kind == 3:
        d[: dh // 2] = F32(1.25)
    return d


CAM = (525.0, 523.5, 319.5, 239.5, 0.0, 0.0)


def test_restatement_matches_the_literal_transcription():
    rng = np.random.default_rng(11)
    im_w, im_h = 40, 30
    for trial in range(40):
        kind = trial % 4
        size = [(30, 40), (15, 20), (23, 31), (45, 57)][trial % 4]   # equal, half, non-integer ratios (down and up)
        depth = scene(rng, *size, kind)
        if trial % 5 == 4:
            depth = depth.astype(np.float64) + rng.uniform(-1e-9, 1e-9, size)   # 64F: rounded to float first
        n = 1 if trial % 7 == 0 else int(rng.integers(2, 9))
        check(random_parts(rng, n, im_w, im_h), depth, im_w, im_h, CAM if trial % 2 else (300.0, 310.0, 20.0, 15.0, 0.5, -0.25))


def test_invalid_rule():
    depth = np.zeros((30, 40), F32)
    depth[10:20, 10:20] = 2.0
    # the first box with a non-empty ROI has no valid pixel: invalid, although a later box has some
    o = check([(0, 0, 4, 4), (10, 10, 5, 5)], depth, 40, 30, CAM)
    assert not o["valid"] and np.isnan(o["zmin"])
    # the first box is outside the image (empty ROI: skipped), the second has points: valid
    o = check([(50, 50, 4, 4), (10, 10, 5, 5)], depth, 40, 30, CAM)
    assert o["valid"] and o["zmin"] == 2.0
    # no box with a non-empty ROI at all (deviation: invalid, the reference asserts)
    o = check([(50, 50, 4, 4)], depth, 40, 30, CAM)
    assert not o["valid"]
    # boxes that scale to nothing on a small depth map
    o = check([(10, 10, 2, 2)], np.ones((3, 4), F32), 40, 30, CAM)
    assert not o["valid"]
    # inf - inf: the cube contains a NaN, skipped
    o = check([(10, 10, 5, 5)], np.full((30, 40), np.inf, F32), 40, 30, CAM)
    assert not o["valid"] and o["zmin"] == np.inf


def test_point_counts_around_the_resample_size():
    rng = np.random.default_rng(5)
    for n in (1, 2, 399, 400, 401, 1000):
        depth = np.zeros((40, 60), F32)
        flat = rng.uniform(0.5, 3.0, 40 * 60).astype(F32)
        depth.ravel()[:n] = flat[:n]                 # rows of 60: the first n pixels in raster order
        rows = (n + 59) // 60
        o = check([(0, 0, 60, rows)], depth, 60, 40, CAM)   # one part: bbn is empty, N = n
        assert o["valid"]


def test_known_answers():
    depth = np.full((30, 40), F32(2.0))
    o = check([(5, 5, 10, 10), (12, 8, 6, 6)], depth, 40, 30, CAM)
    assert o["valid"] and o["zmin"] == o["zmax"] == 2.0 and o["depth3d"] == 0.0
    # two planes, 70 % near and 30 % far under one box: the walk from the median stops before the step
    depth = np.full((20, 20), F32(1.0))
    depth[14:] = F32(3.0)
    o = check([(0, 0, 20, 20)], depth, 20, 20, CAM)
    assert o["zmin"] == o["zmax"] == 1.0
    pts = box3d_ref.resample(np.sort(depth.ravel()))
    dmin, dmax = box3d_ref.walk(box3d_ref.dog_filter(pts))
    assert dmin == 0 and 200 < dmax < 280 - 5
    # centroids at x.5 round half to even
    assert box3d_ref.bounding_box_norm([(0, 0, 1, 1)]) == (0, 0, 0, 0)        # 0.5 -> 0
    assert box3d_ref.bounding_box_norm([(1, 1, 1, 1)]) == (2, 2, 0, 0)        # 1.5 -> 2
    assert box3d_ref.bounding_box_norm([(2, 2, 1, 1)]) == (2, 2, 0, 0)        # 2.5 -> 2
    # the derivative of Gaussian has 32 nonzero taps: 0, 17 and 34 vanish
    assert len(box3d_ref.TAPS) == 32
    assert sorted(set(range(-17, 18)) - set(box3d_ref.OFFS.tolist())) == [-17, 0, 17]


def test_detector_mirror_methods():
    from partsbaseddetector_amd import PartsBasedDetector
    from partsbaseddetector_amd.detector import Candidate
    rng = np.random.default_rng(3)
    for _ in range(50):
        parts = random_parts(rng, int(rng.integers(1, 12)), 80, 60).astype(np.int32)
        c = Candidate(parts, np.zeros(len(parts), np.float32), 0)
        assert c.boundingBoxNorm() == box3d_ref.bounding_box_norm(parts)
        assert c.boundingBox() == box3d_ref.bounding_box(parts)
    det = PartsBasedDetector()
    assert det._camera is None
    det.setBoundingBoxes3D((500.0, 500.0, 320.0, 240.0))
    assert det._camera.fx == 500.0 and det._camera.tx == 0.0
    det.setBoundingBoxes3D(None)
    assert det._camera is None
    assert callable(det.computeBoundingBoxes)


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"\b(pbd_[a-z0-9_]+)\s*\(", hdr))
    tune = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libpbd_hip_tune.so"))
    for name in NAMES:
        assert name in declared
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name) and hasattr(tune, name)
    for m in ("set_box3d", "get_box3d", "candidates_box3d"):
        assert hasattr(capi.Handle, m)
    assert capi.lib().pbd_abi_version() == 5 == capi.PBD_ABI_VERSION


def test_struct_layouts():
    assert C.sizeof(capi.pbd_camera) == 48
    assert [getattr(capi.pbd_camera, f).offset for f in ("fx", "fy", "cx", "cy", "tx", "ty")] == [0, 8, 16, 24, 32, 40]
    assert C.sizeof(capi.pbd_box3d) == 80 == capi.BOX3D_DTYPE.itemsize
    offs = {f: getattr(capi.pbd_box3d, f).offset for f, _ in capi.pbd_box3d._fields_}
    assert offs == {"valid": 0, "x": 4, "y": 8, "width": 12, "height": 16, "zmin": 20, "zmax": 24, "reserved": 28,
                    "x3d": 32, "y3d": 40, "z3d": 48, "width3d": 56, "height3d": 64, "depth3d": 72}
    assert all(capi.BOX3D_DTYPE.fields[f][1] == o for f, o in offs.items())
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    assert "double fx, fy, cx, cy, tx, ty;" in hdr
    src = open(os.path.join(ROOT, "partsbaseddetector_amd", "csrc", "pbd_api.cpp")).read()
    assert 'static_assert(sizeof(pbd_box3d) == 80' in src and 'static_assert(sizeof(pbd_camera) == 48' in src


def test_argument_errors_before_any_hip_call():
    L = capi.lib()
    cam = capi.camera(CAM)
    heads = (capi.pbd_candidate_head * 1)()
    boxes = (C.c_int32 * 64)()
    out = (capi.pbd_box3d * 1)()
    cnt = C.c_int(-1)
    for bad in (None, C.byref(cam)):
        assert L.pbd_set_box3d(None, 1, bad) == capi.PBD_ERR_ARG
        assert L.pbd_candidates_box3d(None, bad, None, capi.PBD_DEPTH_32F, 0, 0, 0, 4, 4, heads, boxes, 1, out, None) == capi.PBD_ERR_ARG
    assert L.pbd_get_box3d(None, 0, out, None, 1, C.byref(cnt)) == capi.PBD_ERR_ARG
    assert cnt.value == -1
    assert capi.camera((1.0, 2.0, 3.0, 4.0)).ty == 0.0
