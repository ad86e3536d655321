"""3-D bounding boxes on the device (k_box3d.hip) against tests/box3d_ref.py: zmin, zmax, valid, the image-space cube and the
projected Rect3d bit for bit; part centres bit for bit where every summation order is exact, else within 1e-12.

Whole paths are checked against pbd_candidates_box3d of the records the same frame returned."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_person_model, make_tree_model
from tests import box3d_ref

pytestmark = pytest.mark.gpu

W, H = 640, 480
CAM = (525.0, 523.5, 319.5, 239.5, 0.0, 0.0)
FIELDS = ("zmin", "zmax", "x3d", "y3d", "z3d", "width3d", "height3d", "depth3d")


def same_float(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b))))


def assert_boxes(got, exp, what=""):
    assert len(got) == len(exp), what
    for f in ("valid", "x", "y", "width", "height"):
        assert np.array_equal(got[f], exp[f]), (what, f)
    for f in FIELDS:
        bad = ~((got[f] == exp[f]) | (np.isnan(got[f]) & np.isnan(exp[f])))
        assert not bad.any(), (what, f, np.flatnonzero(bad)[:5], got[f][bad][:5], exp[f][bad][:5])


def assert_centres(got, exp, exact, what=""):
    if exact:
        assert same_float(got, exp), what
    else:
        np.testing.assert_allclose(got, exp, rtol=1e-12, atol=1e-300, err_msg=str(what))


def scene(seed, w, hgt, dtype=np.float32, quantised=False, kind="planes"):
    """planes with noise and holes (0); quantised: multiples of 2^-10, where every double sum is exact"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:hgt, 0:w].astype(np.float64)
    d = 3.0 + 0.002 * yy
    d = np.where(xx < w * 0.4, 1.2 + 0.0005 * xx, d)
    d = np.where((yy > hgt * 0.6) & (xx > w * 0.5), 2.0 + 0.001 * (xx - w * 0.5), d)
    d = d + rng.normal(0, 0.01, d.shape)
    d[rng.random(d.shape) < 0.05] = 0.0
    if kind == "holes":
        d[:] = 0.0
    elif kind == "special":
        d[rng.random(d.shape) < 0.05] = np.nan
        d[rng.random(d.shape) < 0.01] = np.inf
        d[rng.random(d.shape) < 0.01] = -np.inf
        d[rng.random(d.shape) < 0.02] = -1.5
    if quantised:
        d = np.round(d * 1024.0) / 1024.0
    return d.astype(dtype)


def records(seed, n, mp, im_w, im_h, big=90, whole=0.05):
    rng = np.random.default_rng(seed)
    heads = np.zeros(n, capi.HEAD_DTYPE)
    heads["nparts"] = np.where(rng.random(n) < 0.1, 1, rng.integers(1, mp + 1, n))
    heads["score"] = rng.normal(0, 1, n)
    boxes = np.zeros((n, mp, 4), np.int32)
    cx, cy = rng.integers(-20, im_w + 20, n), rng.integers(-20, im_h + 20, n)
    boxes[..., 0] = cx[:, None] + rng.integers(-big, big, (n, mp))
    boxes[..., 1] = cy[:, None] + rng.integers(-big, big, (n, mp))
    boxes[..., 2] = rng.integers(1, 40, (n, mp))
    boxes[..., 3] = rng.integers(1, 40, (n, mp))
    wh = rng.random(n) < whole
    boxes[wh, :, 0], boxes[wh, :, 1], boxes[wh, :, 2], boxes[wh, :, 3] = -2, -2, im_w + 4, im_h + 4
    return heads, boxes


@pytest.fixture(scope="module")
def handles():
    m = make_person_model()
    hs = {dt: capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, dtype=dt) for dt in (np.float32, np.float64)}
    yield hs
    for h in hs.values():
        h.close()


# ---- the stand-alone primitive --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dsize", [(640, 480), (320, 240), (501, 371)])
@pytest.mark.parametrize("kind", ["planes", "holes", "special"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_primitive_matches_restatement(gpu_required, handles, dsize, kind, dt):
    h = handles[dt]
    heads, boxes = records(sum(dsize) + len(kind), 32, h.max_parts, W, H, whole=0.03 if kind == "planes" else 0.0)
    for quantised in (True, False):
        depth = scene(7, *dsize, dtype=dt, quantised=quantised, kind=kind)
        got, gc = h.candidates_box3d(heads, boxes, depth, W, H, CAM)
        exp, ec = box3d_ref.box3d(heads, boxes, depth, W, H, CAM, h.max_parts)
        assert_boxes(got, exp, (dsize, kind, quantised))
        assert_centres(gc, ec, quantised or kind == "holes", (dsize, kind, quantised))
        if kind == "planes":
            assert got["valid"].sum() > len(got) // 2
        if kind == "holes":
            assert not got["valid"].any()


def test_primitive_point_counts_and_edges(gpu_required, handles):
    """N = 1, 399, 400, 401 and beyond, single-part records, a depth map of another aspect, an empty depth map"""
    h = handles[np.float32]
    rng = np.random.default_rng(2)
    depth = np.zeros((60, 80), np.float32)
    depth.ravel()[:4000] = rng.uniform(0.5, 3.0, 4000)
    heads = np.zeros(6, capi.HEAD_DTYPE)
    heads["nparts"] = 1
    boxes = np.zeros((6, h.max_parts, 4), np.int32)
    for i, n in enumerate((1, 2, 399, 400, 401, 1000)):
        d = np.zeros_like(depth)
        d.ravel()[:n] = depth.ravel()[:n]
        boxes[i, 0] = (0, 0, 80, (n + 79) // 80)
        got, _ = h.candidates_box3d(heads[i:i + 1], boxes[i:i + 1], d, 80, 60, CAM)
        exp, _ = box3d_ref.box3d(heads[i:i + 1], boxes[i:i + 1], d, 80, 60, CAM, h.max_parts)
        assert_boxes(got, exp, n)
        assert got["valid"][0]
    got, gc = h.candidates_box3d(heads, boxes, None, 80, 60, CAM)
    assert not got["valid"].any() and not gc.any()


def test_primitive_large_records(gpu_required, handles):
    """full-frame boxes on a 1920x1080 depth map: (nparts + 1) * dw * dh keys per record, far beyond any LDS tile"""
    h = handles[np.float32]
    w, hgt = 1920, 1080
    depth = scene(9, w, hgt, quantised=True)
    heads = np.zeros(2, capi.HEAD_DTYPE)
    heads["nparts"] = h.max_parts
    boxes = np.zeros((2, h.max_parts, 4), np.int32)
    boxes[0] = (-5, -5, w + 10, hgt + 10)
    boxes[1, :, 0] = np.arange(h.max_parts) * 40
    boxes[1, :, 1] = np.arange(h.max_parts) * 20
    boxes[1, :, 2] = w
    boxes[1, :, 3] = hgt
    got, gc = h.candidates_box3d(heads, boxes, depth, w, hgt, CAM)
    exp, ec = box3d_ref.box3d(heads, boxes, depth, w, hgt, CAM, h.max_parts)
    assert_boxes(got, exp, "1080p")
    assert_centres(gc, ec, True, "1080p")
    assert got["valid"].all()


def test_primitive_errors(gpu_required, handles):
    h = handles[np.float32]
    heads, boxes = records(1, 4, h.max_parts, W, H)
    depth = scene(1, W, H)
    for cam in ((0.0, 500.0, 1.0, 1.0), (500.0, 0.0, 1.0, 1.0), (np.nan, 500.0, 1.0, 1.0), (500.0, 500.0, np.inf, 1.0)):
        with pytest.raises(capi.PbdError) as e:
            h.candidates_box3d(heads, boxes, depth, W, H, cam)
        assert e.value.code == capi.PBD_ERR_ARG
    for iw, ih in ((0, H), (W, -1)):
        with pytest.raises(capi.PbdError) as e:
            h.candidates_box3d(heads, boxes, depth, iw, ih, CAM)
        assert e.value.code == capi.PBD_ERR_ARG
    bad = heads.copy()
    bad["nparts"][2] = h.max_parts + 1
    with pytest.raises(capi.PbdError) as e:
        h.candidates_box3d(bad, boxes, depth, W, H, CAM)
    assert e.value.code == capi.PBD_ERR_ARG
    bad["nparts"][2] = 0
    with pytest.raises(capi.PbdError) as e:
        h.candidates_box3d(bad, boxes, depth, W, H, CAM)
    assert e.value.code == capi.PBD_ERR_ARG
    with pytest.raises(capi.PbdError) as e:
        h.candidates_box3d(heads, boxes, depth.astype(np.uint16), W, H, CAM, depth_dtype=np.uint16)
    assert e.value.code == capi.PBD_ERR_UNSUPPORTED
    L = capi.lib()
    out = (capi.pbd_box3d * 4)()
    assert L.pbd_candidates_box3d(h.h, None, None, capi.PBD_DEPTH_32F, 0, 0, 0, W, H, heads.ctypes.data_as(C.c_void_p),
                                  boxes.ctypes.data_as(C.c_void_p), 4, out, None) == capi.PBD_ERR_ARG


# ---- whole paths --------------------------------------------------------------------------------------------------------
def bench_threshold(model, w, hgt, dtype=np.float32):
    """bench.py's threshold: the 99.9th percentile of component 0's root scores of the seed frame."""
    model.thresh = 3.0e38
    h = capi.Handle(model, dtype=dtype)
    h.detect(make_image(0, w, hgt))
    h._geo = h.geometry(w, hgt)
    vals = np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])])
    h.close()
    return float(np.float32(np.percentile(vals, 99.9)))


@pytest.fixture(scope="module")
def person():
    m = make_person_model()
    m.thresh = bench_threshold(m, W, H)
    return m


def expect(h, res, depth, w=W, hgt=H):
    """pbd_candidates_box3d of the records a frame returned"""
    heads, boxes, _ = res
    if len(heads) == 0:
        return np.zeros(0, capi.BOX3D_DTYPE), np.zeros((0, h.max_parts, 3))
    return h.candidates_box3d(heads, boxes, depth, w, hgt, CAM)


def assert_frame(h, res, depth, frame=0, what=""):
    got, gc = h.get_box3d(frame)
    exp, ec = expect(h, res, depth)
    assert_boxes(got, exp, what)
    assert same_float(gc, ec), what
    return got


def state_error(h, frame=0):
    with pytest.raises(capi.PbdError) as e:
        h.get_box3d(frame)
    return e.value.code == capi.PBD_ERR_STATE


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_frame_paths(gpu_required, person, dtype):
    import torch
    im = make_image(1, W, H)
    depth = scene(1, W, H, dtype)
    h = capi.Handle(person, dtype=dtype)
    raw = h.detect(im)
    assert len(raw[0]) > 20
    assert state_error(h)                          # plain frame
    h.detect_rgbd(im, depth)
    assert state_error(h)                          # setting off
    h.set_box3d(True, CAM)
    res = h.detect_rgbd(im, depth)
    assert res[0].tobytes() == raw[0].tobytes() and np.array_equal(res[1], raw[1])   # records unchanged
    got = assert_frame(h, res, depth, what="raw")
    assert got["valid"].sum() > len(got) // 2
    assert state_error(h, 1)
    for zf in (None, 0.03):
        if zf is not None:
            h.set_depth_filter(True, zf)
        for mode, ov in ((capi.PBD_CAND_RAW, 0.0), (capi.PBD_CAND_SORT_NMS, 0.1), (capi.PBD_CAND_SORT, 0.0)):
            h.set_candidate_filter(mode, ov)
            res = h.detect_rgbd(im, depth)
            assert_frame(h, res, depth, what=(zf, mode))
    d_im = torch.from_numpy(im).cuda()
    d_z = torch.from_numpy(depth).cuda()
    h.enqueue_rgbd_dev(d_im.data_ptr(), W, H, 3, d_z.data_ptr())
    assert state_error(h)                          # pending
    res = h.collect()
    assert_frame(h, res, depth, what="device")
    h.detect(im)
    assert state_error(h)                          # a plain frame in between
    h.set_box3d(False)
    h.detect_rgbd(im, depth)
    assert state_error(h)
    h.close()


@pytest.mark.parametrize("clusters", [False, True], ids=["box3d", "cluster3d"])
def test_stage_entry_after_rgbd_frame_computes_no_boxes(gpu_required, person, clusters):
    """pbd_dp_argmin on the plan an RGB-D frame left: a frame of its own that computes neither boxes nor clusters, so the getters
    answer PBD_ERR_STATE (include/pbd_c.h) instead of the RGB-D frame's results mapped onto other records; its records are a fresh
    handle's staged ones; the next RGB-D frame on the handle returns the first one's boxes again, in bits"""
    im = make_image(1, W, H)
    depth = scene(1, W, H)
    h = capi.Handle(person)
    h.set_box3d(True, CAM)
    if clusters:
        h.set_cluster3d(True)
    res = h.detect_rgbd(im, depth)
    assert len(res[0]) > 20
    boxes = assert_frame(h, res, depth, what="first")
    centres = h.get_box3d(0)[1]
    cl = h.get_cluster3d(0) if clusters else None
    staged = h.dp_argmin()
    assert state_error(h)
    if clusters:
        with pytest.raises(capi.PbdError) as e:
            h.get_cluster3d(0)
        assert e.value.code == capi.PBD_ERR_STATE
    fresh = capi.Handle(person)
    fresh.pyramid(im); fresh.pdf(); fresh.dp_min()
    exp = fresh.dp_argmin()
    fresh.close()
    assert len(staged[0]) == len(exp[0]) == len(res[0])
    for k in range(3):
        assert np.asarray(staged[k]).tobytes() == np.asarray(exp[k]).tobytes(), k
    again = h.detect_rgbd(im, depth)
    for k in range(3):
        assert np.asarray(again[k]).tobytes() == np.asarray(res[k]).tobytes(), k
    b2, c2 = h.get_box3d(0)
    assert_boxes(b2, boxes, "again")
    assert same_float(c2, centres) and all(same_float(b2[f], boxes[f]) for f in FIELDS)
    if clusters:
        cl2 = h.get_cluster3d(0)
        assert all(same_float(cl2[0][f], cl[0][f]) for f in cl[0].dtype.names) and np.array_equal(cl2[1], cl[1])
    h.close()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("nb", [1, 4])
def test_batches(gpu_required, person, graph, nb):
    import torch
    ims = [make_image(10 + f, W, H) for f in range(nb)]
    depths = [scene(20 + f, W, H) for f in range(nb)]
    h = capi.Handle(person, graph=graph)
    h.detect_batch(ims)
    h.detect_batch(ims)
    h.set_box3d(True, CAM)
    for zf, mode in ((None, capi.PBD_CAND_RAW), (0.03, capi.PBD_CAND_SORT_NMS), (None, capi.PBD_CAND_SORT_NMS)):
        h.set_depth_filter(zf is not None, 0.03)
        h.set_candidate_filter(mode, 0.1)
        for f, res in enumerate(h.detect_batch_rgbd(ims, depths)):
            assert_frame(h, res, depths[f], f, ("host", zf, mode, f))
        some = [d if f % 2 == 0 else None for f, d in enumerate(depths)]
        for f, res in enumerate(h.detect_batch_rgbd(ims, some)):
            if f % 2 == 0:
                assert_frame(h, res, depths[f], f, ("some NULL", f))
            elif nb > 1:
                assert state_error(h, f)
        d_ims = torch.from_numpy(np.stack(ims)).cuda()
        d_zs = torch.from_numpy(np.stack(depths)).cuda()
        h.enqueue_batch_rgbd_dev(d_ims.data_ptr(), d_zs.data_ptr(), nb, W, H, 3)
        for f, res in enumerate(h.collect_batch()):
            assert_frame(h, res, depths[f], f, ("device", zf, mode, f))
    h.detect_batch(ims)
    assert state_error(h)
    h.close()


def test_group_member_refused(gpu_required):
    m = make_tree_model([-1, 0, 1, 1, 0], 3, seed=5)
    g = capi.Group(m, [0, 0])
    L = capi.lib()
    mem = C.c_void_p(L.pbd_group_member(g.g, 0))
    cam = capi.camera(CAM)
    assert L.pbd_set_box3d(mem, 1, C.byref(cam)) == capi.PBD_ERR_UNSUPPORTED
    out = (capi.pbd_box3d * 1)()
    cnt = C.c_int(0)
    assert L.pbd_get_box3d(mem, 0, out, None, 1, C.byref(cnt)) == capi.PBD_ERR_UNSUPPORTED
    g.close()


def test_detector_mirror(gpu_required, person):
    from partsbaseddetector_amd import PartsBasedDetector
    im = make_image(6, W, H)
    depth = scene(6, W, H)
    det = PartsBasedDetector()
    det.setBoundingBoxes3D(CAM)
    det.distributeModel(person)
    got = det.detect(im, depth)
    assert len(got) > 0 and all(c.box3d is not None for c in got)
    rects, centres = det.computeBoundingBoxes(im.shape, depth, got, CAM)
    for c, r, ce in zip(got, rects, centres):
        if c.box3d["valid"]:
            assert same_float([c.box3d[k] for k in ("x3d", "y3d", "z3d", "width3d", "height3d", "depth3d")], r)
            assert same_float(c.part_centers, ce)
        else:
            assert r == (0.0,) * 6 and len(ce) == 0 and len(c.part_centers) == 0
    from partsbaseddetector_amd.detector import Candidate
    heads, boxes, _ = Candidate._pack(got)
    exp, _ = box3d_ref.box3d(heads, boxes, depth, W, H, CAM)
    assert_boxes(np.array([c.box3d for c in got]), exp, "mirror vs restatement")
    det.setBoundingBoxes3D(None)
    assert all(c.box3d is None for c in det.detect(im, depth))
