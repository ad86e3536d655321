"""Object clusters on the device (k_cluster3d.hip) against tests/cluster3d_ref.py: cropped, nclusters, size, first and the kept
clusters' indices exactly; centroids bit for bit on quantised scenes (every double sum exact), else within rtol 1e-12.

The in-frame step is checked against pbd_candidates_cluster3d on the numpy cloud of the frame's depth and the frame's own
pbd_get_box3d boxes."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_person_model, make_tree_model
from tests import cluster3d_ref as ref

pytestmark = pytest.mark.gpu

W, H = 640, 480
CAM = (525.0, 523.5, 319.5, 239.5, 0.0, 0.0)
F32 = np.float32


def rgbd_scene(seed, w=W, hgt=H, dtype=np.float32, quantised=False, special=True):
    """a wall at 2.5 m, blobs in front of it (pairs of blobs 5 and 6 pixels apart at 1 m: 9.5 mm and 11.4 mm, just under and just
    over 1 cm), 1 mm noise, holes, and NaN / inf / negative pixels"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:hgt, 0:w].astype(np.float64)
    d = 2.5 + 0.0004 * xx
    for k in range(6):
        cx, cy, r = rng.uniform(0.15, 0.85) * w, rng.uniform(0.15, 0.85) * hgt, rng.uniform(0.03, 0.08) * w
        d = np.where((xx - cx) ** 2 + (yy - cy) ** 2 < r * r, rng.uniform(1.0, 2.0), d)
    sx, sy = int(w * 0.3), int(hgt * 0.2)
    for gap, row in ((5, 0), (6, 25)):   # two 12 x 12 squares at 1 m, `gap` pixels apart
        d[sy + row:sy + row + 12, sx:sx + 12] = 1.0
        d[sy + row:sy + row + 12, sx + 12 + gap - 1:sx + 24 + gap - 1] = 1.0
    d = d + rng.normal(0, 0.001, d.shape) * (d != 1.0)
    d[rng.random(d.shape) < 0.04] = 0.0
    if special:
        d[rng.random(d.shape) < 0.01] = np.nan
        d[rng.random(d.shape) < 0.005] = np.inf
        d[rng.random(d.shape) < 0.005] = -np.inf
        d[rng.random(d.shape) < 0.005] = -0.8
    if quantised:
        d = np.round(d * 1024.0) / 1024.0
    return d.astype(dtype)


def boxes_around(cloud, seed, n):
    """n boxes: around random pixel windows' points, whole-cloud, skipped and degenerate ones"""
    rng = np.random.default_rng(seed)
    hgt, w = cloud.shape[:2]
    out = np.zeros(n, capi.BOX3D_DTYPE)
    for i in range(n):
        k = i % 8
        if k == 6:
            continue                                                   # skipped record: all zeros
        if k == 7:
            out[i]["x3d"], out[i]["width3d"], out[i]["height3d"], out[i]["depth3d"] = 0.1, -1.0, 1.0, 1.0   # negative volume
            continue
        x0, y0 = int(rng.integers(0, w - 8)), int(rng.integers(0, hgt - 8))
        x1, y1 = min(w, x0 + int(rng.integers(8, w // 3))), min(hgt, y0 + int(rng.integers(8, hgt // 3)))
        p = cloud[y0:y1, x0:x1].reshape(-1, 3)
        p = p[np.all(np.isfinite(p), axis=1)]
        if len(p) == 0 or k == 5:
            lo, hi = np.array([-3.0, -3.0, -3.0]), np.array([3.0, 3.0, 3.0])
        else:
            lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
            hi[2] = lo[2] + (hi[2] - lo[2]) * rng.uniform(0.3, 1.0)
        out[i]["x3d"], out[i]["y3d"], out[i]["z3d"] = lo
        out[i]["width3d"], out[i]["height3d"], out[i]["depth3d"] = hi - lo
        out[i]["valid"] = 1
    return out


def assert_clusters(got, exp, exact, what=""):
    (g, gi), (e, ei) = got, exp
    assert len(g) == len(e), what
    for f in ("cropped", "nclusters", "size", "first"):
        bad = g[f] != e[f]
        assert not bad.any(), (what, f, np.flatnonzero(bad)[:5], g[f][bad][:5], e[f][bad][:5])
    assert np.array_equal(gi, ei), what
    for f in ("cx", "cy", "cz"):
        assert np.array_equal(np.isnan(g[f]), np.isnan(e[f])), (what, f)
        ok = ~np.isnan(e[f])
        if exact:
            assert np.array_equal(g[f][ok], e[f][ok]), (what, f)
        else:
            np.testing.assert_allclose(g[f][ok], e[f][ok], rtol=1e-12, atol=0, err_msg=str((what, f)))


@pytest.fixture(scope="module")
def handle():
    h = capi.Handle(make_tree_model([-1, 0, 1, 1, 0], 3, seed=5))
    yield h
    h.close()


# ---- the stand-alone primitive --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantised", [True, False])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_rgbd_scene_matches_restatement(gpu_required, handle, quantised, dt):
    depth = rgbd_scene(3, dtype=dt, quantised=quantised)
    cloud = ref.depth_cloud(depth, CAM)
    boxes = boxes_around(cloud, 4, 48)
    got = handle.candidates_cluster3d(cloud, boxes)
    exp = ref.cluster_objects(cloud, boxes)
    assert_clusters(got, exp, quantised, (quantised, dt))
    assert (got[0]["size"] > 100).sum() > 10 and (got[0]["nclusters"] > 1).sum() > 5


def test_gap_just_under_and_over_tol(gpu_required, handle):
    depth = np.zeros((H, W), np.float32)
    sx, sy = int(W * 0.3), int(H * 0.2)
    for gap, row in ((5, 0), (6, 25)):
        depth[sy + row:sy + row + 12, sx:sx + 12] = 1.0
        depth[sy + row:sy + row + 12, sx + 12 + gap - 1:sx + 24 + gap - 1] = 1.0
    cloud = ref.depth_cloud(depth, CAM)
    boxes = np.zeros(2, capi.BOX3D_DTYPE)
    for i, row in enumerate((0, 25)):
        p = cloud[sy + row:sy + row + 12, sx:sx + 40].reshape(-1, 3)
        p = p[np.all(np.isfinite(p), axis=1)]
        lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64) + [0, 0, 0.01]
        boxes[i]["x3d"], boxes[i]["y3d"], boxes[i]["z3d"] = lo
        boxes[i]["width3d"], boxes[i]["height3d"], boxes[i]["depth3d"] = hi - lo
    got = handle.candidates_cluster3d(cloud, boxes)
    assert_clusters(got, ref.cluster_objects(cloud, boxes), False)
    assert list(got[0]["nclusters"]) == [1, 2] and list(got[0]["size"]) == [288, 144]


def test_d2_boundary_and_ties(gpu_required, handle):
    """tol 2^-4 on a 2^-6 grid: d2 == r2 joins; two equal largest clusters: the one with the smallest index wins"""
    s = 2.0 ** -6
    cloud = np.full((4, 8, 3), np.nan, F32)
    pts = np.array([[13, 0, 0], [0, 0, 0], [4, 0, 0], [13, 4, 0], [8, 0, 0], [13, 4, 4], [20, 4, 4], [23, 5, 4]], np.float64) * s
    for k, p in enumerate(pts):
        cloud[1 + k // 8 * 2, k % 8] = p
    b = np.zeros(3, capi.BOX3D_DTYPE)
    b[0]["width3d"] = b[0]["height3d"] = b[0]["depth3d"] = 0.5
    b[1] = b[0]; b[1]["x3d"] = 3 * s
    b[2] = b[0]; b[2]["x3d"], b[2]["width3d"] = 0.5, -0.5
    for tol in (0.0625, float(np.nextafter(F32(0.0625), F32(0)))):
        got = handle.candidates_cluster3d(cloud, b, tol)
        assert_clusters(got, ref.cluster_objects(cloud, b, tol), True, tol)
    got = handle.candidates_cluster3d(cloud, b, 0.0625)
    assert got[0]["nclusters"][0] == 3 and got[0]["size"][0] == 3 and got[0]["first"][0] == 8 + 0   # row 0 col 0 of the cloud
    res, idx = handle.candidates_cluster3d(cloud, b, 1e20)   # r2 = inf: one cluster
    assert res["nclusters"][0] == 1 and res["size"][0] == 8


def test_empty_skipped_degenerate(gpu_required, handle):
    cloud = ref.depth_cloud(rgbd_scene(5, 64, 48), CAM)
    b = np.zeros(6, capi.BOX3D_DTYPE)
    b[1]["width3d"], b[1]["height3d"], b[1]["depth3d"] = 1e-6, 1.0, 1.0          # volume exactly 1e-6: kept
    b[2]["width3d"], b[2]["height3d"], b[2]["depth3d"] = np.nextafter(1e-6, 0), 1.0, 1.0
    b[3]["x3d"], b[3]["width3d"], b[3]["height3d"], b[3]["depth3d"] = 5.0, -10.0, -10.0, 10.0   # min > max on x, y
    b[4]["z3d"], b[4]["width3d"], b[4]["height3d"], b[4]["depth3d"] = 100.0, 1.0, 1.0, 1.0     # nothing inside
    b[5]["x3d"] = b[5]["y3d"] = b[5]["z3d"] = -1e39
    b[5]["width3d"] = b[5]["height3d"] = b[5]["depth3d"] = 2e39                            # min / max at +-inf
    got = handle.candidates_cluster3d(cloud, b)
    assert_clusters(got, ref.cluster_objects(cloud, b), False)
    assert list(got[0]["cropped"][[0, 2, 3, 4]]) == [0, 0, 0, 0] and got[0]["cropped"][5] > 1000
    res, idx = handle.candidates_cluster3d(np.zeros((0, 0, 3), F32), b)
    assert not res["cropped"].any() and len(idx) == 0 and np.isnan(res["cx"]).all() and (res["first"] == -1).all()
    res, idx = handle.candidates_cluster3d(cloud, np.zeros(0, capi.BOX3D_DTYPE))
    assert len(res) == 0 and len(idx) == 0


@pytest.mark.parametrize("ps,pad", [(12, 0), (16, 0), (32, 0), (16, 48), (32, 8)])
def test_point_and_row_strides(gpu_required, handle, ps, pad):
    cloud = ref.depth_cloud(rgbd_scene(6, 160, 120, quantised=True), CAM)
    ch, cw = cloud.shape[:2]
    rs = cw * ps + pad
    buf = np.full((ch, rs), 0xAB, np.uint8)
    v = buf.reshape(-1)
    for r in range(ch):
        row = np.frombuffer(v[r * rs:r * rs + cw * ps].tobytes(), np.uint8).reshape(cw, ps).copy()
        row[:, :12] = cloud[r].astype(F32).view(np.uint8).reshape(cw, 12)
        v[r * rs:r * rs + cw * ps] = row.reshape(-1)
    boxes = boxes_around(cloud, 7, 24)
    got = handle.cluster3d_raw(buf, cw, ch, ps, rs, boxes)
    assert_clusters(got, ref.cluster_objects(cloud, boxes), True, (ps, pad))


def test_thousand_records(gpu_required, handle):
    depth = rgbd_scene(8, 160, 120)
    cloud = ref.depth_cloud(depth, (131.25, 130.9, 79.5, 59.5))
    boxes = boxes_around(cloud, 9, 1000)
    got = handle.candidates_cluster3d(cloud, boxes)
    assert_clusters(got, ref.cluster_objects(cloud, boxes), False)


def test_full_frame_1080p(gpu_required, handle):
    """one record over a whole 1920 x 1080 cloud (2 M points, quantised): scattered points and a 3 mm chain of 3 000"""
    rng = np.random.default_rng(10)
    w, hgt = 1920, 1080
    cloud = (rng.integers(0, 10 * 1024, (hgt, w, 3)) * 2.0 ** -10).astype(F32)
    cloud.reshape(-1, 3)[rng.random(w * hgt) < 0.01] = np.nan
    chain = np.zeros((3000, 3))
    chain[:, 0] = 1.0 + np.arange(3000) * 3 * 2.0 ** -10
    chain[:, 1] = chain[:, 2] = 4.0
    cloud.reshape(-1, 3)[np.sort(rng.choice(w * hgt, 3000, replace=False))] = chain.astype(F32)
    b = np.zeros(2, capi.BOX3D_DTYPE)
    b[0]["width3d"] = b[0]["height3d"] = b[0]["depth3d"] = 10.0
    b[1]["x3d"], b[1]["y3d"], b[1]["z3d"] = 0.9, 3.9, 3.9
    b[1]["width3d"], b[1]["height3d"], b[1]["depth3d"] = 9.0, 0.2, 0.2
    got = handle.candidates_cluster3d(cloud, b)
    exp = ref.cluster_objects(cloud, b)
    assert_clusters(got, exp, True)
    assert got[0]["size"][0] >= 3000 and got[0]["cropped"][0] > 2_000_000


def test_errors_and_capacity(gpu_required, handle):
    L = capi.lib()
    cloud = ref.depth_cloud(rgbd_scene(11, 64, 48), CAM)
    boxes = boxes_around(cloud, 12, 8)
    out = np.zeros(8, capi.CLUSTER3D_DTYPE)
    tot = C.c_int(-1)
    cp, bp, op = cloud.ctypes.data_as(C.c_void_p), boxes.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def call(cloud_p=cp, cw=64, ch=48, ps=12, rs=64 * 12, tol=0.01, idx=None, cap=0, count=8):
        return L.pbd_candidates_cluster3d(handle.h, cloud_p, cw, ch, ps, rs, bp, count, C.c_float(tol), op, idx, cap, C.byref(tot))

    for tol in (0.0, -0.01, float("nan"), float("inf")):
        assert call(tol=tol) == capi.PBD_ERR_ARG
    assert call(ps=8) == capi.PBD_ERR_ARG
    assert call(ps=14, rs=64 * 14) == capi.PBD_ERR_ARG
    assert call(rs=63 * 12) == capi.PBD_ERR_ARG
    assert call(cloud_p=None) == capi.PBD_ERR_ARG
    assert call(cw=-1) == capi.PBD_ERR_ARG
    assert call(cloud_p=None, cw=0, ch=0) == capi.PBD_OK and tot.value == 0
    assert call() == capi.PBD_OK
    res, idx = ref.cluster_objects(cloud, boxes)
    assert tot.value == len(idx) > 10
    small = np.zeros(len(idx) - 1, np.int32)
    tot.value = -1
    assert call(idx=small.ctypes.data_as(C.c_void_p), cap=len(small)) == capi.PBD_ERR_CAPACITY and tot.value == len(idx)
    full = np.zeros(len(idx), np.int32)
    assert call(idx=full.ctypes.data_as(C.c_void_p), cap=len(full)) == capi.PBD_OK and np.array_equal(full, idx)
    assert L.pbd_set_cluster3d(handle.h, 1, C.c_float(0.0)) == capi.PBD_ERR_ARG
    assert L.pbd_set_cluster3d(handle.h, 1, C.c_float(float("nan"))) == capi.PBD_ERR_ARG


# ---- the in-frame step ----------------------------------------------------------------------------------------------------
def bench_threshold(model, w, hgt, q=99.9):
    """bench.py's threshold: the 99.9th percentile of component 0's root scores of the seed frame."""
    model.thresh = 3.0e38
    h = capi.Handle(model)
    h.detect(make_image(0, w, hgt))
    h._geo = h.geometry(w, hgt)
    vals = np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])])
    h.close()
    return float(np.float32(np.percentile(vals, q)))


@pytest.fixture(scope="module")
def person():
    m = make_person_model()
    m.thresh = bench_threshold(m, W, H)
    return m


def assert_frame(h, depth, frame=0, what=""):
    b3, _ = h.get_box3d(frame)
    got = h.get_cluster3d(frame)
    cloud = ref.depth_cloud(depth, CAM)
    exp = h.candidates_cluster3d(cloud, b3)
    assert_clusters(got, exp, False, what)
    return got


def state_error(h, frame=0):
    with pytest.raises(capi.PbdError) as e:
        h.get_cluster3d(frame)
    return e.value.code == capi.PBD_ERR_STATE


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_frame_paths(gpu_required, person, dtype):
    import torch
    im = make_image(1, W, H)
    depth = rgbd_scene(1, dtype=dtype)
    h = capi.Handle(person, dtype=dtype)
    raw = h.detect(im)
    assert len(raw[0]) > 20
    h.set_box3d(True, CAM)
    res0 = h.detect_rgbd(im, depth)
    b30, c30 = h.get_box3d(0)
    assert state_error(h)                          # clusters off
    h.set_cluster3d(True, 0.01)
    res = h.detect_rgbd(im, depth)
    assert res[0].tobytes() == raw[0].tobytes() and np.array_equal(res[1], raw[1])   # records unchanged
    b3, c3 = h.get_box3d(0)
    assert b3.tobytes() == b30.tobytes() and c3.tobytes() == c30.tobytes()             # boxes unchanged
    got = assert_frame(h, depth, what="raw")
    assert (got[0]["size"] > 0).sum() > len(got[0]) // 2
    assert state_error(h, 1)
    for zf in (None, 0.03):
        h.set_depth_filter(zf is not None, 0.03)
        for mode, ov in ((capi.PBD_CAND_RAW, 0.0), (capi.PBD_CAND_SORT_NMS, 0.1)):
            h.set_candidate_filter(mode, ov)
            h.detect_rgbd(im, depth)
            assert_frame(h, depth, what=(zf, mode))
    d_im = torch.from_numpy(im).cuda()
    d_z = torch.from_numpy(depth).cuda()
    h.enqueue_rgbd_dev(d_im.data_ptr(), W, H, 3, d_z.data_ptr())
    assert state_error(h)                          # pending
    with pytest.raises(capi.PbdError):
        h.set_cluster3d(False)                     # (a frame is in flight)
    h.collect()
    assert_frame(h, depth, what="device")
    h.detect(im)
    assert state_error(h)                          # a plain frame in between
    h.set_cluster3d(False)
    h.detect_rgbd(im, depth)
    assert state_error(h)
    h.set_depth_filter(False)
    h.set_candidate_filter(capi.PBD_CAND_RAW, 0.0)
    assert h.detect(im)[0].tobytes() == raw[0].tobytes()
    h.close()


@pytest.mark.parametrize("nb", [1, 4])
def test_batches(gpu_required, person, nb):
    import torch
    ims = [make_image(10 + f, W, H) for f in range(nb)]
    depths = [rgbd_scene(20 + f) for f in range(nb)]
    h = capi.Handle(person)
    plain = h.detect_batch(ims)
    h.set_box3d(True, CAM)
    h.set_cluster3d(True)
    for zf, mode in ((None, capi.PBD_CAND_RAW), (0.03, capi.PBD_CAND_SORT_NMS), (None, capi.PBD_CAND_SORT_NMS)):
        h.set_depth_filter(zf is not None, 0.03)
        h.set_candidate_filter(mode, 0.1)
        for f, res in enumerate(h.detect_batch_rgbd(ims, depths)):
            assert_frame(h, depths[f], f, ("host", zf, mode, f))
        some = [d if f % 2 == 0 else None for f, d in enumerate(depths)]
        h.detect_batch_rgbd(ims, some)
        for f in range(nb):
            if f % 2 == 0:
                assert_frame(h, depths[f], f, ("some NULL", f))
            else:
                assert state_error(h, f)
        d_ims = torch.from_numpy(np.stack(ims)).cuda()
        d_zs = torch.from_numpy(np.stack(depths)).cuda()
        h.enqueue_batch_rgbd_dev(d_ims.data_ptr(), d_zs.data_ptr(), nb, W, H, 3)
        h.collect_batch()
        for f in range(nb):
            assert_frame(h, depths[f], f, ("device", zf, mode, f))
    h.set_depth_filter(False)
    h.set_candidate_filter(capi.PBD_CAND_RAW, 0.0)
    again = h.detect_batch(ims)
    assert all(a[0].tobytes() == b[0].tobytes() for a, b in zip(again, plain))
    assert state_error(h)
    h.close()


def test_pool_overflow_reruns(gpu_required):
    """a frame whose kept clusters need more than the pool holds: the collect runs those records again, results unchanged"""
    m = make_person_model()
    m.thresh = bench_threshold(m, W, H, 99.5)
    im = make_image(1, W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (1.5 + 0.001 * xx + 0.0005 * yy).astype(np.float32)   # one tilted wall: a record keeps about all of its box
    h = capi.Handle(m, max_candidates=32768)
    h.set_box3d(True, CAM)
    h.set_cluster3d(True)
    for _ in range(2):
        h.detect_rgbd(im, depth, 32768)
        got = assert_frame(h, depth, what="wall")
    assert got[0]["size"].sum() > 4 * W * H
    h.close()


def test_group_member_refused(gpu_required):
    m = make_tree_model([-1, 0, 1, 1, 0], 3, seed=5)
    g = capi.Group(m, [0, 0])
    L = capi.lib()
    mem = C.c_void_p(L.pbd_group_member(g.g, 0))
    assert L.pbd_set_cluster3d(mem, 1, C.c_float(0.01)) == capi.PBD_ERR_UNSUPPORTED
    out = (C.c_char * 40)()
    cnt, tot = C.c_int(0), C.c_int(0)
    assert L.pbd_get_cluster3d(mem, 0, out, 1, C.byref(cnt), None, 0, C.byref(tot)) == capi.PBD_ERR_UNSUPPORTED
    g.close()


def test_detector_mirror(gpu_required, person):
    from partsbaseddetector_amd import PartsBasedDetector
    im = make_image(6, W, H)
    depth = rgbd_scene(6)
    det = PartsBasedDetector()
    det.setBoundingBoxes3D(CAM)
    det.setObjectClusters(0.01)
    det.distributeModel(person)
    got = det.detect(im, depth)
    assert len(got) > 0 and all(c.cluster is not None and c.centre3d.shape == (3,) for c in got)
    clusters, centres = det.cluster_objects(ref.depth_cloud(depth, CAM), np.array([c.box3d for c in got]))
    for c, k, ce in zip(got, clusters, centres):
        assert np.array_equal(c.cluster, k)
        assert np.array_equal(np.isnan(c.centre3d), np.isnan(ce))
        np.testing.assert_allclose(c.centre3d[~np.isnan(ce)], ce[~np.isnan(ce)], rtol=1e-12)
    det.setObjectClusters(None)
    assert all(c.cluster is None and c.box3d is not None for c in det.detect(im, depth))
