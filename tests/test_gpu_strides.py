"""Row strides, ROI views and unaligned bases on every entry of include/pbd_c.h that takes an image or a depth image.

The reference of every case is the SAME entry on the packed copy of the frame (np.ascontiguousarray(view), or a packed device tensor);
the packed path is pinned to the oracle and the definitions by the rest of the suite.  Equality is in bits — heads.tobytes(), boxes,
locs, counts, and where a stage is read back every level image and every feature plane — and no tolerance appears anywhere.  The
frames, layouts and fills are tests/stride_cases.py's: what lies between the rows of a view (seeded noise; NaN, 0 and 1e6 around depth
images) differs between the two fills and must never reach a result."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from tests import stride_cases as sc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
ARG, STATE, OK = capi.PBD_ERR_ARG, capi.PBD_ERR_STATE, capi.PBD_OK
V, D = C.c_void_p, C.c_double
DEPTH_FRAME = "bgr100x75"                      # the frame of the RGB-D cases
ZF = {"planes": 1.0, "blobs": 0.3}             # zfactor per scene: the CPU restatement keeps 55 and 33 of this frame's 76 records


class Env:
    pass


@pytest.fixture(scope="module")
def env(gpu_required, orc):
    e = Env()
    e.model = sc.model()
    e.model.thresh = sc.threshold(orc, e.model)
    e.frames = sc.all_frames()
    e.h = {F32: capi.Handle(e.model), F64: capi.Handle(e.model, dtype=F64)}
    e.refs = {}
    yield e
    for h in e.h.values():
        h.close()


def geom(im):
    return im.shape[1], im.shape[0], 1 if im.ndim == 2 else im.shape[2]


def same(got, exp, what=""):
    """records, bit for bit"""
    assert len(got[0]) == len(exp[0]), (what, len(got[0]), len(exp[0]))
    assert got[0].tobytes() == exp[0].tobytes(), what
    assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]), what


def same_arrays(got, exp, what=""):
    assert len(got) == len(exp), what
    for i, (g, x) in enumerate(zip(got, exp)):
        g, x = np.asarray(g), np.asarray(x)
        assert g.shape == x.shape and g.dtype == x.dtype and g.tobytes() == x.tobytes(), (what, i)


def ref(e, dtype, name):
    """the packed frame's records on the shared handle of `dtype`: at least 20"""
    if (dtype, name) not in e.refs:
        e.refs[dtype, name] = e.h[dtype].detect(e.frames[name])
    r = e.refs[dtype, name]
    assert len(r[0]) >= sc.MIN_RECORDS, (name, len(r[0]))
    return r


def stage_planes(h):
    """every level image and feature plane after pyramid() / pyramid_image()"""
    return [a for l in range(h._geo["nlevels"]) for a in (h.level_image_raw(l), h.level_features(l))]


def plan_planes(h, im, imdtype=None):
    """the same of the frame the handle's plan holds (after a detect)"""
    w, hgt, cn = geom(im)
    dt = im.dtype if imdtype is None else imdtype
    return [a for l in range(h.geometry(w, hgt)["nlevels"]) for a in h.frame_planes(0, l, w, hgt, cn, dt)]


def truth_of(rec):
    """the part boxes (x, y, width, height) of the best record: a truth set its frame surely has a pose for"""
    i = int(np.argmax(rec[0]["score"]))
    return rec[1][i][:int(rec[0]["nparts"][i])].copy()


def gts_of(rec):
    """gt boxes (x1, y1, x2, y2): the extents of the best and the worst record, a fractional one and one far outside"""
    out = []
    for i in (int(np.argmax(rec[0]["score"])), int(np.argmin(rec[0]["score"]))):
        b = rec[1][i][:int(rec[0]["nparts"][i])].astype(np.float64)
        out.append([b[:, 0].min(), b[:, 1].min(), (b[:, 0] + b[:, 2]).max(), (b[:, 1] + b[:, 3]).max()])
    out += [[10.25, 8.5, 60.0, 55.75], [5000.0, 5000.0, 5100.0, 5200.0]]
    return np.asarray(out, np.float64)


def warp_boxes(w, hgt):
    """boxes (x1, y1, x2, y2), 1-based inclusive, that overhang every edge of the frame, cover it, and lie inside"""
    return np.asarray([(-5, 10, 30, 50), (10, -6, 50, 30), (w - 30, 20, w + 8, 60), (20, hgt - 30, 60, hgt + 7),
                       (-10, -10, w + 10, hgt + 10), (w - 12, hgt - 9, w + 3, hgt + 4), (-3, -3, 9, 7), (30, 20, 69, 59)], np.float64)


def device(parent):
    import torch
    return torch.from_numpy(parent).cuda()


def dev_ptr(t, view, parent):
    return t.data_ptr() + sc.offset_of(view, parent)


CASES = [(n, l) for n in sc.FRAMES for l in sc.LAYOUTS]
CASE_IDS = [f"{n}-{l}" for n, l in CASES]


# ---- host frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layout", CASES, ids=CASE_IDS)
def test_host_detect_entries(env, name, layout):
    """detect, enqueue + collect, enqueue_host_ptr, detect_image (8-bit), detect_latent, detect_gtbox and the pyramid behind them"""
    im = env.frames[name]
    w, hgt, cn = geom(im)
    h = env.h[F32]
    exp = ref(env, F32, name)
    truth, gts = truth_of(exp), gts_of(exp)
    lat, gt = h.detect_latent(im, truth, 0.5), h.detect_gtbox(im, gts, 0.3)
    assert len(lat[0]) == 1 and gt[3][:2].any() and not gt[3][3]
    h.detect(im)
    planes = plan_planes(h, im)
    for fill in sc.FILLS:
        view, _ = sc.embed(im, layout, fill)
        what = (name, layout, fill)
        same(h.detect(view), exp, what)
        same_arrays(plan_planes(h, im), planes, what)
        h.enqueue(view)
        same(h.collect(), exp, what)
        h.enqueue_host_ptr(view.ctypes.data, w, hgt, cn, stride=view.strides[0])
        same(h.collect(), exp, what)
        same(h.detect_image(view), exp, what)
        same(h.detect_latent(view, truth, 0.5), lat, what)
        same_arrays(h.detect_gtbox(view, gts, 0.3), gt, what)
    if layout in sc.OPTION_LAYOUTS:
        view, _ = sc.embed(im, layout, sc.FILLS[0])
        same(env.h[F64].detect(view), ref(env, F64, name), (name, layout, "double"))


@pytest.mark.parametrize("name,layout", CASES, ids=CASE_IDS)
def test_host_stage_and_primitive_entries(env, name, layout):
    """pyramid, pyramid_image, hog (float and double), resize, pyrdown"""
    im = env.frames[name]
    w, hgt, _ = geom(im)
    sizes = ((w * 3 // 4, hgt * 3 // 4), (w + 13, hgt + 9), (w, hgt))
    exp = {}
    for dt, h in env.h.items():
        h.pyramid(im)
        exp["pyr", dt] = stage_planes(h)
        h.pyramid_image(im)
        exp["pyri", dt] = stage_planes(h)
        exp["hog", dt] = h.hog(im)
    h = env.h[F32]
    exp["resize"] = [h.resize(im, ow, oh) for ow, oh in sizes]
    exp["pyrdown"] = h.pyrdown(im)
    same_arrays(exp["pyri", F32], exp["pyr", F32])
    for fill in sc.FILLS:
        view, _ = sc.embed(im, layout, fill)
        what = (name, layout, fill)
        for dt, hd in env.h.items():
            hd.pyramid(view)
            same_arrays(stage_planes(hd), exp["pyr", dt], what)
            hd.pyramid_image(view)
            same_arrays(stage_planes(hd), exp["pyri", dt], what)
            same_arrays([hd.hog(view)], [exp["hog", dt]], what)
        same_arrays([h.resize(view, ow, oh) for ow, oh in sizes], exp["resize"], what)
        same_arrays([h.pyrdown(view)], [exp["pyrdown"]], what)


@pytest.mark.parametrize("name,layout", CASES, ids=CASE_IDS)
def test_host_warped_positives(env, name, layout):
    """warp_windows (float and double) and QpCache.write_warped: the boxes overhang the frame, so a border replicated from the parent's
    neighbouring pixel instead of the ROI's edge pixel shows in the windows"""
    im = env.frames[name]
    w, hgt, _ = geom(im)
    boxes = warp_boxes(w, hgt)
    ids = np.arange(50, 50 + len(boxes), dtype=np.int32)
    exp = {dt: h.warp_windows(im, boxes, 1) for dt, h in env.h.items()}
    q = capi.QpCache(env.h[F32], len(boxes), 1.0, 1.0)
    assert q.write_warped(im, boxes, 1, 0, 0.0, ids)[0] == len(boxes)
    cols = q.get()
    q.close()
    for fill in sc.FILLS:
        view, _ = sc.embed(im, layout, fill)
        for dt, h in env.h.items():
            same_arrays(h.warp_windows(view, boxes, 1), exp[dt], (name, layout, fill, dt))
        q = capi.QpCache(env.h[F32], len(boxes), 1.0, 1.0)
        written, status = q.write_warped(view, boxes, 1, 0, 0.0, ids)
        assert written == len(boxes) and (status == capi.PBD_WARP_WRITTEN).all()
        same_arrays(q.get(), cols, (name, layout, fill))
        q.close()


@pytest.mark.parametrize("kind", list(sc.WIDE))
@pytest.mark.parametrize("layout", sc.WIDE_LAYOUTS)
def test_host_wide_depths(env, kind, layout):
    """detect_image and pyramid_image of 16-bit, float and double frames: the stride is in bytes"""
    im = env.frames[kind]
    for dt in (F32, F64):
        h = env.h[dt]
        exp = h.detect_image(im)
        assert len(exp[0]) >= sc.MIN_RECORDS
        h.pyramid_image(im)
        planes = stage_planes(h)
        for fill in sc.FILLS:
            view, _ = sc.embed(im, layout, fill)
            assert view.strides[0] % im.itemsize == 0 and view.strides[0] > 101 * 3 * im.itemsize
            same(h.detect_image(view), exp, (kind, layout, fill))
            h.pyramid_image(view)
            same_arrays(stage_planes(h), planes, (kind, layout, fill))


@pytest.mark.parametrize("layout", sc.LAYOUTS)
def test_tune_plan(env, layout):
    """pbd_tune_plan measures on the strided frame (its times are not compared); the records after it are the packed ones"""
    name = "bgr101x77"
    im = env.frames[name]
    h = capi.Handle(env.model)
    for fill in sc.FILLS:
        view, _ = sc.embed(im, layout, fill)
        chosen, ms = h.tune_plan(view)
        assert chosen in (1, 2) and min(ms) > 0
        same(h.detect(view), ref(env, F32, name), (layout, fill))
    assert h.tune_plan(sc.embed(im, layout, sc.FILLS[0])[0], batch=2)[0] in (1, 2)
    same(h.detect(im), ref(env, F32, name), layout)
    h.close()


def roi_batch(fill, cn=3):
    """four different 100 x 75 frames as four ROIs of one 320 x 240 parent of noise: one stride, four unaligned bases"""
    w, hgt = 100, 75
    parent = np.random.default_rng(fill).integers(0, 256, (240, 320, cn), dtype=np.uint8)
    frames = sc.batch_frames(cn)
    views = []
    for f, (x, y) in zip(frames, ((7, 5), (121, 3), (9, 101), (215, 160))):
        parent[y:y + hgt, x:x + w] = f
        views.append(parent[y:y + hgt, x:x + w])
    return frames, views


def test_host_batches(env):
    """detect_batch, detect_batch_latent, detect_batch_gtbox: four ROIs of one parent sharing one stride"""
    h = env.h[F32]
    frames, _ = roi_batch(0)
    exp = h.detect_batch(frames)
    assert all(len(r[0]) >= sc.MIN_RECORDS for r in exp)
    truths = [np.concatenate([truth_of(r), np.zeros((5 - len(truth_of(r)), 4), np.int32)]) for r in exp]
    gts = [gts_of(r) for r in exp]
    lat, gt = h.detect_batch_latent(frames, truths, 0.5), h.detect_batch_gtbox(frames, gts, 0.3)
    assert all(len(r[0]) == 1 for r in lat) and all(g[3][:2].any() for g in gt)
    for dt in (F32, F64):
        hd = env.h[dt]
        expd = exp if dt == F32 else hd.detect_batch(frames)
        for fill in sc.FILLS:
            _, views = roi_batch(fill)
            assert capi._frames(views)[1] == 960 and not views[0].flags["C_CONTIGUOUS"]
            for g, x in zip(hd.detect_batch(views), expd):
                same(g, x, (dt, fill))
            if dt == F32:
                for g, x in zip(h.detect_batch_latent(views, truths, 0.5), lat):
                    same(g, x, ("latent", fill))
                for g, x in zip(h.detect_batch_gtbox(views, gts, 0.3), gt):
                    same_arrays(g, x, ("gtbox", fill))


def test_groups(env):
    """Group([0, 0]).detect and .detect_batch"""
    g = capi.Group(env.model, [0, 0], gather=capi.PBD_GATHER_HOST)
    frames, _ = roi_batch(0)
    exp = g.detect_batch(frames)
    for r, x in zip(exp, env.h[F32].detect_batch(frames)):
        same(r, x, "group vs handle")
    assert all(len(r[0]) >= sc.MIN_RECORDS for r in exp)
    for fill in sc.FILLS:
        _, views = roi_batch(fill)
        for r, x in zip(g.detect_batch(views), exp):
            same(r, x, fill)
    for name in sc.FRAMES:
        im = env.frames[name]
        one = g.detect(im)
        same(one, ref(env, F32, name), name)
        for layout in sc.LAYOUTS:
            for fill in sc.FILLS:
                same(g.detect(sc.embed(im, layout, fill)[0]), one, (name, layout, fill))
    g.close()


# ---- device frames ----------------------------------------------------------------------------------------------------------
def device_entries(h, im, layout, exp, lat, gt, truth, gts, planes, imdtype, what):
    w, hgt, cn = geom(im)
    for fill in sc.FILLS:
        view, parent = sc.embed(im, layout, fill)
        t = device(parent)
        p, s = dev_ptr(t, view, parent), view.strides[0]
        same(h.detect_dev(p, w, hgt, cn, stride=s), exp, (what, fill))
        same_arrays(plan_planes(h, im, imdtype), planes, (what, fill))
        h.enqueue_dev(p, w, hgt, cn, stride=s)
        same(h.collect(), exp, (what, fill))
        same(h.detect_latent_dev(p, w, hgt, cn, truth, 0.5, stride=s), lat, (what, fill))
        same_arrays(h.detect_gtbox_dev(p, w, hgt, cn, gts, 0.3, stride=s), gt, (what, fill))
        del t


def packed_device_refs(h, im):
    """records, latent record, gt-box winners and planes of the packed device tensor"""
    w, hgt, cn = geom(im)
    t = device(np.ascontiguousarray(im).reshape(-1))
    exp = h.detect_dev(t.data_ptr(), w, hgt, cn)
    assert len(exp[0]) >= sc.MIN_RECORDS, len(exp[0])
    truth, gts = truth_of(exp), gts_of(exp)
    lat = h.detect_latent_dev(t.data_ptr(), w, hgt, cn, truth, 0.5)
    gt = h.detect_gtbox_dev(t.data_ptr(), w, hgt, cn, gts, 0.3)
    assert len(lat[0]) == 1 and gt[3][:2].any()
    return exp, lat, gt, truth, gts


@pytest.mark.parametrize("name,layout", CASES, ids=CASE_IDS)
def test_device_frames(env, name, layout):
    """detect_dev, enqueue_dev, detect_latent_dev, detect_gtbox_dev read the caller's strided buffer in place (k_resize_linear_u8)"""
    im = env.frames[name]
    h = env.h[F32]
    exp, lat, gt, truth, gts = packed_device_refs(h, im)
    same(exp, ref(env, F32, name), "device vs host")
    h.detect(im)
    device_entries(h, im, layout, exp, lat, gt, truth, gts, plan_planes(h, im), None, (name, layout))


@pytest.mark.parametrize("layout", sc.OPTION_LAYOUTS)
@pytest.mark.parametrize("dtype,kind", [(F32, capi.PBD_PYRAMID_MATLAB), (F64, capi.PBD_PYRAMID_OPENCV), (F64, capi.PBD_PYRAMID_MATLAB)],
                         ids=["f32-matlab", "f64-opencv", "f64-matlab"])
def test_device_frames_scalar_types_and_pyramid_kinds(env, dtype, kind, layout):
    """the same on double handles and under the MATLAB pyramid (k_resize_area<uint8_t> reads the strided buffer); float handles under
    the default pyramid: test_device_frames"""
    h = capi.Handle(env.model, dtype=dtype)
    h.set_pyramid_kind(kind)
    imdtype = F64 if kind == capi.PBD_PYRAMID_MATLAB else None
    for name in sc.FRAMES:
        im = env.frames[name]
        exp, lat, gt, truth, gts = packed_device_refs(h, im)
        same(h.detect(im), exp, "device vs host")
        device_entries(h, im, layout, exp, lat, gt, truth, gts, plan_planes(h, im, imdtype), imdtype, (name, layout, kind))
        if kind == capi.PBD_PYRAMID_MATLAB:         # host frames under the MATLAB kind
            same(h.detect(sc.embed(im, layout, sc.FILLS[1])[0]), exp, (name, layout, "host"))
    h.close()


# ---- graph replay -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sc.OPTION_LAYOUTS)
@pytest.mark.parametrize("where", ["device", "host"])
def test_graph_eager_captured_replayed(env, where, layout):
    """graph=1: frame 1 reads the strided buffer eagerly, frames 2 and 3 go through the copy into the handle's own image in front of
    the capture and the replay.  Three DIFFERENT frames, each against its own packed result: a replay on a stale image fails."""
    frames = sc.graph_frames() + [env.frames["bgr101x77"]]
    plain = env.h[F32]
    exps, planes = [], []
    for f in frames:
        exps.append(plain.detect(f))
        planes.append(plan_planes(plain, f))
        assert len(exps[-1][0]) >= sc.MIN_RECORDS
    assert len({x[0].tobytes() for x in exps}) == len(frames)
    h = capi.Handle(env.model, graph=1)
    for rnd, fill in enumerate(sc.FILLS):
        for i, f in enumerate(frames):
            view, parent = sc.embed(f, layout, fill)
            if where == "device":
                t = device(parent)
                got = h.detect_dev(dev_ptr(t, view, parent), 101, 77, 3, stride=view.strides[0])
            else:
                got = h.detect(view)
            same(got, exps[i], (where, layout, rnd, i))
            same_arrays(plan_planes(h, f), planes[i], (where, layout, rnd, i))
    h.close()


# ---- depth images -----------------------------------------------------------------------------------------------------------
def depth_case(env, dtype):
    im = env.frames[DEPTH_FRAME]
    w, hgt, _ = geom(im)
    return im, w, hgt, sc.depth_images(w, hgt, dtype)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_host_depth_entries(env, dtype):
    """detect_rgbd and detect_batch_rgbd (one frame's depth None) with strided depth views and strided frames"""
    im, w, hgt, depths = depth_case(env, dtype)
    raw = ref(env, dtype, DEPTH_FRAME)
    h = capi.Handle(env.model, dtype=dtype)
    frames = [im] + sc.batch_frames()[2:]
    for dname, d in depths.items():
        h.set_depth_filter(True, ZF[dname])
        exp = h.detect_rgbd(im, d)
        assert sc.MIN_RECORDS <= len(exp[0]) < len(raw[0]), (dname, len(exp[0]), len(raw[0]))   # the filter is at work
        bexp = h.detect_batch_rgbd(frames, [d, None, d])
        same(bexp[0], exp, "batch vs single")
        for layout in sc.DEPTH_LAYOUTS:
            for fill in sc.FILLS:
                zv, _ = sc.embed_depth(d, layout, fill)
                what = (dname, layout, fill)
                same(h.detect_rgbd(im, zv), exp, what)
                same(h.detect_rgbd(sc.embed(im, "roi", fill)[0], zv), exp, what)
                zv2, _ = sc.embed_depth(d, layout, fill + 1)           # a second view of the same stride
                views = [sc.embed(f, "pad3", fill)[0] for f in frames]
                for g, x in zip(h.detect_batch_rgbd(views, [zv, None, zv2]), bexp):
                    same(g, x, what)
    h.close()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_depth_primitives(env, dtype):
    """candidates_depth_filter, and candidates_box3d in 32F and 64F, with strided depth"""
    im, w, hgt, _ = depth_case(env, dtype)
    h = env.h[dtype]
    recs = ref(env, dtype, DEPTH_FRAME)
    for dname, d in sc.depth_images(w, hgt, dtype).items():
        kept = h.candidates_depth_filter(*recs, d, ZF[dname])
        assert sc.MIN_RECORDS <= len(kept[0]) < len(recs[0])
        for layout in sc.DEPTH_LAYOUTS:
            for fill in sc.FILLS:
                same(h.candidates_depth_filter(*recs, sc.embed_depth(d, layout, fill)[0], ZF[dname]), kept, (dname, layout, fill))
    for zt in (F32, F64):
        for dname, d in sc.depth_images(w, hgt, zt).items():
            b3 = h.candidates_box3d(recs[0], recs[1], d, w, hgt, sc.CAM, depth_dtype=zt)
            assert b3[0]["valid"].any()
            for layout in sc.DEPTH_LAYOUTS:
                for fill in sc.FILLS:
                    got = h.candidates_box3d(recs[0], recs[1], sc.embed_depth(d, layout, fill)[0], w, hgt, sc.CAM, depth_dtype=zt)
                    same_arrays(got, b3, (zt, dname, layout, fill))


@pytest.mark.parametrize("stage", ["depth_filter", "box3d", "cluster3d"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_device_depth(env, dtype, stage):
    """enqueue_rgbd_dev with a padded dstride: zselect (k_zfilter.hip), b3_px (k_box3d.hip) and the in-frame cloud of k_cluster3d.hip
    read the caller's strided depth image in place"""
    im, w, hgt, depths = depth_case(env, dtype)
    raw = ref(env, dtype, DEPTH_FRAME)
    h = capi.Handle(env.model, dtype=dtype)
    if stage == "depth_filter":
        h.set_depth_filter(True, ZF["planes"])
    else:
        h.set_box3d(True, sc.CAM)
        if stage == "cluster3d":
            h.set_cluster3d(True, 0.01)

    def results():
        out = list(h.collect())
        if stage != "depth_filter":
            out += list(h.get_box3d(0))
        if stage == "cluster3d":
            out += list(h.get_cluster3d(0))
        return out

    d = depths["planes" if stage == "depth_filter" else "blobs"]
    t_im, t_z = device(im.reshape(-1)), device(d.view(np.uint8).reshape(-1))
    h.enqueue_rgbd_dev(t_im.data_ptr(), w, hgt, 3, t_z.data_ptr())
    exp = results()
    if stage == "depth_filter":
        assert sc.MIN_RECORDS <= len(exp[0]) < len(raw[0])
    else:
        same(exp[:3], raw, "records unchanged")
        assert len(exp[3]) == len(raw[0]) and exp[3]["valid"].any()
    if stage == "cluster3d":
        assert len(exp[5]) == len(raw[0]) and (exp[5]["size"] > 0).any()
    for layout in sc.DEPTH_LAYOUTS:
        for fill in sc.FILLS:
            zv, zparent = sc.embed_depth(d, layout, fill)
            view, parent = sc.embed(im, "roi" if layout == "roi" else "pad1", fill)
            tz, ti = device(zparent), device(parent)
            h.enqueue_rgbd_dev(dev_ptr(ti, view, parent), w, hgt, 3, dev_ptr(tz, zv, zparent), dstride=zv.strides[0], stride=view.strides[0])
            same_arrays(results(), exp, (stage, layout, fill))
            h.enqueue_rgbd_dev(t_im.data_ptr(), w, hgt, 3, dev_ptr(tz, zv, zparent), dstride=zv.strides[0])
            same_arrays(results(), exp, (stage, layout, fill, "packed frame"))
    h.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def rec_bufs(h, n=4096):
    heads = np.zeros(n, capi.HEAD_DTYPE)
    boxes, locs = np.zeros((n, h.max_parts, 4), np.int32), np.zeros((n, h.max_parts, 3), np.int32)
    return (heads, boxes, locs), (V(heads.ctypes.data), V(boxes.ctypes.data), V(locs.ctypes.data))


def no_pending(h):
    """the handle has no pending frame: a collect is refused as one without a detect"""
    keep, ptrs = rec_bufs(h, 16)
    cnt = C.c_int(0)
    return h.L.pbd_detect_collect(h.h, *ptrs, 16, C.byref(cnt)) == STATE


def frame_entries(env, h, im, dev):
    """(the example cache of the warp entry, {entry: call(stride) -> status}, the output buffers — the caller holds them while it
    calls): raw calls of every entry of a float handle that takes a `stride`, every other argument valid"""
    L = h.L
    w, hgt, cn = geom(im)
    P, dP = V(im.ctypes.data), V(dev.data_ptr())
    two = (V * 2)(im.ctypes.data, im.ctypes.data)
    keep, R = rec_bufs(h, 2 * 4096)
    cnt, counts = C.c_int(0), (C.c_int * 2)()
    exp = ref(env, F32, "bgr101x77")
    tr = np.zeros((2, h.max_parts, 4), np.int32)
    tr[:, :5] = truth_of(exp)
    gt = np.zeros((2, capi.PBD_GT_MAX, 4), np.float64)
    gt[:, :4] = gts_of(exp)
    ngt = np.array([4, 4], np.int32)
    found, o = np.zeros(2 * capi.PBD_GT_MAX, np.int32), np.zeros(2 * capi.PBD_GT_MAX, np.float64)
    keep_g, G = rec_bufs(h, 2 * capi.PBD_GT_MAX)
    hog_out = np.zeros((hgt // 4 + 2) * (w // 4 + 2) * 32, np.float32)
    small = np.zeros((hgt, w, 3), np.uint8)
    a, b = C.c_int(0), C.c_int(0)
    boxes = warp_boxes(w, hgt)
    kh, kw = h.filter_size(1)
    win = np.zeros((len(boxes), (kh + 2) * 4, (kw + 2) * 4, 3), np.float64)
    feat = np.zeros((len(boxes), kh, kw, 32), np.float32)
    q = capi.QpCache(h, len(boxes), 1.0, 1.0)
    status, written = np.zeros(len(boxes), np.int32), C.c_int(0)
    chosen, ms = C.c_int(0), (C.c_double * 2)()
    tp, gp = V(tr.ctypes.data), V(gt.ctypes.data)
    return q, (keep, keep_g, tr, gt), {
        "pbd_detect_u8": lambda s: L.pbd_detect_u8(h.h, P, w, hgt, cn, s, *R, 4096, C.byref(cnt)),
        "pbd_detect_enqueue_u8": lambda s: L.pbd_detect_enqueue_u8(h.h, P, w, hgt, cn, s),
        "pbd_detect_image": lambda s: L.pbd_detect_image(h.h, P, capi.PBD_DEPTH_8U, w, hgt, cn, s, *R, 4096, C.byref(cnt)),
        "pbd_detect_dev_u8": lambda s: L.pbd_detect_dev_u8(h.h, dP, w, hgt, cn, s, *R, 4096, C.byref(cnt)),
        "pbd_detect_enqueue_dev_u8": lambda s: L.pbd_detect_enqueue_dev_u8(h.h, dP, w, hgt, cn, s),
        "pbd_detect_batch_u8": lambda s: L.pbd_detect_batch_u8(h.h, two, 2, w, hgt, cn, s, *R, 4096, counts),
        "pbd_detect_batch_enqueue_u8": lambda s: L.pbd_detect_batch_enqueue_u8(h.h, two, 2, w, hgt, cn, s),
        "pbd_pyramid_u8": lambda s: L.pbd_pyramid_u8(h.h, P, w, hgt, cn, s),
        "pbd_pyramid_image": lambda s: L.pbd_pyramid_image(h.h, P, capi.PBD_DEPTH_8U, w, hgt, cn, s),
        "pbd_hog_u8": lambda s: L.pbd_hog_u8(h.h, P, w, hgt, cn, s, V(hog_out.ctypes.data), C.byref(a), C.byref(b)),
        "pbd_resize_u8": lambda s: L.pbd_resize_u8(h.h, P, w, hgt, cn, s, V(small.ctypes.data), w - 7, hgt - 5),
        "pbd_pyrdown_u8": lambda s: L.pbd_pyrdown_u8(h.h, P, w, hgt, cn, s, V(small.ctypes.data)),
        "pbd_detect_latent_u8": lambda s: L.pbd_detect_latent_u8(h.h, P, w, hgt, cn, s, tp, None, -1, D(0.5), *R, C.byref(cnt)),
        "pbd_detect_latent_dev_u8": lambda s: L.pbd_detect_latent_dev_u8(h.h, dP, w, hgt, cn, s, tp, None, -1, D(0.5), *R, C.byref(cnt)),
        "pbd_detect_batch_latent_u8": lambda s: L.pbd_detect_batch_latent_u8(h.h, two, 2, w, hgt, cn, s, tp, None, -1, D(0.5), *R, counts),
        "pbd_detect_gtbox_u8": lambda s: L.pbd_detect_gtbox_u8(h.h, P, w, hgt, cn, s, gp, 4, D(0.3), *G, V(found.ctypes.data),
                                                              V(o.ctypes.data), C.byref(cnt)),
        "pbd_detect_gtbox_dev_u8": lambda s: L.pbd_detect_gtbox_dev_u8(h.h, dP, w, hgt, cn, s, gp, 4, D(0.3), *G, V(found.ctypes.data),
                                                                      V(o.ctypes.data), C.byref(cnt)),
        "pbd_detect_batch_gtbox_u8": lambda s: L.pbd_detect_batch_gtbox_u8(h.h, two, 2, w, hgt, cn, s, gp, V(ngt.ctypes.data), D(0.3), *G,
                                                                          V(found.ctypes.data), V(o.ctypes.data), C.byref(cnt)),
        "pbd_warp_windows_u8": lambda s: L.pbd_warp_windows_u8(h.h, P, w, hgt, cn, s, V(boxes.ctypes.data), len(boxes), 1,
                                                              V(win.ctypes.data), V(feat.ctypes.data)),
        "pbd_qp_write_warped_u8": lambda s: L.pbd_qp_write_warped_u8(q.q, P, w, hgt, cn, s, V(boxes.ctypes.data), None, len(boxes), 1, 0,
                                                                    0.0, V(status.ctypes.data), C.byref(written)),
        "pbd_tune_plan": lambda s: L.pbd_tune_plan(h.h, P, w, hgt, cn, s, 1, C.byref(chosen), ms),
    }


ENQUEUES = {"pbd_detect_enqueue_u8", "pbd_detect_enqueue_dev_u8", "pbd_detect_batch_enqueue_u8"}


def test_refusals_frame_stride(env):
    """stride = w * cn - 1 and negative strides: PBD_ERR_ARG from every entry, no frame left pending, the next valid call is right"""
    name = "bgr101x77"
    im = env.frames[name]
    w, hgt, cn = geom(im)
    row = w * cn
    h = env.h[F32]
    exp = ref(env, F32, name)
    dev = device(im.reshape(-1))
    q, outputs, entries = frame_entries(env, h, im, dev)
    for entry, call in entries.items():
        for bad in (row - 1, -1, -row, 0):
            assert call(bad) == ARG, (entry, bad)
            assert no_pending(h), (entry, bad)
        assert call(row) == OK, entry                       # every other argument was valid: the stride alone was refused
        if entry == "pbd_detect_batch_enqueue_u8":
            h._nb = 2
            for r in h.collect_batch():
                same(r, exp, entry)
        elif entry in ENQUEUES:
            same(h.collect(), exp, entry)
        else:
            assert no_pending(h), entry
        same(h.detect(sc.embed(im, "pad1", 1)[0]), exp, entry)
    q.close()
    del outputs
    # the double handle's own entries
    hd = env.h[F64]
    out = np.zeros((hgt // 4 + 2) * (w // 4 + 2) * 32, np.float64)
    a, b = C.c_int(0), C.c_int(0)
    boxes = warp_boxes(w, hgt)
    win, feat = np.zeros((len(boxes), 28, 28, 3), np.float64), np.zeros((len(boxes), 5, 5, 32), np.float64)
    for bad in (row - 1, -1):
        assert hd.L.pbd_hog_u8_f64(hd.h, V(im.ctypes.data), w, hgt, cn, bad, V(out.ctypes.data), C.byref(a), C.byref(b)) == ARG
        assert hd.L.pbd_warp_windows_u8_f64(hd.h, V(im.ctypes.data), w, hgt, cn, bad, V(boxes.ctypes.data), len(boxes), 1,
                                            V(win.ctypes.data), V(feat.ctypes.data)) == ARG
    same_arrays([hd.hog(sc.embed(im, "pad1", 1)[0])], [hd.hog(im)])
    same(hd.detect(im), ref(env, F64, name), "double")


def test_refusals_group(env):
    im = env.frames["bgr101x77"]
    w, hgt, cn = geom(im)
    g = capi.Group(env.model, [0, 0], gather=capi.PBD_GATHER_HOST)
    keep, R = rec_bufs(g, 2 * 4096)
    cnt, counts = C.c_int(0), np.zeros(2, np.int32)
    two = (V * 2)(im.ctypes.data, im.ctypes.data)
    for bad in (w * cn - 1, -1):
        assert g.L.pbd_group_detect_u8(g.g, V(im.ctypes.data), w, hgt, cn, bad, *R, 4096, C.byref(cnt)) == ARG
        assert g.L.pbd_group_detect_batch_u8(g.g, two, 2, w, hgt, cn, bad, *R, 4096, V(counts.ctypes.data)) == ARG
        same(g.detect(sc.embed(im, "roi", 2)[0]), ref(env, F32, "bgr101x77"), bad)
        for r in g.detect_batch([im, sc.embed(im, "roi", 2)[0]]):
            same(r, ref(env, F32, "bgr101x77"), bad)
    g.close()


@pytest.mark.parametrize("kind", list(sc.WIDE))
def test_refusals_wide_stride(env, kind):
    """wide depths: a stride in bytes below the row, negative, or no multiple of the element size"""
    im = env.frames[kind]
    w, hgt, cn = geom(im)
    row, esz = w * cn * im.itemsize, im.itemsize
    h = env.h[F32]
    exp = h.detect_image(im)
    keep, R = rec_bufs(h)
    cnt = C.c_int(0)
    depth = capi.DEPTH_OF[im.dtype]
    for bad in (row - esz, row - 1, -row, row + 1, row + esz - 1, 512 * esz + 1):
        assert h.L.pbd_detect_image(h.h, V(im.ctypes.data), depth, w, hgt, cn, bad, *R, 4096, C.byref(cnt)) == ARG, (kind, bad)
        assert h.L.pbd_pyramid_image(h.h, V(im.ctypes.data), depth, w, hgt, cn, bad) == ARG, (kind, bad)
        assert no_pending(h)
    assert h.L.pbd_detect_image(h.h, V(im.ctypes.data), depth, w, hgt, cn, row, *R, 4096, C.byref(cnt)) == OK and cnt.value == len(exp[0])
    same(h.detect_image(sc.embed(im, "pad1", 1)[0]), exp, kind)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_refusals_depth_stride(env, dtype):
    """dstride < w * ts or dstride % ts != 0 on the depth-carrying entries and the depth primitives; a bad frame stride on them too"""
    im, w, hgt, depths = depth_case(env, dtype)
    d = depths["planes"]
    ts = d.itemsize
    zrow, row = w * ts, w * 3
    dt = capi.DEPTH_OF[d.dtype]
    h = capi.Handle(env.model, dtype=dtype)
    h.set_depth_filter(True, ZF["planes"])
    L = h.L
    exp = h.detect_rgbd(im, d)
    recs = ref(env, dtype, DEPTH_FRAME)
    kept = h.candidates_depth_filter(*recs, d, ZF["planes"])
    keep, R = rec_bufs(h, 2 * 4096)
    cnt, counts = C.c_int(0), (C.c_int * 2)()
    P, Z = V(im.ctypes.data), V(d.ctypes.data)
    two, ztwo = (V * 2)(im.ctypes.data, im.ctypes.data), (V * 2)(d.ctypes.data, None)
    t_im, t_z = device(im.reshape(-1)), device(d.view(np.uint8).reshape(-1))
    dP, dZ = V(t_im.data_ptr()), V(t_z.data_ptr())
    hd, bx, lc = (np.ascontiguousarray(a).copy() for a in recs)
    b3, cen = np.zeros(len(hd), capi.BOX3D_DTYPE), np.zeros((len(hd), h.max_parts, 3), np.float64)
    cam = capi.camera(sc.CAM)
    k = C.c_int(0)
    calls = {
        "pbd_detect_rgbd_u8": lambda s, ds: L.pbd_detect_rgbd_u8(h.h, P, w, hgt, 3, s, Z, dt, ds, *R, 4096, C.byref(cnt)),
        "pbd_detect_rgbd_enqueue_dev_u8": lambda s, ds: L.pbd_detect_rgbd_enqueue_dev_u8(h.h, dP, w, hgt, 3, s, dZ, dt, ds),
        "pbd_detect_batch_rgbd_u8": lambda s, ds: L.pbd_detect_batch_rgbd_u8(h.h, two, ztwo, 2, w, hgt, 3, s, dt, ds, *R, 4096, counts),
    }
    for entry, call in calls.items():
        for ds in (zrow - ts, zrow - 1, zrow + 1, zrow + ts - 1, -zrow, 0):
            assert call(row, ds) == ARG, (entry, ds)
            assert no_pending(h), (entry, ds)
        for s in (row - 1, -1):
            assert call(s, zrow) == ARG, (entry, s)
            assert no_pending(h), (entry, s)
        assert call(row, zrow) == OK, entry
        if "enqueue" in entry:
            same(h.collect(), exp, entry)
        same(h.detect_rgbd(im, sc.embed_depth(d, "pad1", 1)[0]), exp, entry)
    for ds in (zrow - ts, zrow - 1, zrow + 1, -zrow, 0):
        assert L.pbd_candidates_depth_filter(h.h, C.c_float(ZF["planes"]), Z, dt, w, hgt, ds, V(hd.ctypes.data), V(bx.ctypes.data),
                                             V(lc.ctypes.data), len(hd), C.byref(k)) == ARG, ds
        assert L.pbd_candidates_box3d(h.h, C.byref(cam), Z, dt, w, hgt, ds, w, hgt, V(hd.ctypes.data), V(bx.ctypes.data), len(hd),
                                      V(b3.ctypes.data), V(cen.ctypes.data)) == ARG, ds
    assert hd.tobytes() == np.ascontiguousarray(recs[0]).tobytes()                       # a refused filter call leaves the records alone
    same(h.candidates_depth_filter(*recs, sc.embed_depth(d, "pitch512", 1)[0], ZF["planes"]), kept, "after refusals")
    h.close()
