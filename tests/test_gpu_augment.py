"""Virtual positives on the device (k_augment.hip; include/pbd_c.h "virtual positives") against pbd_augment_host_u8, which
tests/test_augment_cpu.py holds to the definition: every byte of pbd_augment_u8 and pbd_augment_dev_u8; and the seam that keeps virtual
positives in device memory — pbd_qp_write_warped_dev_u8, latentPositives and train() on capi.DeviceFrame items — against the same calls
on host arrays, in bits."""
import numpy as np
import pytest
import torch

from partsbaseddetector_amd import PartsBasedDetector, capi
from partsbaseddetector_amd.augment import augment_positives
from partsbaseddetector_amd.model import init_model, make_image
from partsbaseddetector_amd.train import train
from tests import augment_ref as ref
from tests import test_gpu_train as tt
from tests import warp_cases as wc

pytestmark = pytest.mark.gpu

IN_PAD, OUT_PAD, SENTINEL = 5, 7, 0x5A


def _dev_padded(im):
    """the frame in device memory inside rows IN_PAD bytes longer -> DeviceFrame"""
    a = np.asarray(im)
    hgt, w = a.shape[:2]
    cn = 1 if a.ndim == 2 else a.shape[2]
    buf = np.full((hgt, w * cn + IN_PAD), 0xA5, np.uint8)
    buf[:, :w * cn] = a.reshape(hgt, w * cn)
    t = torch.from_numpy(buf).cuda()
    return capi.DeviceFrame(t.data_ptr(), w, hgt, cn, w * cn + IN_PAD, t)


def _canvases(w, hgt, specs):
    ops = capi.augment_ops(specs)
    return [capi.augment_canvas(w, hgt, ops[i]) for i in range(len(specs))]


def _check_routes(im, specs, what):
    """both device routes through padded strides with sentinels against the host definition, in bytes"""
    a = np.asarray(im)
    hgt, w = a.shape[:2]
    cn = 1 if a.ndim == 2 else a.shape[2]
    canv = _canvases(w, hgt, specs)
    want = capi.augment_host(np.ascontiguousarray(a), specs)
    bufs = [np.full((r, c * cn + OUT_PAD), SENTINEL, np.uint8) for r, c in canv]
    got = capi.augment(ref.padded(a), specs, outs=bufs)
    touts = [torch.full((r, c * cn + OUT_PAD), SENTINEL, dtype=torch.uint8, device="cuda") for r, c in canv]
    frames = capi.augment_dev(_dev_padded(a), specs, outs=touts)
    for sp, wnt, g, b, f, t, (r, c) in zip(specs, want, got, bufs, frames, touts, canv):
        assert g.shape == wnt.shape and np.array_equal(g, wnt), (what, sp, "pbd_augment_u8", np.argwhere(g != wnt)[:3])
        assert (b[:, c * cn:] == SENTINEL).all(), (what, sp, "pbd_augment_u8 wrote behind a canvas row")
        d = f.numpy()
        assert (f.hgt, f.w, f.cn, f.stride) == (r, c, cn, c * cn + OUT_PAD)
        assert d.shape == wnt.shape and np.array_equal(d, wnt), (what, sp, "pbd_augment_dev_u8", np.argwhere(d != wnt)[:3])
        assert (t.cpu().numpy()[:, c * cn:] == SENTINEL).all(), (what, sp, "pbd_augment_dev_u8 wrote behind a canvas row")
    return want


# ---- device against host -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w, hgt, cn", ref.FRAMES)
def test_device_equals_host_on_the_grid(gpu_required, w, hgt, cn):
    _check_routes(ref.frame(w, hgt, cn), ref.grid_specs(), (w, hgt, cn))


def test_ten_ops_in_one_call_equal_one_call_each(gpu_required):
    im = ref.frame(37, 29, 3)
    specs = [(f, d, m) for f in (False, True) for d, m in ((None, 0), (7.5, 1), (-7.5, 1), (15.0, 0), (-15.0, 1))]
    assert len(specs) == 10
    together = capi.augment(im, specs)
    t = torch.from_numpy(im).cuda()
    together_dev = capi.augment_dev(t, specs)
    for sp, g, gd in zip(specs, together, together_dev):
        assert np.array_equal(capi.augment(im, [sp])[0], g), sp
        assert np.array_equal(capi.augment_dev(t, [sp])[0].numpy(), g), sp
        assert np.array_equal(gd.numpy(), g), sp


def test_partial_tiles(gpu_required):
    """130 x 70 at 15 degrees: the canvas is no multiple of the 64 x 4 tile, nor are the plain and the mirrored copy in the same launch"""
    for cn in (3, 1):
        im = ref.frame(130, 70, cn)
        specs = [(False, 15.0, 1), (True, 15.0, 0), (True, None, 0), (False, -15.0, 1)]
        canv = _canvases(130, 70, specs)
        assert any(c % 64 for _, c in canv) and any(r % 4 for r, _ in canv)
        _check_routes(im, specs, ("partial", cn))


# ---- warped positives from device memory -------------------------------------------------------------------------------------------------
def _cache(h, capacity=8):
    return capi.QpCache(h, capacity, 0.002, 0.004)


def test_write_warped_dev_equals_write_warped_in_bits(gpu_required):
    model = wc.model_for(0)
    h = capi.Handle(model)
    _, boxes = wc.boxes_of(0)
    for cn in (3, 1):
        im = wc.frame(cn)
        assert im.shape[:2] == (80, 96)
        ids = np.arange(50, 50 + len(boxes), dtype=np.int32)
        for frame in (capi.DeviceFrame.from_tensor(torch.from_numpy(im).cuda()), _dev_padded(im)):
            qa, qb = _cache(h, len(boxes) - 3), _cache(h, len(boxes) - 3)      # the last boxes find the cache full
            wa, sa = qa.write_warped(im, boxes, 0, 0, 600.0, ids)             # 40 x 40 boxes pass, the 27 x 21 corner box is skipped
            wb, sb = qb.write_warped_dev(frame, boxes=boxes, filter=0, bias=0, min_area=600.0, ids=ids)
            assert wa == wb > 0 and sa.tobytes() == sb.tobytes()
            assert {capi.PBD_WARP_SKIPPED, capi.PBD_WARP_WRITTEN} <= set(sa.tolist())
            assert qa.dims() == qb.dims()
            for g, e, name in zip(qb.get(0, qb.dims()[2]), qa.get(0, qa.dims()[2]), ("x", "ids", "b", "d")):
                assert np.asarray(g).tobytes() == np.asarray(e).tobytes(), (cn, name)
            qa.close(); qb.close()
    # the detector's writeWarped takes the frame where it takes the array
    det = PartsBasedDetector(device=0)
    det.distributeModel(model)
    im = wc.frame(3)
    qa, qb = _cache(det.handle), _cache(det.handle)
    ra = det.writeWarped(im, boxes[:3], qa, ids=[1, 2, 3])
    rb = det.writeWarped(capi.DeviceFrame.from_tensor(torch.from_numpy(im).cuda()), boxes[:3], qb, ids=[1, 2, 3])
    assert ra[0] == rb[0] and ra[1].tobytes() == rb[1].tobytes()
    assert all(np.asarray(g).tobytes() == np.asarray(e).tobytes() for g, e in zip(qb.get(), qa.get()))
    det.handle.close()
    h.close()


def test_write_warped_dev_refusals_match(gpu_required):
    model = wc.model_for(0)
    h = capi.Handle(model)
    im = wc.frame(3)
    t = torch.from_numpy(im).cuda()
    frame = capi.DeviceFrame.from_tensor(t)
    _, boxes = wc.boxes_of(0)
    qa, qb = _cache(h), _cache(h)
    assert qa.write_warped(im, boxes[:2], 0, 0)[0] == qb.write_warped_dev(frame, boxes=boxes[:2])[0] == 2
    before = [np.asarray(v).tobytes() for v in qb.get(0, 8)]

    def both(boxes=boxes[:3], filter=0, bias=0, min_area=0.0, cn=3):
        errs = []
        for q, call in ((qa, lambda: qa.write_warped(im if cn == 3 else np.zeros((8, 8, 2), np.uint8), boxes, filter, bias, min_area)),
                        (qb, lambda: qb.write_warped_dev(t.data_ptr(), 96, 80, cn, boxes, filter, bias, min_area))):
            with pytest.raises(capi.PbdError) as e:
                call()
            errs.append((e.value.code, str(e.value)))
        assert errs[0] == errs[1], errs
        assert [np.asarray(v).tobytes() for v in qb.get(0, 8)] == before and qb.dims() == qa.dims()
        return errs[0][0]

    bad = boxes[:3].copy(); bad[1, 2] = np.nan
    assert both(boxes=bad) == capi.PBD_ERR_ARG
    bad = boxes[:3].copy(); bad[0] = (1, 1, 12000, 40)
    assert both(boxes=bad) == capi.PBD_ERR_UNSUPPORTED
    assert both(filter=len(model.filtersw)) == capi.PBD_ERR_ARG
    assert both(bias=-1) == capi.PBD_ERR_ARG
    assert both(min_area=np.nan) == capi.PBD_ERR_ARG
    assert both(cn=2) == capi.PBD_ERR_ARG
    h.enqueue(im)
    assert both() == capi.PBD_ERR_STATE
    h.collect(4096)
    with pytest.raises(capi.PbdError) as e:      # a NULL device pointer, like a NULL image
        qb.write_warped_dev(0, 96, 80, 3, boxes[:1])
    assert e.value.code == capi.PBD_ERR_ARG
    assert qb.write_warped_dev(frame, boxes=boxes[2:3])[0] == 1
    qa.close(); qb.close()
    h.close()


# ---- latent positives from device memory -------------------------------------------------------------------------------------------------
def test_latent_positives_from_a_device_frame_equal_the_arrays(gpu_required):
    model = tt.make_model("tree_k")
    items = tt.latent_items(model)
    dev_items = [(capi.DeviceFrame.from_tensor(torch.from_numpy(np.ascontiguousarray(it[0])).cuda()),) + tuple(it[1:]) for it in items]
    (da, qa), (db, qb) = tt.twins(model, np.float32)
    ca, ba = da.latentPositives(items, qa)
    cb, bb = db.latentPositives(dev_items, qb)
    assert ca.tolist() == cb.tolist() and ca.sum() > 0
    assert len(ba) == len(bb) and all((x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()) for x, y in zip(ba, bb))
    assert any(b is not None and b["written"] for b in bb)
    tt.same_caches(qa, qb, "latentPositives: DeviceFrame items against arrays")
    for d in (da, db):
        d.handle.close()


# ---- training on device-resident virtual positives -----------------------------------------------------------------------------------------
def _box(points):
    """a root box around two keypoints: their bounding box grown by 14 pixels (every box is at least 28 a side: none is skipped)"""
    p = np.asarray(points, np.float64)
    return (float(p[:, 0].min() - 14), float(p[:, 1].min() - 14), float(p[:, 0].max() + 14), float(p[:, 1].max() + 14))


def test_training_on_device_resident_virtual_positives(gpu_required):
    annotated = [(make_image(3, tt.SW, tt.SH), np.array([[30.0, 28.0], [52.0, 44.0]])), (make_image(4, tt.SW, tt.SH), np.array([[60.0, 30.0], [48.0, 55.0]]))]
    virt = augment_positives(annotated, mirror=[1, 0], degrees=(15.0,), keep_on_device=True)
    assert len(virt) == 8 and all(isinstance(v[0], capi.DeviceFrame) for v in virt[2:]) and virt[0][0] is annotated[0][0]
    host = [(v[0].numpy() if isinstance(v[0], capi.DeviceFrame) else v[0], v[1]) for v in virt]
    want = augment_positives(annotated, mirror=[1, 0], degrees=(15.0,), _route=capi.augment_host)
    assert all(np.array_equal(h[0], w[0]) and h[1].tobytes() == w[1].tobytes() for h, w in zip(host, want))
    negatives = [make_image(s, tt.SW, tt.SH) for s in (11, 12)]
    results = []
    for pos in (virt, host):
        model, report = train(init_model(None, None, 4, tsize=(5, 5)), [(im, _box(pts)) for im, pts in pos], negatives, 1, iter=1, max_iter=200,
                              seed=1, max_candidates=tt.MAXC)
        assert report[0]["numpositives"] == [8]
        results.append((model.weight_vector().tobytes(), np.float32(model.thresh).tobytes(), report[0]["mined"], report[0]["lb"], report[0]["ub"]))
    assert results[0] == results[1]
    assert np.isfinite(np.frombuffer(results[0][1], np.float32)[0])


# ---- the C++ layer -------------------------------------------------------------------------------------------------------------------------
def test_cpp_layer_device_route(gpu_required, tmp_path):
    """pbd::augment on the device (tests/tools/augment_check.cpp) gives the host definition's bytes"""
    import os
    im, lines = ref.cpp_check(tmp_path, os.path.dirname(capi.LIB_PATH), "device")
    ref.cpp_expect(im, lines, capi.augment_host, capi.map_rotate_points, capi.flip_points)
