"""Latent positives on the device (k_qp_latent.hip, k_qp.hip's write, pbd_qp_latent.cpp; include/pbd_c.h "latent positives"):
pbd_qp_write_latent_* against the route it replaces — pbd_detect_latent_u8 on a twin handle, the record home, and back through
pbd_qp_write(head, locs, 1, 1, id) into a twin cache — in bits; frames without a pose; a full cache; batches whose middle frame has no
pose; the croppos view against a contiguous copy; a refused record; what lingers on the handle; every refusal with the cache untouched;
latentPositives as its loop of primitives; the score identity; the C++ demo.

Truth boxes are the boxes of a pose the model returns on the frame (a plain detect's record): its own cells overlap them exactly."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import PartsBasedDetector, capi
from partsbaseddetector_amd.model import dense_feature_vectors, make_image, make_tree_model, make_tree_model_k, make_voc_like_model
from tests.feature_vector_ref import window_bounds
from tests.part_scores_ref import bound as ps_bound

pytestmark = pytest.mark.gpu

SW, SH = 100, 80
CAP = 16
MAXC = 4096
CPOS, CNEG = 0.002, 0.004
FAR = [50000, 50000, 20, 20]   # a truth box nowhere near the frame: no cell is admissible


def make_model(kind):
    if kind == "multi":
        return make_voc_like_model(seed=11)                                  # three components, mixed filter sizes
    return make_tree_model_k([-1, 0, 1, 1], [1, 3, 2, 2], seed=21)          # four parts, 1-3 mixtures


def handle(model, dtype=np.float32, pad=0, pyr=None, **kw):
    h = capi.Handle(model, dtype=dtype, max_candidates=MAXC, **kw)
    if pad:
        h.set_boundary_pad(pad)
    if pyr is not None:
        h.set_pyramid_kind(pyr)
    return h


_poses = {}


def poses(kind, seed, dtype=np.float32, pad=0, pyr=None, w=SW, hgt=SH):
    """(frame, heads, boxes, locs) of a plain detect at the 90th percentile of the frame's root scores: poses the model returns there.
    Computed once per configuration and left unchanged."""
    key = (kind, seed, np.dtype(dtype).name, pad, pyr, w, hgt)
    if key not in _poses:
        model = make_model(kind)
        im = make_image(seed, w, hgt)
        h = handle(model, dtype, pad, pyr)
        h.pyramid(im); h.pdf(); h.dp_min()
        v = np.concatenate([h.root(l, c)[0].ravel() for l in range(h._geo["nlevels"]) for c in range(model.ncomponents)])
        h.set_threshold(float(np.float32(np.percentile(v[np.isfinite(v)], 90.0))))
        got = h.detect(im, capacity=MAXC)
        h.close()
        assert len(got[0]) > 8
        _poses[key] = (im,) + tuple(got)
    return _poses[key]


def truth_of(model, heads, boxes, i):
    """record i's boxes as a truth set [max_parts, 4]"""
    t = np.zeros((model.max_parts, 4), np.int32)
    n = int(heads["nparts"][i])
    t[:n] = boxes[i][:n]
    return t


def best(heads, where=None):
    idx = np.arange(len(heads)) if where is None else np.flatnonzero(where)
    assert len(idx), "no pose of the wanted kind on this frame"
    return int(idx[np.argmax(heads["score"][idx])])


def snapshot(q):
    """everything of a cache a call could change, as bytes: every column of the capacity, dims, the solver's a, sv, w and stats"""
    cap = q.dims()[2]
    a, sv, w, st = q.state()
    return [v.tobytes() for v in q.get(0, cap)] + [repr(q.dims()), a.tobytes(), sv.tobytes(), w.tobytes(), st.tobytes()]


def same_caches(q, t, what=""):
    for i, (g, e) in enumerate(zip(snapshot(q), snapshot(t))):
        assert g == e, (what, ("x", "ids", "b", "d", "dims", "a", "sv", "w", "stats")[i])


def host_route(g, t, im, truth, overlap, id, mix=None, component=-1):
    """what the call replaces: detect_latent, the record home, and back into pbd_qp_write with label +1 -> (heads, locs, written)"""
    heads, _, locs = g.detect_latent(im, truth, overlap, mix, component)
    return heads, locs, (t.write(heads, locs, 1, id) if len(heads) else 0)


def check_block(blk, heads, locs, written):
    assert int(blk["found"]) == len(heads) and int(blk["written"]) == written
    if len(heads):
        assert (int(blk["component"]), int(blk["level"])) == (int(heads[0]["component"]), int(heads[0]["level"]))
        assert (int(blk["x"]), int(blk["y"])) == (int(locs[0, 0, 0]), int(locs[0, 0, 1]))
        assert np.float64(blk["score"]).tobytes() == np.float64(heads[0]["score"]).tobytes()
    else:
        assert not any(int(blk[k]) for k in ("component", "level", "x", "y")) and blk["score"] == 0


# ---- 1. equals the host route, in bits -------------------------------------------------------------------------------------------------
# name -> (model, dtype, pad, pyramid kind, what is given: "mix" / "component" / None, border: the truth reaches over the frame's edge)
EQUAL = {
    "tree_f32": ("tree_k", np.float32, 0, None, None, False),
    "tree_f64": ("tree_k", np.float64, 0, None, None, False),
    "multi_f32": ("multi", np.float32, 0, None, None, False),
    "multi_f64_component": ("multi", np.float64, 0, None, "component", False),
    "tree_f32_mix": ("tree_k", np.float32, 0, None, "mix", False),
    "tree_f32_pad_border": ("tree_k", np.float32, 3, None, None, True),
    "tree_f64_matlab_pyramid": ("tree_k", np.float64, 0, capi.PBD_PYRAMID_MATLAB, None, False),
    # the handle's candidate filter on the single record: the scan reads the filter's count block instead of the back-tracking's list
    "tree_f32_sort_nms": ("tree_k", np.float32, 0, None, None, False),
    "multi_f64_sort": ("multi", np.float64, 0, None, None, False),
}
SORT_NMS = (capi.PBD_CAND_SORT_NMS, 0.5)
FILTER = {"tree_f32_sort_nms": SORT_NMS, "multi_f64_sort": (capi.PBD_CAND_SORT, 0.0)}


@pytest.mark.parametrize("name", sorted(EQUAL))
def test_equals_the_host_route(gpu_required, name):
    kind, dtype, pad, pyr, given, border = EQUAL[name]
    model = make_model(kind)
    im, heads, boxes, locs = poses(kind, 3, dtype, pad, pyr)
    i = best(heads, heads["component"] == 1 if given == "component" else None)
    truth = truth_of(model, heads, boxes, i)
    overlap = 0.7
    if border:   # the pose's boxes moved to hang over the frame's left edge: the poses that overlap them stand at the border, where
        np_ = int(heads["nparts"][i])                             # the planes carry the boundary pad
        truth[:np_, 0] -= truth[:np_, 0].min() + 6
        overlap = 0.5
    mix = None
    if given == "mix":       # the pose's own mixtures for parts 1 and 3, the others free
        mix = np.full(model.max_parts, -1, np.int32)
        mix[[1, 3]] = locs[i][[1, 3], 2]
    component = 1 if given == "component" else -1
    h, g = (handle(model, dtype, pad, pyr, cand_filter=FILTER.get(name)) for _ in range(2))
    q, t = capi.QpCache(h, CAP, CPOS, CNEG), capi.QpCache(g, CAP, CPOS, CNEG)
    hd, lc, wr = host_route(g, t, im, truth, overlap, 5, mix, component)
    assert len(hd) == 1 and wr == 1
    if border:                                                    # the pose found stands at the frame's left border
        assert g.detect_latent(im, truth, overlap)[1][0][:int(hd[0]["nparts"]), 0].min() <= 0 and g.boundary_pad == pad
    ub0 = q.state()[3][3]
    blk = q.write_latent(im, truth, overlap, 5, mix, component)
    check_block(blk, hd, lc, 1)
    same_caches(q, t, name)
    assert q.dims()[3] == 1 and q.state()[3][3] == ub0 == 0          # ub does not move
    ids = q.get()[1]
    assert ids[0].tolist() == [1, 5, int(hd[0]["level"]), int(lc[0, 0, 0]), int(lc[0, 0, 1])]
    a, sv = q.state()[:2]
    assert a[0] == 0 and sv[0] == 1
    # the frame's feature planes are resident: the feature vector of the returned head is the host route's
    fa, fb = h.candidates_features(hd, lc), g.candidates_features(hd, lc)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fa, fb))
    h.close(); g.close()


def test_write_latent_dev_from_a_torch_tensor(gpu_required):
    import torch
    model = make_model("tree_k")
    im, heads, boxes, locs = poses("tree_k", 3)
    truth = truth_of(model, heads, boxes, best(heads))
    h, g = handle(model), handle(model)
    q, t = capi.QpCache(h, CAP, CPOS, CNEG), capi.QpCache(g, CAP, CPOS, CNEG)
    d_im = torch.from_numpy(im).cuda()
    torch.cuda.synchronize()
    got = q.write_latent_dev(d_im.data_ptr(), SW, SH, 3, truth, 0.7, 11)
    want = t.write_latent(im, truth, 0.7, 11)
    assert got.tobytes() == want.tobytes() and got["written"] == 1
    same_caches(q, t, "device frame")
    h.close(); g.close()


# ---- 2. no pose ------------------------------------------------------------------------------------------------------------------------
def test_no_pose(gpu_required):
    model = make_model("tree_k")
    im, heads, boxes, locs = poses("tree_k", 3)
    h = handle(model)
    q = capi.QpCache(h, CAP, CPOS, CNEG)
    q.write_latent(im, truth_of(model, heads, boxes, best(heads)), 0.7, 1)
    before = snapshot(q)
    blk = q.write_latent(im, np.tile(np.array(FAR, np.int32), (model.max_parts, 1)), 0.5, 2)
    check_block(blk, heads[:0], locs[:0], 0)
    assert snapshot(q) == before and q.dims()[3] == 1
    h.close()


# ---- 3. a full cache; behind examples already held -----------------------------------------------------------------------------------
def test_full_cache_and_behind_other_examples(gpu_required):
    model = make_model("tree_k")
    im, heads, boxes, locs = poses("tree_k", 3)
    order = np.argsort(-heads["score"])
    ta, tb = truth_of(model, heads, boxes, int(order[0])), truth_of(model, heads, boxes, int(order[len(order) // 2]))
    h, g = handle(model), handle(model)
    one = capi.QpCache(h, 1, CPOS, CNEG)
    first = one.write_latent(im, ta, 0.7, 1)
    assert (first["found"], first["written"]) == (1, 1)
    before = snapshot(one)
    second = one.write_latent(im, tb, 0.7, 2)
    assert (second["found"], second["written"]) == (1, 0) and one.dims()[3] == 1 and snapshot(one) == before
    # at n > 0: two negatives first, then two latent positives behind them; the earlier columns are untouched
    q, t = capi.QpCache(h, CAP, CPOS, CNEG), capi.QpCache(g, CAP, CPOS, CNEG)
    assert len(g.detect_latent(im, ta, 0.7)[0]) == 1               # (the twin's planes of this frame resident, as the first handle's are)
    for c in (q, t):
        assert c.write(heads[order[:2]], locs[order[:2]], -1, 9) == 2
    held = [v.copy() for v in q.get(0, 2)]
    for k, tr in enumerate((ta, tb)):
        hd, lc, wr = host_route(g, t, im, tr, 0.7, 20 + k)
        check_block(q.write_latent(im, tr, 0.7, 20 + k), hd, lc, wr)
    assert q.dims()[3] == 4
    same_caches(q, t, "behind two negatives")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(held, q.get(0, 2)))
    assert q.get()[1][:, 0].tolist() == [-1, -1, 1, 1]
    h.close(); g.close()


# ---- 4. batches: the middle frame has no pose -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [None, SORT_NMS], ids=["raw", "sort_nms"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_batch_equals_the_frames_one_by_one(gpu_required, dtype, filt):
    model = make_model("tree_k")
    sets = [poses("tree_k", s, dtype) for s in (3, 4, 5)]
    ims = [s[0] for s in sets]
    far = np.tile(np.array(FAR, np.int32), (model.max_parts, 1))
    truths = [truth_of(model, sets[0][1], sets[0][2], best(sets[0][1])), far, truth_of(model, sets[2][1], sets[2][2], best(sets[2][1]))]
    ids = [31, 32, 33]
    h, g = handle(model, dtype, cand_filter=filt), handle(model, dtype, cand_filter=filt)
    q, t = capi.QpCache(h, CAP, CPOS, CNEG), capi.QpCache(g, CAP, CPOS, CNEG)
    one = [t.write_latent(im, tr, 0.7, i) for im, tr, i in zip(ims, truths, ids)]
    if filt:   # the single calls are themselves the host route's, on a filtered handle too
        r = capi.QpCache(g, CAP, CPOS, CNEG)
        for im, tr, i in zip(ims, truths, ids):
            host_route(g, r, im, tr, 0.7, i)
        same_caches(t, r, "single calls on a filtered handle")
    got = q.write_latent_batch(ims, truths, 0.7, ids)
    assert got.tobytes() == np.array(one, capi.LATENT_EXAMPLE_DTYPE).tobytes()
    assert got["found"].tolist() == [1, 0, 1] and got["written"].tolist() == [1, 0, 1]
    same_caches(q, t, "batch")
    rows = q.get()[1]
    assert rows[:, 1].tolist() == [31, 33]                          # the ids of the frames that have a pose, in frame order
    for r, f in zip(rows, (0, 2)):                                    # ... with the frame's own level and root cell
        assert r.tolist() == [1, ids[f], int(got[f]["level"]), int(got[f]["x"]), int(got[f]["y"])]
    # the found frames in other places of the batch, and room for one example only: the first found frame takes it
    q2 = capi.QpCache(h, 1, CPOS, CNEG)
    got2 = q2.write_latent_batch([ims[1], ims[0], ims[2]], [far, truths[0], truths[2]], 0.7, [41, 42, 43])
    assert got2["found"].tolist() == [0, 1, 1] and got2["written"].tolist() == [0, 1, 0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(q2.get(0, 1)[0:1] + q2.get(0, 1)[2:], q.get(0, 1)[0:1] + q.get(0, 1)[2:]))
    assert q2.get()[1][0].tolist() == [1, 42] + rows[0, 2:].tolist()
    h.close(); g.close()


# ---- 5. the crop as a view -----------------------------------------------------------------------------------------------------------
def test_crop_as_a_view(gpu_required):
    model = make_model("tree_k")
    im, heads, boxes, locs = poses("tree_k", 6, w=200, hgt=150)
    # a pose away from the frame's corner, so that the view starts inside a row
    inner = np.array([boxes[i][:heads["nparts"][i], 0].min() > 60 and boxes[i][:heads["nparts"][i], 1].min() > 40 for i in range(len(heads))])
    i = best(heads, inner)
    np_ = int(heads["nparts"][i])
    roi, rel = capi.croppos(boxes[i][:np_], np_, 200, 150)
    x, y, w, hh = roi
    assert x > 0 and y > 0 and (w < 200 or hh < 150)
    view = im[y:y + hh, x:x + w]
    assert not view.flags["C_CONTIGUOUS"]
    h, g = handle(model), handle(model)
    q, t = capi.QpCache(h, CAP, CPOS, CNEG), capi.QpCache(g, CAP, CPOS, CNEG)
    a = q.write_latent(view, rel, 0.6, 3)
    b = t.write_latent(np.ascontiguousarray(view), rel, 0.6, 3)
    assert a.tobytes() == b.tobytes() and a["found"] == 1 and a["written"] == 1
    same_caches(q, t, "view against copy")
    h.close(); g.close()


# ---- 6. a record pbd_qp_write refuses -------------------------------------------------------------------------------------------------
def test_refused_record(gpu_required):
    """parts 1 and 2 share their def id (filter ids distinct: latent detection accepts the model): every pose repeats a dense start"""
    model = make_tree_model([-1, 0, 0], 1, seed=3)
    model.defid[0][2] = list(model.defid[0][1])
    im = make_image(3, SW, SH)
    h = handle(model)
    h.pyramid(im); h.pdf(); h.dp_min()
    v = np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])])
    h.set_threshold(float(np.float32(np.percentile(v[np.isfinite(v)], 95.0))))
    heads, boxes, locs = h.detect(im, capacity=MAXC)
    plain = [a.copy() for a in (heads, boxes, locs)]
    truth = truth_of(model, heads, boxes, best(heads))
    q = capi.QpCache(h, CAP, CPOS, CNEG)
    hd, _, lc = h.detect_latent(im, truth, 0.7)
    assert len(hd) == 1
    with pytest.raises(capi.PbdError) as e:                  # the host route refuses the same record
        q.write(hd, lc, 1, 9)
    assert e.value.code == capi.PBD_ERR_ARG
    before = snapshot(q)
    with pytest.raises(capi.PbdError) as e:
        q.write_latent(im, truth, 0.7, 9)
    assert e.value.code == capi.PBD_ERR_ARG and "frame 0" in str(e.value) and "qp_write.m:34-35" in str(e.value)
    assert snapshot(q) == before and q.dims()[3] == 0
    blk = q.last_latent[0]                                   # found and the head fields are filled, written = 0
    check_block(blk, hd, lc, 0)
    again = h.detect(im, capacity=MAXC)                      # the handle continues to work for a plain detect
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, plain))
    h.close()


# ---- 7. nothing lingers ---------------------------------------------------------------------------------------------------------------
def test_nothing_lingers(gpu_required):
    model = make_model("tree_k")
    im, heads, boxes, locs = poses("tree_k", 3)
    truth = truth_of(model, heads, boxes, best(heads))
    h, g = handle(model), handle(model)
    thr = float(np.sort(heads["score"])[-8])
    for x in (h, g):
        x.set_threshold(thr)
    q, t = capi.QpCache(h, 64, CPOS, CNEG), capi.QpCache(g, 64, CPOS, CNEG)
    q.state()
    ub0 = q.state()[3][3]
    assert q.write_latent(im, truth, 0.7, 1)["written"] == 1
    assert q.state()[3][3] == ub0
    host_route(g, t, im, truth, 0.7, 1)
    fresh = handle(model)
    fresh.set_threshold(thr)
    want = fresh.detect(im, capacity=MAXC)
    got = h.detect(im, capacity=MAXC)                        # the mask is gone with the next frame's responses
    assert len(want[0]) >= 4 and all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    rec, wr, _ = q.mine(im, 2)                               # ... and mining on the same cache equals its host route
    assert rec == len(want[0]) and wr == t.write(want[0], want[2], -1, 2)
    t.state()
    for name, a, b in zip(("x", "ids", "b", "d"), q.get(0, 64), t.get(0, 64)):
        assert a.tobytes() == b.tobytes(), name
    assert q.write_latent(im, truth, 0.7, 3)["written"] == 1    # and a latent positive behind the mined negatives
    hd, lc, wr = host_route(g, t, im, truth, 0.7, 3)
    assert wr == 1
    for name, a, b in zip(("x", "ids", "b", "d"), q.get(0, 64), t.get(0, 64)):
        assert a.tobytes() == b.tobytes(), name
    for x in (h, g, fresh):
        x.close()


# ---- 8. refusals leave nothing behind ---------------------------------------------------------------------------------------------------
def refused(q, call, code, what):
    before = snapshot(q)
    with pytest.raises(capi.PbdError) as e:
        call()
    assert e.value.code == code, (what, str(e.value))
    assert snapshot(q) == before, what
    return e.value


def test_refusals(gpu_required):
    model = make_model("tree_k")
    im, heads, boxes, locs = poses("tree_k", 3)
    truth = truth_of(model, heads, boxes, best(heads))
    h = handle(model)
    h.set_threshold(1e30)
    q = capi.QpCache(h, CAP, CPOS, CNEG)
    assert q.write_latent(im, truth, 0.7, 1)["written"] == 1      # (a cache that holds an example)

    def go():
        return q.write_latent(im, truth, 0.7, 9)

    h.set_part_scores(True)
    refused(q, go, capi.PBD_ERR_UNSUPPORTED, "per-part scores on")
    h.set_part_scores(False)
    h.set_depth_filter(True)
    refused(q, go, capi.PBD_ERR_UNSUPPORTED, "depth pruning on")
    h.set_depth_filter(False)
    h.enqueue(im)
    refused(q, go, capi.PBD_ERR_STATE, "a frame pending")
    h.collect(capacity=MAXC)
    bad = truth.copy(); bad[1, 2] = -1
    refused(q, lambda: q.write_latent(im, bad, 0.7, 9), capi.PBD_ERR_ARG, "negative width")
    refused(q, lambda: q.write_latent(im, truth, 1.0, 9), capi.PBD_ERR_ARG, "overlap 1")
    # nframes = 0 and 65, through the C entry
    ptrs = (C.c_void_p * 65)(*([im.ctypes.data] * 65))
    tr = np.ascontiguousarray(np.tile(truth, (65, 1, 1)))
    ids = np.arange(65, dtype=np.int32)
    out = np.zeros(65, capi.LATENT_EXAMPLE_DTYPE)
    for n in (0, 65):
        before = snapshot(q)
        rc = h.L.pbd_qp_write_latent_batch_u8(q.q, ptrs, n, SW, SH, 3, SW * 3, tr.ctypes.data, None, -1, C.c_double(0.7), ids.ctypes.data,
                                              out.ctypes.data)
        assert rc == capi.PBD_ERR_ARG and snapshot(q) == before, n
    assert h.L.pbd_qp_write_latent_u8(q.q, im.ctypes.data, SW, SH, 3, SW * 3, None, None, -1, C.c_double(0.7), 1, out.ctypes.data) == capi.PBD_ERR_ARG
    assert h.L.pbd_qp_write_latent_u8(q.q, im.ctypes.data, SW, SH, 3, SW * 3, tr.ctypes.data, None, -1, C.c_double(0.7), 1, None) == capi.PBD_ERR_ARG
    assert q.write_latent(im, truth, 0.7, 2)["written"] == 1 and q.dims()[3] == 2      # the handle and the cache are fine afterwards
    h.close()
    # the compact memory plan, on every frame
    c = handle(model, dp_mode=2)
    qc = capi.QpCache(c, CAP, CPOS, CNEG)
    err = refused(qc, lambda: qc.write_latent(im, truth, 0.7, 9), capi.PBD_ERR_UNSUPPORTED, "compact plan")
    assert "compact" in str(err)
    assert len(c.detect_latent(im, truth, 0.7)[0]) == 1            # nothing pending: latent detection itself works on this plan
    c.close()
    # the score-map NMS
    n = handle(model, nms_sz=1)
    qn = capi.QpCache(n, CAP, CPOS, CNEG)
    refused(qn, lambda: qn.write_latent(im, truth, 0.7, 9), capi.PBD_ERR_UNSUPPORTED, "score-map NMS")
    n.close()
    # a filter id shared between two slots of the components searched
    shared = make_model("tree_k")
    shared.filterid[0][3][1] = shared.filterid[0][2][0]
    s = handle(shared)
    qs = capi.QpCache(s, CAP, CPOS, CNEG)
    err = refused(qs, lambda: qs.write_latent(im, truth, 0.7, 9), capi.PBD_ERR_UNSUPPORTED, "shared filter id")
    assert "shared" in str(err)
    s.close()
    # a pbd_group member takes no example cache at all: the entry cannot be reached with one
    grp = capi.Group(model, [0], gather=capi.PBD_GATHER_HOST)
    member = C.c_void_p(grp.L.pbd_group_member(grp.g, 0))
    qg = C.c_void_p()
    assert grp.L.pbd_qp_create(member, CAP, CPOS, CNEG, None, None, C.byref(qg)) == capi.PBD_ERR_UNSUPPORTED and not qg.value
    grp.close()


# ---- 9. latentPositives is its loop of primitives --------------------------------------------------------------------------------------
def test_latent_positives_is_the_loop_of_primitives(gpu_required):
    model = make_model("tree_k")
    minsize = float(np.prod(model.filter_sizes().max(axis=0) * model.sbin))
    items = []
    for seed in (6, 7):
        im, heads, boxes, locs = poses("tree_k", seed, w=200, hgt=150)
        big = np.array([((boxes[i][:heads["nparts"][i], 2] + 1.0) * (boxes[i][:heads["nparts"][i], 3] + 1.0)).min() >= minsize for i in range(len(heads))])
        i = best(heads, big)
        items.append((im, boxes[i][:int(heads["nparts"][i])].copy()))
    small = items[0][1].copy()
    small[1, 2:] = (3, 3)                                          # one part below the minimum area: the item is skipped
    assert 16 < minsize
    items = [items[0], (items[0][0], small), items[1] + (np.full(4, -1, np.int32),)]
    dets = []
    for _ in range(2):
        d = PartsBasedDetector(device=0, max_candidates=MAXC)
        d.distributeModel(model)
        dets.append(d)
    q, t = capi.QpCache(dets[0].handle, CAP, CPOS, CNEG), capi.QpCache(dets[1].handle, CAP, CPOS, CNEG)
    counts, blocks = dets[0].latentPositives(items, q, overlap=0.6, first_id=1)
    want_counts, want = np.zeros(model.ncomponents, np.int64), []
    for i, item in enumerate(items):                               # train.m:172-193, written out
        im, truth = item[0], np.asarray(item[1], np.int32)
        if ((truth[:, 2] + 1.0) * (truth[:, 3] + 1.0) < minsize).any():
            want.append(None)
            continue
        (x, y, w, hh), rel = capi.croppos(truth, len(truth), im.shape[1], im.shape[0])
        blk = t.write_latent(im[y:y + hh, x:x + w], rel, 0.6, i + 1, item[2] if len(item) > 2 else None)
        want.append(blk)
        if blk["found"]:
            want_counts[int(blk["component"])] += 1
    assert counts.tolist() == want_counts.tolist() and counts.sum() == 2
    assert [b is None for b in blocks] == [False, True, False] == [b is None for b in want]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(blocks, want) if a is not None)
    same_caches(q, t, "latentPositives")
    assert q.get()[1][:, :2].tolist() == [[1, 1], [1, 3]]          # the 1-based item index, the skipped item counted
    other = capi.QpCache(dets[1].handle, CAP, CPOS, CNEG)
    with pytest.raises(ValueError):
        dets[0].latentPositives(items, other)
    for d in dets:
        d.handle.close()


# ---- 10. the score identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_score_identity(gpu_required, dtype):
    """train.m:198-204 qp_scorepos: score(qp.w + qp.w0 .* qp.wreg, qp.x, I) / Cpos with qp.w = (weights - w0) .* wreg, so the vector is
    weights .* wreg and the written column Cpos x / wreg scores Cpos (weights . x): the record's own score.  The tolerance is the sum of
    the two bounds the existing tests hold the two halves of this identity to, not a new one:
      the written example against the dense feature vector — tests/test_qp_cpu.py
        test_a_written_example_scores_like_the_dense_feature_vector: (2^-24 + (n + 7) u) sum |terms|, here divided by Cpos;
      the dense feature vector against the record's score — tests/test_gpu_feature_vector.py test_wx_reproduces_the_score:
        part_scores_ref.bound + feature_vector_ref.window_bounds (exact bank, dt_correct_ptr = 1);
    and 2^-24 |score| for the head's float32 score."""
    U = 2.0 ** -53
    kw = dict(conv_mode=capi.PBD_CONV_EXACT, dt_correct_ptr=1)
    model = make_model("tree_k")
    im, heads, boxes, locs = poses("tree_k", 3)
    truth = truth_of(model, heads, boxes, best(heads))
    h = handle(model, dtype, **kw)
    q = capi.QpCache(h, CAP, CPOS, CNEG)
    blk = q.write_latent(im, truth, 0.7, 1)
    assert blk["written"] == 1
    w, wreg, w0, _ = model.qp_vectors()
    got = float(q.score(w * wreg)[0]) / CPOS
    g = handle(model, dtype, **kw)
    hd, _, lc = g.detect_latent(im, truth, 0.7)
    check_block(blk, hd, lc, 1)
    fb, fw = g.candidates_features(hd, lc)
    ps = g.candidates_part_scores(hd, lc)
    dense = dense_feature_vectors(model, fb, fw)[0]
    nz = np.flatnonzero(dense)
    terms = w[nz] * dense[nz]
    tol = (2.0 ** -24 + (len(nz) + 7) * U) * math.fsum(np.abs(terms).tolist()) * (1 + 1e-6)
    tol += float((ps_bound(ps, hd["nparts"], dtype) + window_bounds(model, fb, fw, dtype))[0]) + 2.0 ** -24 * abs(float(blk["score"]))
    err = abs(got - float(blk["score"]))
    print(f"LATENT-WRITE score identity {np.dtype(dtype).name}: score {float(blk['score']):.9g} from the cache {got:.9g} error {err:.3e} tolerance {tol:.3e}")
    assert tol < 1e-3 * (1 + abs(float(blk["score"]))), "the composed bound says nothing at this size"
    assert err <= tol
    h.close(); g.close()


# ---- 11. the C++ host layer ------------------------------------------------------------------------------------------------------------
def test_cpp_demo_poslatent(gpu_required, tmp_path):
    """host/demo.cpp --poslatent FILE x,y,w,h;... (pbd::PartsBasedDetector::latentPositives): the block is the binding's for the same frame"""
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "host", "pbd_demo")
    assert os.path.exists(exe), "build() did not produce the C++ demo"
    model = make_model("tree_k")
    minsize = float(np.prod(model.filter_sizes().max(axis=0) * model.sbin))
    im, heads, boxes, locs = poses("tree_k", 6, w=200, hgt=150)
    big = np.array([((boxes[i][:heads["nparts"][i], 2] + 1.0) * (boxes[i][:heads["nparts"][i], 3] + 1.0)).min() >= minsize for i in range(len(heads))])
    i = best(heads, big)
    truth = boxes[i][:int(heads["nparts"][i])]
    model.save(str(tmp_path / "model.bin"))
    im.tofile(str(tmp_path / "f0.raw"))
    # a second item one pixel below the minimum area in one part — (18 + 1) * (20 + 1) = 399 < 400 —: skipped on both sides
    assert minsize == 400.0
    small = truth.copy()
    small[1, 2:] = (18, 20)

    def arg_of(t):
        return ";".join(",".join(str(int(v)) for v in row) for row in t)

    out = subprocess.run([exe, str(tmp_path / "model.bin"), str(tmp_path / "f0.raw"), "200", "150", "3", "--poslatent", str(tmp_path / "f0.raw"),
                          arg_of(truth), "--poslatent", str(tmp_path / "f0.raw"), arg_of(small)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    det = PartsBasedDetector(device=0, conv_mode=capi.PBD_CONV_EXACT)
    det.distributeModel(model)
    q = capi.QpCache(det.handle, 256, 1.0, 1.0)
    counts, blocks = det.latentPositives([(im, truth), (im, small)], q, overlap=0.6, first_id=1)
    b = blocks[0]
    assert b is not None and b["found"] == 1 and blocks[1] is None
    assert "Poslatent 1: skipped (a box below the minimum area)" in out.stdout.splitlines(), out.stdout
    at_min = truth.copy()
    at_min[1, 2:] = (19, 19)                                       # (19 + 1) * (19 + 1) = 400: not below, not skipped
    assert det.latentPositives([(im, at_min)], capi.QpCache(det.handle, 4, 1.0, 1.0), overlap=0.6)[1][0] is not None
    line = (f"Poslatent 0: found {int(b['found'])} written {int(b['written'])} component {int(b['component'])} level {int(b['level'])} "
            f"x {int(b['x'])} y {int(b['y'])} score {'%.17g' % float(b['score'])}")
    assert line in out.stdout.splitlines(), out.stdout
    assert "Positives per component: " + " ".join(str(int(c)) for c in counts) in out.stdout
    assert f"Cache: {q.dims()[3]} of 256 examples" in out.stdout
    det.handle.close()
