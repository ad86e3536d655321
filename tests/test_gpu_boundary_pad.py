"""Boundary padding (pbd_set_boundary_pad) on the GPU against the composed oracle of tests/boundary_pad_ref.py: bit-exact parity of
the VALU path, the default bank within the project's tolerances, a detection that reaches over the frame border, every detect path
against the single-frame result, and the interplay with the other opt-in steps."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_person_model, make_tree_model, make_tree_model_k
from tests import boundary_pad_ref as bp
from tests import depth_ref, nms_ref
from tests.part_scores_ref import bound, totals
from tests.util import assert_candidates_equal

pytestmark = pytest.mark.gpu
W, H = 200, 150
CAP = 8192


def composed(model, im, pad, pct=99.5, dtype=np.float32, correct_ptr=0, levels=None):
    """the composed oracle with the threshold at a percentile of its own (padded) root scores"""
    model.thresh = -1e30
    c = bp.compose(model, im, pad, dtype, correct_ptr, levels, capacity=1)
    model.thresh = float(np.float32(np.percentile(np.concatenate([r.ravel() for r in c.rootv if r is not None]), pct)))
    return bp.compose(model, im, pad, dtype, correct_ptr, levels, capacity=CAP)


def same(a, b, what=""):
    assert len(a[0]) == len(b[0]), (what, len(a[0]), len(b[0]))
    assert_candidates_equal(a, b, score_tol=0.0)


def person():
    return make_person_model(K=2)


def uneven():
    return make_tree_model_k([-1, 0, 0, 1, 1], [2, 3, 1, 4, 2], seed=13)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("pad", [1, 3])
@pytest.mark.parametrize("kind", ["person", "uneven"])
def test_exact_bank_is_bit_identical_to_the_composed_oracle(gpu_required, kind, pad, dtype):
    model = person() if kind == "person" else uneven()
    im = make_image(4, W, H)
    ref = composed(model, im, pad, dtype=dtype)
    assert len(ref.heads) > 10
    h = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, max_candidates=CAP)
    h.set_boundary_pad(pad)
    assert h.boundary_pad == pad
    h.pyramid(im)
    g = h._geo
    assert g["nlevels"] == ref.nlevels
    nf = len(model.filtersw)
    for l in range(ref.nlevels):
        assert (g["cell_h"][l], g["cell_w"][l]) == ref.feat[l].shape[:2]           # padded planes
        np.testing.assert_array_equal(h.level_features(l), ref.feat[l])
    np.testing.assert_array_equal(g["scales"], np.asarray(ref.scales, np.float32))
    h.pdf()
    for l in (0, 3, ref.nlevels // 2, ref.nlevels - 1):
        if ref.resp[l] is None:
            continue
        for n in (0, nf // 2, nf - 1):
            np.testing.assert_array_equal(h.level_response(l, n), ref.resp[l][n])
    got = h.detect(im, CAP)
    same(got, (ref.heads, ref.boxes, ref.locs))
    h._geo = h.geometry(W, H)
    for l in (0, 5, ref.nlevels - 1):
        if ref.rootv[l] is not None:
            np.testing.assert_array_equal(h.root(l, 0)[0], ref.rootv[l][0])
    h.close()


def test_default_bank_within_the_project_tolerances(gpu_required):
    model = make_person_model()
    im = make_image(6, W, H)
    ref = composed(model, im, 3)
    h = capi.Handle(model, max_candidates=CAP)          # PBD_CONV_AUTO: the split-product bank
    assert h.conv_mode == capi.PBD_CONV_SPLIT
    h.set_boundary_pad(3)
    h.pyramid(im)
    h.pdf()
    nf = len(model.filtersw)
    worst = 0.0
    for l in range(ref.nlevels):
        if ref.resp[l] is None:
            continue
        np.testing.assert_array_equal(h.level_features(l), ref.feat[l])
        for n in (0, 77, nf - 1):
            worst = max(worst, float(np.abs(h.level_response(l, n) - ref.resp[l][n]).max()))
    print(f"padded responses: worst |device - oracle| = {worst:.3e}")
    assert worst < 2e-5
    got = h.detect(im, CAP)
    at = {(int(got[0]["level"][i]), int(got[0]["component"][i]), int(got[2][i, 0, 1]), int(got[2][i, 0, 0])): i for i in range(len(got[0]))}
    sure = 0
    for i in range(len(ref.heads)):
        if ref.heads["score"][i] <= model.thresh + 1e-4:
            continue
        sure += 1
        key = (int(ref.heads["level"][i]), int(ref.heads["component"][i]), int(ref.locs[i, 0, 1]), int(ref.locs[i, 0, 0]))
        assert key in at, key
        j = at[key]
        assert abs(float(got[0]["score"][j]) - float(ref.heads["score"][i])) <= 1e-4
        np.testing.assert_array_equal(got[1][j, 0], ref.boxes[i, 0])
    assert sure > 10
    h.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_detection_reaches_over_the_frame_border(gpu_required, dtype):
    """A model whose last channel is a positive "outside the image" weight: the composed oracle itself returns candidates whose root
    cell lies in the padding ring, clear of the threshold, with root boxes that start at a negative coordinate or end beyond the
    frame — and the device returns exactly them.  Without the step no root box can start before -scale."""
    w, hgt, pad = 160, 120, 3
    im = make_image(11, w, hgt)
    model = bp.occlusion_trained(make_tree_model([-1, 0, 0], 2, seed=21))
    ref = composed(model, im, pad, pct=99.0, dtype=dtype)
    ring = []
    for i in range(len(ref.heads)):
        l = ref.heads["level"][i]
        Hl, Wl = ref.rootv[l].shape[1:]
        x, y = ref.locs[i, 0, :2]
        bx, by, bw, bh = ref.boxes[i, 0]
        if (x < pad or y < pad or x >= Wl - pad or y >= Hl - pad) and (bx < -ref.scales[l] or by < -ref.scales[l] or bx + bw >= w or by + bh >= hgt) \
                and ref.heads["score"][i] > model.thresh + 0.01:
            ring.append(i)
    assert len(ring) > 0
    h = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, max_candidates=CAP)
    h.set_boundary_pad(pad)
    got = h.detect(im, CAP)
    same(got, (ref.heads, ref.boxes, ref.locs))
    for i in ring[:50]:
        np.testing.assert_array_equal(got[1][i], ref.boxes[i])
        assert got[0]["score"][i] == ref.heads["score"][i]
    h.set_boundary_pad(0)
    off = h.detect(im, CAP)
    assert all(off[1][i, 0, 0] >= -np.ceil(ref.scales[off[0]["level"][i]]) for i in range(len(off[0])))
    h.close()


def test_every_path_gives_the_single_frame_result(gpu_required):
    import torch
    model = make_person_model()
    frames = [make_image(20 + i, W, H) for i in range(4)]
    composed(model, frames[0], 3, pct=99.0)                  # (sets the threshold, from frame 0's padded root scores)
    h = capi.Handle(model, max_candidates=CAP)
    h.set_boundary_pad(3)
    refs = [h.detect(f, CAP) for f in frames]               # two and more different frames in a row on one handle
    print("candidates per frame:", [len(r[0]) for r in refs])
    assert len(refs[0][0]) > 20 and all(len(r[0]) > 0 for r in refs)
    fresh = capi.Handle(model, max_candidates=CAP)
    fresh.set_boundary_pad(3)
    for f in (3, 0):
        same(fresh.detect(frames[f], CAP), refs[f], "a frame's result does not depend on what ran before it")
    fresh.close()
    # enqueue / collect, a device-resident image
    h.enqueue(frames[1])
    with pytest.raises(capi.PbdError) as e:
        h.set_boundary_pad(0)
    assert e.value.code == capi.PBD_ERR_STATE and h.boundary_pad == 3
    same(h.collect(CAP), refs[1], "enqueue / collect")
    d = torch.from_numpy(frames[2]).cuda()
    same(h.detect_dev(d.data_ptr(), W, H, 3, capacity=CAP), refs[2], "device image")
    # a caller's border, then the rule's border again
    h.pyramid(frames[0])
    f0 = h.level_features(0)
    mine = f0.copy()
    mine[:3] = 0.25
    mine[:, :3] = 0.25
    h.set_level_features(0, mine)
    np.testing.assert_array_equal(h.level_features(0), mine)   # the caller's border as given
    h.pdf()
    assert np.abs(h.level_response(0, 0)[:6, :6] - bp.orc.pdf_level(mine, model.filtersw)[0][:6, :6]).max() < 2e-5
    same(h.detect(frames[0], CAP), refs[0], "after a caller's border")
    h.pyramid(frames[0])
    np.testing.assert_array_equal(h.level_features(0), f0)
    # batches, eager and replayed
    for graph in (0, 1):
        hb = capi.Handle(model, max_candidates=4 * CAP, graph=graph)
        hb.set_boundary_pad(3)
        for _ in range(3):
            got = hb.detect_batch(frames, CAP)
            for f in range(4):
                same(got[f], refs[f], ("batch", graph, f))
        for _ in range(3):
            same(hb.detect(frames[1], CAP), refs[1], ("single, graph", graph))
        hb.close()
    # compact plan
    hc = capi.Handle(model, max_candidates=CAP, dp_mode=2)
    hc.set_boundary_pad(3)
    for f in (0, 1, 0):
        same(hc.detect(frames[f], CAP), refs[f], ("compact", f))
    hc.close()
    # a level set
    levels = [0, 3, 7, 12]
    h.set_levels(levels)
    k = np.isin(refs[0][0]["level"], levels)
    same(h.detect(frames[0], CAP), (refs[0][0][k], refs[0][1][k], refs[0][2][k]), "level set")
    h.set_levels([])
    # toggling 3 -> 0 -> 3
    never = capi.Handle(model, max_candidates=CAP)
    plain = never.detect(frames[0], CAP)
    assert never.boundary_pad == 0
    never.close()
    h.set_boundary_pad(0)
    same(h.detect(frames[0], CAP), plain, "3 -> 0")
    h.set_boundary_pad(3)
    same(h.detect(frames[0], CAP), refs[0], "0 -> 3")
    for bad in (-1, 9):
        with pytest.raises(capi.PbdError) as e:
            h.set_boundary_pad(bad)
        assert e.value.code == capi.PBD_ERR_ARG and h.boundary_pad == 3
    h.close()
    # a group of two members on one GPU
    g = capi.Group(model, [0, 0], gather=capi.PBD_GATHER_HOST, max_candidates=CAP)
    with pytest.raises(capi.PbdError) as e:
        g.set_boundary_pad(9)
    assert e.value.code == capi.PBD_ERR_ARG
    g.set_boundary_pad(3)
    for i in range(2):
        assert capi.lib().pbd_get_boundary_pad(C.c_void_p(capi.lib().pbd_group_member(g.g, i))) == 3
    got = g.detect_batch(frames, CAP)
    for f in range(4):
        same(got[f], refs[f], ("group batch", f))
    same(g.detect(frames[0], CAP), refs[0], "group, level shards")
    g.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sixteen_bit_image(gpu_required, dtype):
    model = uneven()
    im = (make_image(8, W, H).astype(np.uint16) * 257)
    ref = composed(model, im, 3, dtype=dtype)
    assert len(ref.heads) > 10
    h = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, max_candidates=CAP)
    h.set_boundary_pad(3)
    same(h.detect_image(im, CAP), (ref.heads, ref.boxes, ref.locs))
    h.close()


def test_score_map_nms_on_padded_root_planes(gpu_required, orc):
    model = person()
    im = make_image(9, W, H)
    ref = composed(model, im, 3, pct=97.0)
    sz = 2
    masks = [None if r is None else np.stack([orc.nms_map(r[c], sz) for c in range(r.shape[0])]) for r in ref.rootv]
    for l in (0, 4):
        np.testing.assert_array_equal(masks[l][0], nms_ref.nms_map(ref.rootv[l][0], sz))
    k = np.array([bool(masks[ref.heads["level"][i]][ref.heads["component"][i]][ref.locs[i, 0, 1], ref.locs[i, 0, 0]]) for i in range(len(ref.heads))])
    assert 0 < k.sum() < len(k)
    h = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, max_candidates=CAP, nms_sz=sz)
    h.set_boundary_pad(3)
    same(h.detect(im, CAP), (ref.heads[k], ref.boxes[k], ref.locs[k]))
    h.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_part_scores_rescore_padded_detections(gpu_required, dtype):
    """oracle-free: with dt_correct_ptr = 1 the parts' scores, read at the padded locs from the padded planes, add up to the root score"""
    model = person()
    im = make_image(10, W, H)
    composed(model, im, 3, dtype=dtype, correct_ptr=1)
    h = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, dt_correct_ptr=1, max_candidates=CAP)
    h.set_boundary_pad(3)
    h.set_part_scores(True)
    heads, boxes, locs = h.detect(im, CAP)
    n = len(heads)
    assert n > 10
    ps = h.part_scores(0)
    total, B = totals(ps), bound(ps, heads["nparts"], dtype)
    score = heads["score"].astype(np.float64)
    if np.dtype(dtype) == np.dtype(np.float64):
        h._geo = h.geometry(W, H)
        roots = {}
        for i in range(n):
            key = (int(heads["level"][i]), int(heads["component"][i]))
            if key not in roots:
                roots[key] = h.root(*key)[0]
            score[i] = roots[key][locs[i, 0, 1], locs[i, 0, 0]]
    r = np.abs(total - score) / B
    print(f"padded {np.dtype(dtype).name}: {n} detections, worst |total - score| / B = {r.max():.3f}")
    assert (np.abs(total - score) <= B).all()
    h.close()


def test_candidate_and_depth_filters_on_a_padded_handle(gpu_required, orc):
    model = make_person_model()
    im = make_image(12, W, H)
    composed(model, im, 3, pct=99.0)
    h = capi.Handle(model, max_candidates=CAP)
    h.set_boundary_pad(3)
    raw = h.detect(im, CAP)
    assert len(raw[0]) > 20
    for mode, ov in ((capi.PBD_CAND_SORT, 0.0), (capi.PBD_CAND_SORT_NMS, 0.1)):
        h.set_candidate_filter(mode, ov)
        want = orc.candidates_sort(*raw)
        if mode == capi.PBD_CAND_SORT_NMS:
            want = orc.candidates_nms(*want, W, H, ov)
        got = h.detect(im, CAP)
        same(got, want, (mode, ov))
    h.set_candidate_filter(capi.PBD_CAND_RAW)
    rng = np.random.default_rng(5)
    depth = (1.0 + 0.2 * rng.random((H, W))).astype(np.float32)
    depth[:, : W // 3] = 0
    h.set_depth_filter(True, 0.03)
    got = h.detect_rgbd(im, depth, CAP)
    want = depth_ref.depth_filter(model, *raw, depth, 0.03)
    assert 0 < len(want[0]) <= len(raw[0])
    same(got, want, "depth filter")
    h.close()
