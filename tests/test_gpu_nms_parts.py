"""The part-wise overlap NMS of matlab/detection/nms.m on the device (k_cand_parts.hip behind k_cand_filter's sort), against the host
functions: every result is bit-identical (heads, boxes, locs, counts) to pbd_candidates_sort then pbd_candidates_nms_parts applied to
the unfiltered output of the same handle — or, for the stand-alone primitive, to the caller's records."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_mixed_person_model, make_person_model, make_tree_model
from tests import nms_parts_ref as ref

pytestmark = pytest.mark.gpu

W, H = 640, 480
OVERLAPS = (-0.5, 0.0, 0.3, 1.0, 3.0)
NMS = capi.PBD_CAND_SORT_NMS


def expected(raw, ov, top):
    return capi.candidates_nms_parts(*capi.candidates_sort(*raw), ov, top)


def assert_same(got, exp, what=""):
    assert len(got[0]) == len(exp[0]), (what, len(got[0]), len(exp[0]))
    assert got[0].tobytes() == np.ascontiguousarray(exp[0]).tobytes(), what
    assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]), what


# ---- the stand-alone primitive ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    h = capi.Handle(make_tree_model([-1, 0, 1, 1, 0], 3, seed=5), conv_mode=capi.PBD_CONV_EXACT)
    yield h
    h.close()


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1000, 1001, 1025, 4097])
def test_primitive_matches_host_functions(gpu_required, small, n):
    assert small.max_parts == 5
    recs = ref.records(n * 7 + 3, n, small.max_parts)
    srt = capi.candidates_sort(*recs)
    for top in (0, 7, 1000):
        for ov in OVERLAPS:
            got = small.candidates_filter_parts(*recs, ov, top)
            assert_same(got, capi.candidates_nms_parts(*srt, ov, top), (n, top, ov))
    if n in (65, 1001):   # ... and the host function is the definition
        srt[0]["level"] = np.arange(n)
        for ov in (0.0, 0.3):
            assert [int(v) for v in capi.candidates_nms_parts(*srt, ov, 1000)[0]["level"]] == ref.nms_parts_def(srt[0], srt[1], ov, 1000)


def test_primitive_argument_errors(gpu_required, small):
    heads, boxes, locs = ref.records(3, 8, small.max_parts)
    bad_score = [heads.copy(), heads.copy()]
    bad_score[0]["score"][3] = np.nan
    bad_score[1]["score"][3] = np.inf
    bad_np = [heads.copy(), heads.copy()]
    bad_np[0]["nparts"][0] = small.max_parts + 1
    bad_np[1]["nparts"][7] = -1
    for args in ((bad_score[0], boxes, locs, 0.3, 0), (bad_score[1], boxes, locs, 0.3, 0), (bad_np[0], boxes, locs, 0.3, 0),
                 (bad_np[1], boxes, locs, 0.3, 0), (heads, None, locs, 0.3, 0), (heads, boxes, locs, 0.3, -1),
                 (heads, boxes, locs, float("nan"), 0), (heads, boxes, locs, float("inf"), 0)):
        with pytest.raises(capi.PbdError) as e:
            small.candidates_filter_parts(*args)
        assert e.value.code == capi.PBD_ERR_ARG
    got = small.candidates_filter_parts(heads, boxes, None, 0.3, 0)   # locs are optional
    assert got[0].tobytes() == expected((heads, boxes, locs), 0.3, 0)[0].tobytes()


# ---- whole path ---------------------------------------------------------------------------------------------------------------
def bench_threshold(model, w, hgt, dtype=np.float32):
    """bench.py's threshold: the 99.9th percentile of component 0's root scores of the seed frame."""
    model.thresh = 3.0e38
    h = capi.Handle(model, dtype=dtype)
    im = make_image(0, w, hgt)
    h.detect(im)
    h._geo = h.geometry(w, hgt)
    vals = np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])])
    h.close()
    return float(np.float32(np.percentile(vals, 99.9)))


@pytest.fixture(scope="module")
def person():
    m = make_person_model()
    m.thresh = bench_threshold(m, W, H)
    return m


SETTINGS = ((0.3, 1000), (0.0, 0), (0.3, 7), (-0.5, 1000), (1.0, 1000))


def check(h, call, settings=SETTINGS):
    h.set_candidate_filter(capi.PBD_CAND_RAW)
    raw = call()
    assert len(raw[0]) > 20
    for ov, top in settings:
        h.set_candidate_filter(NMS, ov)
        h.set_candidate_nms(capi.PBD_NMS_PARTS, top)
        assert_same(call(), expected(raw, ov, top), (ov, top))
    h.set_candidate_filter(capi.PBD_CAND_RAW)
    h.set_candidate_nms(capi.PBD_NMS_PAINTED, 0)
    return raw


def test_not_vacuous(gpu_required, orc, person):
    """the CPU oracle's raw output of the tested frame: the parts NMS keeps some, not all, and not what the painted mask keeps"""
    im = make_image(1, W, H)
    raw = orc.detect(person, im)[:3]
    srt = orc.candidates_sort(*raw)
    parts = capi.candidates_nms_parts(*srt, 0.3, 1000)
    painted = orc.candidates_nms(*srt, W, H, 0.3)
    assert 1 < len(parts[0]) < len(raw[0])
    assert parts[0].tobytes() != np.ascontiguousarray(painted[0]).tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_frame_entry_points(gpu_required, person, dtype):
    import torch
    im = make_image(1, W, H)
    h = capi.Handle(person, dtype=dtype)
    raw = check(h, lambda: h.detect(im))
    exp = expected(raw, 0.3, 1000)
    assert 1 < len(exp[0]) < len(raw[0])
    srt = capi.candidates_sort(*raw)
    srt[0]["level"] = np.arange(len(srt[0]))
    assert [int(v) for v in capi.candidates_nms_parts(*srt, 0.3, 1000)[0]["level"]] == ref.nms_parts_def(srt[0], srt[1], 0.3, 1000)
    d = torch.from_numpy(im).cuda()
    check(h, lambda: h.detect_dev(d.data_ptr(), W, H, 3), SETTINGS[:2])

    def enq():
        h.enqueue(im)
        return h.collect()
    check(h, enq, SETTINGS[:2])
    imd = (im.astype(np.float64) * 257).astype(np.uint16)
    check(h, lambda: h.detect_image(imd), SETTINGS[:2])
    h.close()


@pytest.mark.parametrize("graph", [0, 1])
def test_batch_of_three(gpu_required, person, graph):
    frames = [make_image(i, W, H) for i in range(3)]
    h = capi.Handle(person, graph=graph, max_candidates=32768)
    raw = h.detect_batch(frames)
    h.set_candidate_filter(NMS, 0.3)
    for top in (1000, 7):
        h.set_candidate_nms(capi.PBD_NMS_PARTS, top)
        for _ in range(3):   # eager, captured, replayed
            got = h.detect_batch(frames)
            for f in range(3):
                assert_same(got[f], expected(raw[f], 0.3, top), (f, top))
    h.close()


def test_mixed_bank_and_double_handle(gpu_required):
    m = make_mixed_person_model(seed=5, K=2)
    m.thresh = bench_threshold(m, W, H)
    im = make_image(2, W, H)
    h = capi.Handle(m)
    check(h, lambda: h.detect(im), SETTINGS[:3])
    h.close()


def test_switching_kinds_on_a_replaying_handle(gpu_required, orc, person):
    im = make_image(3, W, H)
    h = capi.Handle(person, graph=1)
    raw = [h.detect(im) for _ in range(2)][-1]
    srt = orc.candidates_sort(*raw)
    parts, painted = expected(raw, 0.3, 1000), orc.candidates_nms(*srt, W, H, 0.3)
    h.set_candidate_filter(NMS, 0.3)
    for kind in (capi.PBD_NMS_PARTS, capi.PBD_NMS_PAINTED, capi.PBD_NMS_PARTS):
        h.set_candidate_nms(kind, 1000)
        for _ in range(3):
            assert_same(h.detect(im), parts if kind == capi.PBD_NMS_PARTS else painted, kind)
    h.set_candidate_filter(capi.PBD_CAND_SORT)   # the kind only matters in mode 2
    assert_same(h.detect(im), srt, "sort")
    h.close()


def test_refusals(gpu_required, person):
    im = make_image(1, W, H)
    h = capi.Handle(person)
    for bad in ((2, 0), (-1, 0), (capi.PBD_NMS_PARTS, -1)):
        with pytest.raises(capi.PbdError) as e:
            h.set_candidate_nms(*bad)
        assert e.value.code == capi.PBD_ERR_ARG
    h.enqueue(im)
    with pytest.raises(capi.PbdError) as e:
        h.set_candidate_nms(capi.PBD_NMS_PARTS, 1000)
    assert e.value.code == capi.PBD_ERR_STATE
    h.collect()
    with pytest.raises(capi.PbdError) as e:
        h.set_candidate_filter(3, 0.3)   # no new mode value
    assert e.value.code == capi.PBD_ERR_ARG
    h.close()
    g = capi.Group(person, [0, 0], gather=capi.PBD_GATHER_HOST)
    member = C.c_void_p(capi.lib().pbd_group_member(g.g, 0))
    assert capi.lib().pbd_set_candidate_nms(member, 1, 1000) == capi.PBD_ERR_STATE
    for bad in ((2, 0), (1, -1)):
        with pytest.raises(capi.PbdError) as e:
            g.set_candidate_nms(*bad)
        assert e.value.code == capi.PBD_ERR_ARG
    g.close()


def _detect_raw_call(h, im, capacity):   # (status, *count) of pbd_detect_u8
    heads, boxes, locs = h._bufs(max(capacity, 1))
    cnt = C.c_int(-1)
    rc = h.L.pbd_detect_u8(h.h, im.ctypes.data_as(C.POINTER(C.c_uint8)), W, H, 3, W * 3, heads.ctypes.data_as(C.c_void_p),
                           boxes.ctypes.data_as(C.POINTER(C.c_int32)), locs.ctypes.data_as(C.POINTER(C.c_int32)), capacity,
                           C.byref(cnt))
    return rc, cnt.value


def test_capacity(gpu_required, person):
    im = make_image(1, W, H)
    h = capi.Handle(person)
    raw = h.detect(im)
    n = len(raw[0])
    h.close()
    small = capi.Handle(person, max_candidates=n - 1, cand_filter=(NMS, 0.3), cand_nms=(capi.PBD_NMS_PARTS, 1000))
    assert _detect_raw_call(small, im, 4096) == (capi.PBD_ERR_CAPACITY, n)      # records overflow the device list
    small.close()
    h = capi.Handle(person, cand_filter=(NMS, 0.3), cand_nms=(capi.PBD_NMS_PARTS, 1000))
    kept = len(expected(raw, 0.3, 1000)[0])
    assert _detect_raw_call(h, im, kept - 1) == (capi.PBD_ERR_CAPACITY, kept)   # kept records overflow the caller's
    assert _detect_raw_call(h, im, kept) == (capi.PBD_OK, kept)
    h.close()


def test_group_batch_and_level_shards(gpu_required, person):
    frames = [make_image(i, W, H) for i in range(3)]
    g = capi.Group(person, [0, 0], gather=capi.PBD_GATHER_HOST)
    raw_b = g.detect_batch(frames)
    raw_1 = g.detect(frames[0])
    g.set_candidate_filter(NMS, 0.3)
    for top in (1000, 7):
        g.set_candidate_nms(capi.PBD_NMS_PARTS, top)
        for _ in range(2):
            got = g.detect_batch(frames)
            for f in range(3):
                assert_same(got[f], expected(raw_b[f], 0.3, top), (f, top))
            assert_same(g.detect(frames[0]), expected(raw_1, 0.3, top), ("sharded", top))
    g.close()


def test_rgbd_frame_with_the_depth_filter(gpu_required, person):
    from tests.test_gpu_depth_filter import scene
    im = make_image(1, W, H)
    depth = scene(1, W, H, np.float32)
    h = capi.Handle(person)
    h.set_depth_filter(True, 0.03)
    pruned = h.detect_rgbd(im, depth)
    assert 20 < len(pruned[0]) < len(h.detect(im)[0])
    h.set_candidate_filter(NMS, 0.3)
    h.set_candidate_nms(capi.PBD_NMS_PARTS, 1000)
    exp = expected(pruned, 0.3, 1000)
    assert 1 < len(exp[0]) < len(pruned[0])
    assert_same(h.detect_rgbd(im, depth), exp, "rgbd")
    h.close()


def test_latent_frame(gpu_required, orc):
    from tests.test_gpu_latent import _frame_truth, _tree
    model = _tree("M4", 83)
    im = make_image(54, 160, 120)
    truth = _frame_truth(orc, model, im, 5, (9, 7))
    h = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT)
    raw = h.detect_latent(im, truth, 0.4)
    assert len(raw[0]) == 1
    h.set_candidate_filter(NMS, 0.3)
    h.set_candidate_nms(capi.PBD_NMS_PARTS, 1000)
    assert_same(h.detect_latent(im, truth, 0.4), raw, "latent")
    h.close()


def test_part_scores_follow_the_kept_records(gpu_required, person):
    im = make_image(1, W, H)
    h = capi.Handle(person, cand_filter=(NMS, 0.3), cand_nms=(capi.PBD_NMS_PARTS, 1000))
    h.set_part_scores(True)
    heads, boxes, locs = h.detect(im)
    ps = h.part_scores(0)
    assert 1 < len(heads) == len(ps)
    assert np.array_equal(ps, h.candidates_part_scores(heads, locs))   # ... of the host-selected records, by the stand-alone primitive
    h.close()
