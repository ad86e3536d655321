"""Candidate::sort + Candidate::nonMaximaSuppression on the device (k_cand.hip), against the oracle's host functions.

Every result must be bit-identical (heads, boxes, locs, counts) to orc.candidates_sort, then (mode 2) orc.candidates_nms with the
frame's size, applied to the unfiltered output of the same handle — or, for the stand-alone primitive, to the caller's records."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_mixed_person_model, make_person_model, make_tree_model

pytestmark = pytest.mark.gpu

W, H = 640, 480
OVERLAPS = (-0.5, 0.0, 0.1, 0.2, 0.5, 0.999, 1.0, 3.0)
MODES = ((capi.PBD_CAND_SORT, 0.0), (capi.PBD_CAND_SORT_NMS, 0.0), (capi.PBD_CAND_SORT_NMS, 0.1), (capi.PBD_CAND_SORT_NMS, 0.3))


def expected(orc, res, mode, overlap, w, hgt):
    h, b, l = orc.candidates_sort(*res)
    if mode == capi.PBD_CAND_SORT_NMS:
        h, b, l = orc.candidates_nms(h, b, l, w, hgt, overlap)
    return h, b, l


def assert_same(got, exp, what=""):
    assert len(got[0]) == len(exp[0]), (what, len(got[0]), len(exp[0]))
    assert got[0].tobytes() == np.ascontiguousarray(exp[0]).tobytes(), what
    assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]), what


# ---- the stand-alone primitive on adversarial record sets ----------------------------------------------------------------
def records(seed, n, mp, w, hgt):
    rng = np.random.default_rng(seed)
    heads = np.zeros(n, capi.HEAD_DTYPE)
    ties = np.array([0.0, -0.0, 1.5, -2.25, 0.5], np.float32)
    sc = rng.normal(0, 2, n).astype(np.float32)
    pick = rng.random(n) < 0.4
    sc[pick] = ties[rng.integers(0, len(ties), pick.sum())]
    heads["score"] = sc
    heads["component"] = rng.integers(0, 3, n)
    heads["level"] = rng.integers(0, 40, n)
    heads["nparts"] = rng.integers(0, mp + 1, n)
    big = 200 if n <= 4096 else 48
    boxes = np.zeros((n, mp, 4), np.int32)
    boxes[..., 0] = rng.integers(-big, w + big // 2, (n, mp))
    boxes[..., 1] = rng.integers(-big, hgt + big // 2, (n, mp))
    boxes[..., 2] = rng.integers(-3, big, (n, mp))
    boxes[..., 3] = rng.integers(-3, big, (n, mp))
    junk = np.arange(mp)[None, :] >= np.maximum(heads["nparts"], 1)[:, None]   # unused slots beyond nparts: junk
    boxes[junk] = rng.integers(-2**30, 2**30, (int(junk.sum()), 4))
    empty = rng.random(n) < 0.05
    boxes[empty, :, 2] = 0
    locs = rng.integers(-1000, 1000, (n, mp, 3)).astype(np.int32)
    return heads, boxes, locs


@pytest.fixture(scope="module")
def small():
    h = capi.Handle(make_tree_model([-1, 0, 1, 1, 0], 3, seed=5), conv_mode=capi.PBD_CONV_EXACT)
    yield h
    h.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 4096, 32768])
@pytest.mark.parametrize("size", [(640, 480), (1920, 1080), (641, 37)])
def test_primitive_matches_host_functions(gpu_required, orc, small, n, size):
    w, hgt = size
    recs = records(n * 7 + w, n, small.max_parts, w, hgt)
    got = small.candidates_filter(*recs, w, hgt, capi.PBD_CAND_SORT, 0.0)
    srt = orc.candidates_sort(*recs)
    assert_same(got, srt, "sort")
    for ov in (OVERLAPS if n <= 4096 else (0.0, 0.2, 1.0)):
        got = small.candidates_filter(*recs, w, hgt, capi.PBD_CAND_SORT_NMS, ov)
        assert_same(got, orc.candidates_nms(*srt, w, hgt, ov), f"nms {ov}")


def test_primitive_argument_errors(gpu_required, small):
    heads, boxes, locs = records(3, 8, small.max_parts, W, H)
    for bad in (np.nan, np.inf):
        h2 = heads.copy()
        h2["score"][3] = bad
        with pytest.raises(capi.PbdError) as e:
            small.candidates_filter(h2, boxes, locs, W, H, capi.PBD_CAND_SORT, 0.0)
        assert e.value.code == capi.PBD_ERR_ARG
    h2 = heads.copy()
    h2["nparts"][0] = small.max_parts + 1
    for args in ((heads, boxes, locs, W, H, 3, 0.0), (heads, boxes, locs, W, H, 2, float("nan")), (h2, boxes, locs, W, H, 2, 0.1),
                 (heads, boxes, locs, 0, H, 2, 0.1), (heads, None, locs, W, H, 2, 0.1)):
        with pytest.raises(capi.PbdError) as e:
            small.candidates_filter(*args)
        assert e.value.code == capi.PBD_ERR_ARG
    assert small.candidates_filter(heads, None, None, W, H, capi.PBD_CAND_SORT, 0.0)[0].tobytes() == \
        capi.candidates_sort(heads, boxes, locs)[0].tobytes()


# ---- whole path -----------------------------------------------------------------------------------------------------------
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


def check_modes(orc, h, call, w=W, hgt=H, modes=MODES):
    h.set_candidate_filter(capi.PBD_CAND_RAW)
    raw = call()
    assert len(raw[0]) > 20
    for mode, ov in modes:
        h.set_candidate_filter(mode, ov)
        assert_same(call(), expected(orc, raw, mode, ov, w, hgt), (mode, ov))
    h.set_candidate_filter(capi.PBD_CAND_RAW)
    return raw


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_frame_entry_points(gpu_required, orc, person, dtype):
    import torch
    im = make_image(1, W, H)
    h = capi.Handle(person, dtype=dtype)
    check_modes(orc, h, lambda: h.detect(im))
    d = torch.from_numpy(im).cuda()
    check_modes(orc, h, lambda: h.detect_dev(d.data_ptr(), W, H, 3))

    def enq():
        h.enqueue(im)
        return h.collect()
    check_modes(orc, h, enq)
    for dt, scale in ((np.uint16, 257), (np.float32, 1.0 / 255)):
        imd = (im.astype(np.float64) * scale).astype(dt)
        check_modes(orc, h, lambda: h.detect_image(imd), modes=MODES[:3])
    h.close()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("nb", [1, 4, 16])
def test_batches(gpu_required, orc, person, nb, graph):
    frames = [make_image(i, W, H) for i in range(nb)]
    h = capi.Handle(person, graph=graph, max_candidates=32768)   # (the device list holds the whole batch)
    raw = h.detect_batch(frames)
    for mode, ov in MODES[1:3]:
        h.set_candidate_filter(mode, ov)
        for _ in range(3):   # eager, captured, replayed
            got = h.detect_batch(frames)
            for f in range(nb):
                assert_same(got[f], expected(orc, raw[f], mode, ov, W, H), (f, mode, ov))
    h.close()


def test_mixed_bank_and_score_map_nms(gpu_required, orc):
    m = make_mixed_person_model(seed=5, K=2)
    m.thresh = bench_threshold(m, W, H)
    im = make_image(2, W, H)
    h = capi.Handle(m)
    check_modes(orc, h, lambda: h.detect(im))
    h.close()
    p = make_person_model()
    p.thresh = bench_threshold(p, W, H) - 0.5
    h = capi.Handle(p, nms_sz=2)
    check_modes(orc, h, lambda: h.detect(im))
    h.close()


def test_full_hd_frame(gpu_required, orc):
    m = make_person_model()
    m.thresh = bench_threshold(m, 1920, 1080)
    im = make_image(0, 1920, 1080)
    h = capi.Handle(m, max_candidates=32768, graph=1)
    check_modes(orc, h, lambda: h.detect(im, capacity=32768), 1920, 1080, modes=MODES[:3])
    h.close()


def test_toggling_on_a_replaying_handle(gpu_required, orc, person):
    im = make_image(3, W, H)
    h = capi.Handle(person, graph=1)
    raw = h.detect(im)
    raw = h.detect(im)
    for mode, ov in ((capi.PBD_CAND_SORT, 0.0), (capi.PBD_CAND_SORT_NMS, 0.1), (capi.PBD_CAND_SORT_NMS, 0.3)):
        h.set_candidate_filter(mode, ov)
        for _ in range(2):
            assert_same(h.detect(im), expected(orc, raw, mode, ov, W, H), (mode, ov))
    h.set_candidate_filter(capi.PBD_CAND_RAW)
    never = capi.Handle(person, graph=1)
    ref = [never.detect(im) for _ in range(2)][-1]
    for _ in range(2):
        assert_same(h.detect(im), ref, "off")
    never.close()
    # refused while a frame is pending, and on group members
    h.enqueue(im)
    with pytest.raises(capi.PbdError) as e:
        h.set_candidate_filter(capi.PBD_CAND_SORT)
    assert e.value.code == capi.PBD_ERR_STATE
    h.collect()
    h.close()


def _detect_raw_call(h, im, capacity):   # (status, *count) of pbd_detect_u8
    heads, boxes, locs = h._bufs(max(capacity, 1))
    cnt = C.c_int(-1)
    rc = h.L.pbd_detect_u8(h.h, im.ctypes.data_as(C.POINTER(C.c_uint8)), W, H, 3, W * 3, heads.ctypes.data_as(C.c_void_p),
                           boxes.ctypes.data_as(C.POINTER(C.c_int32)), locs.ctypes.data_as(C.POINTER(C.c_int32)), capacity,
                           C.byref(cnt))
    return rc, cnt.value


def test_capacity(gpu_required, orc, person):
    im = make_image(1, W, H)
    h = capi.Handle(person)
    raw = h.detect(im)
    n = len(raw[0])
    h.close()
    assert n > 20
    small = capi.Handle(person, max_candidates=n - 1, cand_filter=(capi.PBD_CAND_SORT_NMS, 0.1))   # records overflow the device list
    assert _detect_raw_call(small, im, 4096) == (capi.PBD_ERR_CAPACITY, n)
    small.close()
    h = capi.Handle(person, cand_filter=(capi.PBD_CAND_SORT_NMS, 0.1))
    kept = len(expected(orc, raw, capi.PBD_CAND_SORT_NMS, 0.1, W, H)[0])
    assert _detect_raw_call(h, im, kept - 1) == (capi.PBD_ERR_CAPACITY, kept)                       # kept records overflow the caller's
    assert _detect_raw_call(h, im, kept) == (capi.PBD_OK, kept)
    h.close()


def test_group_batch_and_level_shards(gpu_required, orc, person):
    frames = [make_image(i, W, H) for i in range(4)]
    g = capi.Group(person, [0, 0], gather=capi.PBD_GATHER_HOST)
    raw_b = g.detect_batch(frames)
    raw_1 = g.detect(frames[0])
    member = capi.lib().pbd_group_member(g.g, 0)
    assert capi.lib().pbd_set_candidate_filter(C.c_void_p(member), 1, C.c_float(0.0)) == capi.PBD_ERR_STATE
    for mode, ov in MODES[1:3]:
        g.set_candidate_filter(mode, ov)
        for _ in range(2):
            got = g.detect_batch(frames)
            for f in range(4):
                assert_same(got[f], expected(orc, raw_b[f], mode, ov, W, H), (f, mode, ov))
            assert_same(g.detect(frames[0]), expected(orc, raw_1, mode, ov, W, H), ("sharded", mode, ov))
    g.set_candidate_filter(capi.PBD_CAND_RAW)
    assert_same(g.detect(frames[0]), raw_1, "off")
    g.close()
