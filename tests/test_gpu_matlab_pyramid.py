"""The MATLAB pyramid kind (pbd_set_pyramid_kind, PBD_PYRAMID_MATLAB; k_pyramid_mat.hip) on the GPU.  Every tolerance on the level
images is "equal bits": against tests/golden/ref_matpyr_v1.npz (outputs of the compiled matlab/mex/resize.cc / reduce.cc) and against
the numpy restatement of tests/matlab_pyramid_ref.py.  Features by the unchanged check_hog, detections against the restatement
composed with the oracle's stage functions, every detect path against the single-frame result, the feature vector's w . x = score,
the refusals, and the default kind after a round trip through the MATLAB kind."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import dense_feature_vectors, make_image, make_tree_model
from tests import depth_ref
from tests import latent_ref as LR
from tests import matlab_pyramid_ref as mp
from tests.feature_vector_ref import window_bounds, wx
from tests.part_scores_ref import bound
from tests.pyramid_cases import noise
from tests.pyramid_checks import check_geometry, check_hog
from tests.test_matlab_pyramid_cpu import GOLDEN, same_bits
from tests.util import assert_candidates_equal

pytestmark = pytest.mark.gpu
MATLAB, OPENCV = capi.PBD_PYRAMID_MATLAB, capi.PBD_PYRAMID_OPENCV
W, H = mp.PYRAMID_FRAME[1:]          # 96 x 80
CAP = 8192


def small_model(interval=2, seed=7):
    return make_tree_model([-1, 0, 0, 1], 2, seed=seed, sbin=mp.PYRAMID_SBIN, interval=interval)


def matlab_handle(model, **kw):
    h = capi.Handle(model, max_candidates=CAP, **kw)
    h.set_pyramid_kind(MATLAB)
    assert h.pyramid_kind == MATLAB
    return h


def composed(model, im, pad, pct=97.0, dtype=np.float32, correct_ptr=0):
    """the composed reference with the threshold at a percentile of its own root scores"""
    model.thresh = -1e30
    c = mp.compose(model, im, pad, dtype, correct_ptr, capacity=1)
    model.thresh = float(np.float32(np.percentile(np.concatenate([r.ravel() for r in c.rootv if r is not None]), pct)))
    return mp.compose(model, im, pad, dtype, correct_ptr, capacity=CAP)


def same(a, b, what=""):
    assert len(a[0]) == len(b[0]), (what, len(a[0]), len(b[0]))
    assert_candidates_equal(a, b, score_tol=0.0)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def prim():
    h = capi.Handle(small_model())
    yield h
    h.close()


# ---- 1. the two stand-alone entries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mp.resize_cases(), ids=lambda c: c[0])
def test_resize_area_equals_the_compiled_reference(gpu_required, prim, golden, case):
    name, im, scale = case
    got = prim.resize_area(im, scale)
    assert same_bits(got, golden[name]), name
    assert same_bits(got, mp.resize_def(im, scale)), name


def test_resize_area_one_channel_and_refusals(gpu_required, prim):
    im = mp.doubles(9, 31, 23, 1)[..., 0]
    assert same_bits(prim.resize_area(im, 0.6), mp.resize_def(im, 0.6))
    neg = -mp.doubles(10, 9, 7)                                  # the sum starts from +0.0: a -0.0 product never survives
    assert same_bits(prim.resize_area(neg, 0.5), mp.resize_def(neg, 0.5))
    with pytest.raises(capi.PbdError) as e:
        prim.resize_area(im, 1.0000001)
    assert e.value.code == capi.PBD_ERR_ARG and "Invalid scaling factor" in str(e.value)
    for bad in (0.0, -0.5, float("nan"), 1e-9):
        with pytest.raises(capi.PbdError) as e:
            prim.resize_area(im, bad)
        assert e.value.code == capi.PBD_ERR_ARG


def test_reduce_equals_the_compiled_reference(gpu_required, prim, golden):
    for name, im in mp.reduce_cases():
        got = prim.reduce(im)
        assert same_bits(got, golden[name]), name
        assert same_bits(got, mp.reduce_def(im)), name
    for w, h in ((64, 37), (33, 48)):                            # more than one block, one channel
        im = mp.doubles(w, w, h, 1)[..., 0]
        assert same_bits(prim.reduce(im), mp.reduce_def(im)), (w, h)
    for w, h in ((4, 9), (9, 4), (1, 1)):
        with pytest.raises(capi.PbdError) as e:
            prim.reduce(np.zeros((h, w, 3)))
        assert e.value.code == capi.PBD_ERR_ARG


# ---- 2. geometry, level images, features ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", mp.PYRAMID_INTERVALS)
def test_geometry_and_level_images(gpu_required, golden, interval):
    im = noise(*mp.PYRAMID_FRAME)
    g, lv = mp.pyramid_def(im, mp.PYRAMID_SBIN, interval)
    h = matlab_handle(small_model(interval))
    check_geometry(h.geometry(W, H), g, f"interval {interval}")
    h.pyramid(im)
    for l in range(g["nlevels"]):
        got = h.level_image_raw(l)
        assert got.dtype == np.float64
        assert same_bits(got, golden[f"pyr_i{interval}_l{l}"]), (interval, l)
        assert same_bits(got, lv[l]), (interval, l)
        fi, _ = h.frame_planes(0, l, W, H, imdtype=np.float64)
        assert same_bits(fi, lv[l])
    with pytest.raises(capi.PbdError) as e:
        h.level_image(0)                                         # the 8-bit getter
    assert e.value.code == capi.PBD_ERR_STATE
    # the default kind answers with the other geometry on the same handle, and back
    h.set_pyramid_kind(OPENCV)
    go = h.geometry(W, H)
    assert not np.array_equal(go["scales"], g["scales"]) or go["nlevels"] != g["nlevels"]
    h.set_pyramid_kind(MATLAB)
    check_geometry(h.geometry(W, H), g)
    h.close()


def test_one_channel_frame_stays_one_channel(gpu_required):
    im = noise(5, 75, 61, 1)
    g, lv = mp.pyramid_def(im, mp.PYRAMID_SBIN, 2)
    h = matlab_handle(small_model(), dtype=np.float64)
    h.pyramid(im)
    for l in range(g["nlevels"]):
        got = h.level_image_raw(l)
        assert got.shape == lv[l].shape and same_bits(got, lv[l]), l
        check_hog(h.level_features(l), lv[l], mp.PYRAMID_SBIN, f"grey level {l}")
    h.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_features_by_check_hog(gpu_required, dtype):
    """double handle: <= F64_TOL; float handle: within hog_ref.float_bound with nothing excused (tests/test_matlab_pyramid_cpu.py
    asserts that no level of this frame has a near-tie pixel)"""
    im = noise(*mp.PYRAMID_FRAME)
    g, lv = mp.pyramid_def(im, mp.PYRAMID_SBIN, 2)
    h = matlab_handle(small_model(), dtype=dtype)
    h.pyramid(im)
    for l in range(g["nlevels"]):
        got = h.level_features(l)
        assert got.dtype == np.dtype(dtype)
        check_hog(got, lv[l], mp.PYRAMID_SBIN, f"{np.dtype(dtype).name} level {l}")
    h.close()


# ---- 3. detections against the composed reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("pad", [0, 3])
def test_detect_equals_the_composed_reference(gpu_required, pad, dtype):
    model = small_model()
    im = make_image(4, W, H)
    ref = composed(model, im, pad, dtype=dtype)
    assert len(ref.heads) > 10
    h = matlab_handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype)
    if pad:
        h.set_boundary_pad(pad)
    h.pyramid(im)
    for l in range(ref.nlevels):
        np.testing.assert_array_equal(h.level_features(l), ref.feat[l])
    np.testing.assert_array_equal(h._geo["scales"], np.asarray(ref.scales, np.float32))
    h.pdf()
    nf = len(model.filtersw)
    for l in range(ref.nlevels):
        if ref.resp[l] is not None:
            for n in (0, nf - 1):
                np.testing.assert_array_equal(h.level_response(l, n), ref.resp[l][n])
    same(h.detect(im, CAP), (ref.heads, ref.boxes, ref.locs), (pad, dtype))
    h.close()


# ---- 4. every path gives the single-frame result -----------------------------------------------------------------------------------
def test_every_path_gives_the_single_frame_result(gpu_required):
    import torch
    model = small_model()
    frames = [make_image(30 + i, W, H) for i in range(2)]
    composed(model, frames[0], 0, pct=95.0)                      # (sets the threshold)
    h = matlab_handle(model)
    refs = [h.detect(f, CAP) for f in frames]
    assert all(len(r[0]) > 10 for r in refs)
    # enqueue / collect; the setter refuses while the frame is pending
    h.enqueue(frames[1])
    for kind in (OPENCV, MATLAB):
        with pytest.raises(capi.PbdError) as e:
            h.set_pyramid_kind(kind)
        assert e.value.code == capi.PBD_ERR_STATE and h.pyramid_kind == MATLAB
    same(h.collect(CAP), refs[1], "enqueue / collect")
    # host vs device-resident frame
    d = torch.from_numpy(frames[0]).cuda()
    same(h.detect_dev(d.data_ptr(), W, H, 3, capacity=CAP), refs[0], "device image")
    h.close()
    # eager vs graph replay (the second call captures, the third replays); a batch of two vs two single frames
    for graph in (0, 1):
        hg = matlab_handle(model, graph=graph)
        for k in range(4):
            same(hg.detect(frames[k % 2], CAP), refs[k % 2], ("single", graph, k))
        same(hg.detect_dev(d.data_ptr(), W, H, 3, capacity=CAP), refs[0], ("device image", graph))
        for k in range(3):
            got = hg.detect_batch(frames, CAP)
            for f in range(2):
                same(got[f], refs[f], ("batch", graph, k, f))
        hg.close()
    # compact plan
    hc = matlab_handle(model, dp_mode=2)
    for f in (0, 1, 0):
        same(hc.detect(frames[f], CAP), refs[f], ("compact", f))
    hc.close()


def test_rgbd_and_latent_entries(gpu_required, orc):
    model = small_model()
    im = make_image(4, W, H)
    ref = composed(model, im, 0, pct=95.0)
    h = matlab_handle(model, conv_mode=capi.PBD_CONV_EXACT)
    raw = h.detect(im, CAP)
    same(raw, (ref.heads, ref.boxes, ref.locs))
    # depth-consistency pruning of the MATLAB-kind records
    rng = np.random.default_rng(5)
    depth = (1.0 + 0.2 * rng.random((H, W))).astype(np.float32)
    depth[:, : W // 3] = 0
    h.set_depth_filter(True, 0.03)
    want = depth_ref.depth_filter(model, *raw, depth, 0.03)
    assert 0 < len(want[0]) <= len(raw[0])
    same(h.detect_rgbd(im, depth, CAP), want, "depth filter")
    h.set_depth_filter(False)
    # latent detection: the best pose overlapping the boxes of one of the records, on the restated pyramid's responses and scales
    i = int(np.argmax(raw[0]["score"]))
    truth = raw[1][i]
    want = LR.detect(orc, model, ref.scales, lambda l: ref.resp[l], truth, 0.5)
    got = h.detect_latent(im, truth, 0.5)
    assert want["found"] == 1 and len(got[0]) == 1
    assert (int(got[0]["level"][0]), int(got[0]["component"][0])) == (want["level"], want["component"])
    assert got[0]["score"][0] == np.float32(want["score"])
    np.testing.assert_array_equal(got[2][0][:len(want["locs"])], want["locs"])
    np.testing.assert_array_equal(got[1][0][:len(want["boxes"])], want["boxes"])
    h.close()


# ---- 5. the feature vector of a MATLAB-kind detection --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wx_reproduces_the_score(gpu_required, dtype):
    """tests/test_gpu_feature_vector.py's rule: w . x of the gathered feature vector is the record's score within the bounds of
    tests/part_scores_ref.py and tests/feature_vector_ref.py (EXACT bank, dt_correct_ptr = 1)"""
    model = small_model()
    im = make_image(4, W, H)
    composed(model, im, 3, pct=95.0, dtype=dtype, correct_ptr=1)
    h = matlab_handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, dt_correct_ptr=1)
    h.set_boundary_pad(3)                                        # the two together are featpyramid.m
    heads, _, locs = h.detect(im, CAP)
    n = len(heads)
    assert 10 < n < CAP
    blocks, windows = h.candidates_features(heads, locs)
    ps = h.candidates_part_scores(heads, locs)
    score = heads["score"].astype(np.float64)
    if np.dtype(dtype) == np.dtype(np.float64):                  # head.score is float: the root table holds the double
        h._geo = h.geometry(W, H)
        roots = {}
        for i in range(n):
            key = (int(heads["level"][i]), int(heads["component"][i]))
            if key not in roots:
                roots[key] = h.root(*key)[0]
            score[i] = roots[key][locs[i, 0, 1], locs[i, 0, 0]]
        np.testing.assert_array_equal(score.astype(np.float32), heads["score"])
    got, _ = wx(model.weight_vector(), dense_feature_vectors(model, blocks, windows))
    B = bound(ps, heads["nparts"], dtype) + window_bounds(model, blocks, windows, dtype)
    r = np.abs(got - score) / B
    print(f"{np.dtype(dtype).name}: {n} detections, worst |w.x - score| / bound = {r.max():.3f}")
    assert (r <= 1.0).all(), np.argwhere(r > 1.0)[:5]
    h.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_required):
    model = small_model()
    h = matlab_handle(model)
    for bad in (-1, 2, 7):
        with pytest.raises(capi.PbdError) as e:
            h.set_pyramid_kind(bad)
        assert e.value.code == capi.PBD_ERR_ARG and h.pyramid_kind == MATLAB
    im = make_image(4, W, H)
    for wide in (im.astype(np.uint16) * 257, im.astype(np.float32), im.astype(np.float64)):
        for call in (lambda: h.detect_image(wide, CAP), lambda: h.pyramid_image(wide)):
            with pytest.raises(capi.PbdError) as e:
                call()
            assert e.value.code == capi.PBD_ERR_UNSUPPORTED and "8-bit" in str(e.value), e.value
    with pytest.raises(capi.PbdError) as e:
        h.tune_plan(im)
    assert e.value.code == capi.PBD_ERR_UNSUPPORTED and "pbd_tune_plan" in str(e.value)
    with pytest.raises(capi.PbdError) as e:                      # 12000 x 8000 x 3 doubles: refused by the planner, nothing is allocated
        h.begin_frame(12000, 8000, 3)
    assert e.value.code == capi.PBD_ERR_UNSUPPORTED and "budget" in str(e.value)
    with pytest.raises(capi.PbdError) as e:                      # fewer levels than the interval
        h.begin_frame(24, 24, 3)
    assert e.value.code == capi.PBD_ERR_ARG
    assert len(h.detect_image(im, CAP)[0]) >= 0                  # an 8-bit image through pbd_detect_image is a plain frame
    h.set_pyramid_kind(OPENCV)
    assert len(h.detect_image(im.astype(np.uint16) * 257, CAP)[0]) >= 0     # and the default kind takes the other depths as before
    h.close()


# ---- 7. the default kind after a round trip ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
def test_default_kind_is_unchanged_after_a_round_trip(gpu_required, graph):
    model = small_model(interval=3, seed=11)
    frames = [make_image(40 + i, 120, 90) for i in range(2)]
    model.thresh = -1e30
    fresh = capi.Handle(model, max_candidates=CAP, graph=graph)
    fresh.pyramid(frames[0]); fresh.pdf(); fresh.dp_min()
    vals = np.concatenate([fresh.root(l, 0)[0].ravel() for l in range(fresh._geo["nlevels"])])
    fresh.close()
    model.thresh = float(np.float32(np.percentile(vals[np.isfinite(vals)], 95.0)))
    fresh = capi.Handle(model, max_candidates=CAP, graph=graph)
    assert fresh.pyramid_kind == OPENCV
    want = [[fresh.detect(f, CAP) for f in frames] for _ in range(2)][-1]
    want_batch = fresh.detect_batch(frames, CAP)
    fresh.pyramid(frames[0])
    want_img = [fresh.level_image(l) for l in range(fresh._geo["nlevels"])]
    fresh.close()
    assert all(len(r[0]) > 10 for r in want)
    h = capi.Handle(model, max_candidates=CAP, graph=graph)
    for _ in range(2):                                           # (graph handles: a captured default-kind graph exists before the switch)
        for f in (0, 1):
            same(h.detect(frames[f], CAP), want[f], "before")
    h.set_pyramid_kind(MATLAB)
    other = [h.detect(frames[f % 2], CAP) for f in range(3)]
    assert any(len(o[0]) != len(want[i % 2][0]) or not np.array_equal(o[0]["score"], want[i % 2][0]["score"]) for i, o in enumerate(other))
    h.set_pyramid_kind(OPENCV)
    for k in range(3):
        for f in (0, 1):
            same(h.detect(frames[f], CAP), want[f], ("after", k, f))
    got = h.detect_batch(frames, CAP)
    for f in (0, 1):
        same(got[f], want_batch[f], ("batch after", f))
    h.pyramid(frames[0])
    for l, a in enumerate(want_img):
        np.testing.assert_array_equal(h.level_image(l), a)
    h.close()
