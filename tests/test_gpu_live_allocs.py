"""A call gives back what it took: pbd_debug_live_allocs (capi.live_allocs) counts every device and pinned host buffer the library
holds in this process, so "afterwards equals before" is exact — buffers and bytes, no tolerance, whatever else uses the GPU.

1. the refused pbd_dt2d (a map too large for LDS is refused behind the call's allocations) leaves nothing behind;
2. every stand-alone call's temporaries are gone when it returns.  Each call runs twice: the first may allocate buffers that belong to
   the handle from then on (pbd_get_footprint counts them, check 3 sees them go with the handle), the second must move nothing;
3. objects give back everything when they are closed;
4. pbd_get_footprint's model bytes are what they were before the allocations moved into one owner type (MODEL_BYTES: literals from a
   run of the commit before), and the counter's bytes across a create are those plus the two pinned candidate buffers."""
import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_mixed_person_model, make_tree_model
from tests import dt_path_cases as dc
from tests.util import thresh_from_oracle

pytestmark = pytest.mark.gpu

TREE5 = [-1, 0, 1, 1, 0]
W, H = 160, 120
CAM = (525.0, 523.5, 319.5, 239.5, 0.0, 0.0)

KINDS = {   # the handles of checks 3 and 4
    "f32": lambda: capi.Handle(make_tree_model([-1, 0], 1, seed=1), conv_mode=capi.PBD_CONV_EXACT),
    "f64": lambda: capi.Handle(make_tree_model([-1, 0], 1, seed=1), conv_mode=capi.PBD_CONV_EXACT, dtype=np.float64),
    "sized": lambda: capi.Handle(make_mixed_person_model(seed=5, K=2), sized=True),
    "split": lambda: capi.Handle(make_tree_model(TREE5, 3, seed=5), conv_mode=capi.PBD_CONV_SPLIT),
}
# Handle.footprint()[1] of KINDS right after create, on an MI355X, from the commit before this file existed
MODEL_BYTES = {"f32": 2157877, "f64": 3694005, "sized": 11167681, "split": 2655921}


def _recorded(dtype):
    return next(c for c in dc.RECORDED_CASES if np.dtype(c["dtype"]) == np.dtype(dtype))


# ---- 1. the refused dt2d --------------------------------------------------------------------------------------------------------
def test_refused_dt2d_leaves_nothing_behind(gpu_required):
    h = KINDS["f32"]()
    case, fix = _recorded(np.float32), np.load(dc.REF_DT_FIXTURE)
    wide = np.zeros((1, 8192), np.float32)   # a line of 8192 scores: 4 lines x 8192 x 10 bytes of LDS, over the 160 KB a block can have
    before = capi.live_allocs()
    for _ in range(4):
        with pytest.raises(capi.PbdError) as e:
            h.dt2d(wide, -1.0, 0.0, -1.0, 0.0, 1, 1)
        assert "too large" in str(e.value), e.value
    assert capi.live_allocs() == before
    dc.assert_same(h.dt2d(case["make"](), *case["q"]), dc.recorded(fix, case["name"]), case["name"] + " after the refusals")
    assert capi.live_allocs() == before
    h.close()


# ---- 2. call temporaries --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def live(gpu_required, orc):
    """a float and a double handle of one 5-part model, a frame resident on each, and the frame's records"""
    model = make_tree_model(TREE5, 3, seed=5)
    im = make_image(0, W, H)
    model.thresh = thresh_from_oracle(orc, model, im, q=99.0)
    hs = {np.dtype(dt): capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dt) for dt in (np.float32, np.float64)}
    recs = hs[np.dtype(np.float32)].detect(im)
    hs[np.dtype(np.float64)].detect(im)
    assert 4 <= len(recs[0]) <= 2000
    yield hs, model, im, recs
    for h in hs.values():
        h.close()


def _twice_second_moves_nothing(what, fn):
    fn()
    before = capi.live_allocs()
    out = fn()
    assert capi.live_allocs() == before, (what, before, capi.live_allocs())
    return out


def test_image_primitives_give_back_what_they_took(live):
    hs, _, im, _ = live
    h, h64 = hs[np.dtype(np.float32)], hs[np.dtype(np.float64)]
    imd = im.astype(np.float64)
    score = np.random.default_rng(2).normal(0, 1, (37, 53)).astype(np.float32)
    c32, c64 = _recorded(np.float32), _recorded(np.float64)
    calls = {
        "dt2d": lambda: h.dt2d(c32["make"](), *c32["q"]),
        "dt2d_f64": lambda: h64.dt2d(c64["make"](), *c64["q"]),
        "hog": lambda: h.hog(im),
        "hog_f64": lambda: h64.hog(im),
        "resize": lambda: h.resize(im, 101, 75),
        "pyrdown": lambda: h.pyrdown(im),
        "resize_area": lambda: h.resize_area(imd, 0.7),
        "reduce": lambda: h.reduce(imd),
        "nms_map": lambda: h.nms_map(score, 2),
    }
    for what, fn in calls.items():
        _twice_second_moves_nothing(what, fn)


def test_candidate_primitives_give_back_what_they_took(live):
    hs, _, im, (heads, boxes, locs) = live
    h = hs[np.dtype(np.float32)]
    rng = np.random.default_rng(4)
    depth = (2.0 + 0.002 * np.arange(W)[None, :] + rng.normal(0, 0.01, (H, W))).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    cloud = np.stack([(xx - W / 2) * depth / 525.0, (yy - H / 2) * depth / 525.0, depth], axis=2).astype(np.float32)
    _twice_second_moves_nothing("candidates_filter", lambda: h.candidates_filter(heads, boxes, locs, W, H, capi.PBD_CAND_SORT_NMS, 0.3))
    _twice_second_moves_nothing("candidates_filter_parts", lambda: h.candidates_filter_parts(heads, boxes, locs))
    _twice_second_moves_nothing("candidates_depth_filter", lambda: h.candidates_depth_filter(heads, boxes, locs, depth))
    b3, _ = _twice_second_moves_nothing("candidates_box3d", lambda: h.candidates_box3d(heads, boxes, depth, W, H, CAM))
    _twice_second_moves_nothing("candidates_cluster3d", lambda: h.candidates_cluster3d(cloud, b3))
    _twice_second_moves_nothing("candidates_part_scores", lambda: h.candidates_part_scores(heads, locs))
    _twice_second_moves_nothing("candidates_features", lambda: h.candidates_features(heads, locs))


def test_training_calls_give_back_what_they_took(live):
    hs, _, im, (heads, boxes, _) = live
    h = hs[np.dtype(np.float32)]
    w = h.weights()
    _twice_second_moves_nothing("set_weights", lambda: h.set_weights(w))   # (the first call drops the frame plan, the second has none to drop)
    h.detect(im)
    q = capi.QpCache(h, 16)
    box = np.array([[20.0, 15.0, 90.0, 100.0]])
    assert _twice_second_moves_nothing("write_warped", lambda: q.write_warped(im, box, 0, 0))[0] == 1
    length, _, _, n = q.dims()
    assert n == 2
    _twice_second_moves_nothing("score", lambda: q.score(np.ones(length)))
    _twice_second_moves_nothing("lincomb", lambda: q.lincomb(np.ones(n)))
    P = h.max_parts
    ev = capi.Eval(h, P, 64, 4096)
    ngt = 3
    pts = np.random.default_rng(6).uniform(0, W, (ngt, P, 2))
    sc = np.full(ngt, 10.0)
    _twice_second_moves_nothing("add_pck_records", lambda: ev.add_pck_records(heads[:ngt], boxes[:ngt], np.ones(ngt, np.int32), pts, sc))
    _twice_second_moves_nothing("add_apk_records", lambda: ev.add_apk_records(heads, boxes, pts, sc))
    _twice_second_moves_nothing("pck", ev.pck)
    _twice_second_moves_nothing("apk", ev.apk)
    _twice_second_moves_nothing("apk curves", lambda: ev.apk(curves=True))
    before = capi.live_allocs()
    ev.close(); q.close()
    after = capi.live_allocs()
    assert after[0] < before[0] and after[1] < before[1]


def test_handle_less_calls_give_back_what_they_took(gpu_required):
    rng = np.random.default_rng(9)
    d = rng.normal(0, 5, (5, 130, 2))
    _twice_second_moves_nothing("cluster_parts", lambda: capi.cluster_parts(d, TREE5, [3, 6, 2, 4, 6], R=7, seed=1, max_iter=1000))
    small = make_image(5, 32, 24)
    before = capi.live_allocs()
    outs = capi.augment(small, [(False, 15.0, 1), (True, None, 0)])   # (no handle: the very first call keeps nothing either)
    assert len(outs) == 2 and capi.live_allocs() == before


# ---- 3. object lifetimes --------------------------------------------------------------------------------------------------------
def test_objects_give_back_everything_when_closed(gpu_required):
    base = capi.live_allocs()
    im = make_image(3, 64, 48)
    handles = [mk() for mk in KINDS.values()]
    for h in handles:
        h.detect(im)
    h = handles[0]
    q = capi.QpCache(h, 8)
    assert q.write_warped(im, np.array([[5.0, 5.0, 40.0, 40.0], [10.0, 8.0, 50.0, 44.0]]), 0, 0)[0] == 2
    q.solve_pass(np.arange(2, dtype=np.int32))
    ev = capi.Eval(h, h.max_parts, 8, 64)
    store = capi.PyramidStore(h, 1, 64, 48)
    store.put(0, im)
    grp = capi.Group(make_tree_model([-1, 0], 1, seed=1), [0])
    held = capi.live_allocs()
    assert held[0] > base[0] and held[1] > base[1]
    for obj in (grp, store, ev, q, *reversed(handles)):
        obj.close()
    assert capi.live_allocs() == base


# ---- 4. footprint ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_model_footprint_is_the_parent_commits(gpu_required, kind):
    before = capi.live_allocs()
    h = KINDS[kind]()
    created = capi.live_allocs()
    pinned = (capi.HEAD_DTYPE.itemsize + 28 * h.max_parts) * 4096 + 16   # cand_stride x max_candidates records, and the 16-byte count block
    assert h.footprint() == (0, MODEL_BYTES[kind])
    assert created[1] - before[1] == MODEL_BYTES[kind] + pinned
    h.detect(make_image(3, 64, 48))
    assert h.footprint()[1] == MODEL_BYTES[kind]   # a plain frame allocates for the plan only
    h.close()
    assert capi.live_allocs() == before
