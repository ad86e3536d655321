"""A live handle's weights and threshold replaced (k_weights.hip, pbd_weights.cpp; include/pbd_c.h "weight and threshold updates"),
against a FRESH handle created by pbd_create / pbd_create_sized from model.with_weight_vector(w): everything is compared in bits, there
are no tolerances.  Weights A are a builder's, weights B the same builder's under another seed poured into A's structure (so bias,
deformation and filter blocks all differ, anchors and ids do not); the threshold is taken from the root scores of both so that each
returns records, fewer than the capacity, and A's and B's records are asserted to differ."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_tree_model_k, make_voc_like_model

pytestmark = pytest.mark.gpu

W, H = 100, 80
CAP = 4096
F32, F64 = np.float32, np.float64
EXACT, MFMA, SPLIT, SPLIT16 = capi.PBD_CONV_EXACT, capi.PBD_CONV_MFMA, capi.PBD_CONV_SPLIT, capi.PBD_CONV_SPLIT_F16

BUILDERS = {
    # 33 filters: crosses a 32-filter n-tile (the second tile's padding, nfpad); sixteen mixtures: never a fold plan
    "tree33": lambda seed: make_tree_model_k([-1, 0, 0], [3, 16, 14], seed=seed),
    # 16 filters, at most 6 mixtures: a fold plan unless dp_mode 1 asks for the three-kernel structure
    "tree16": lambda seed: make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=seed),
    # a mixed bank: three sizes, so fperm is no identity and every size group is packed on its own
    "voc": lambda seed: make_voc_like_model(seed=seed, roots=((4, 3), (3, 5)), part_size=(2, 2), nparts=(3, 2)),
}


@functools.lru_cache(maxsize=None)
def frame(seed=0):
    return make_image(seed, W, H)


def root_scores(model):
    h = capi.Handle(model, conv_mode=EXACT, max_candidates=CAP)
    h.pyramid(frame()); h.pdf(); h.dp_min()
    g = h._geo
    v = np.concatenate([h.root(l, c)[0].ravel() for l in range(g["nlevels"]) if g["cell_w"][l] * g["cell_h"][l]
                        for c in range(model.ncomponents)])
    h.close()
    return np.sort(v)[::-1]


@functools.lru_cache(maxsize=None)
def setup(name):
    """(model A, model B, w_A, w_B) with one threshold under which both return between 1 and CAP - 1 records of frame()"""
    a = BUILDERS[name](5)
    wa, wb = a.weight_vector(), BUILDERS[name](6).weight_vector()
    assert wa.size == wb.size and (wa != wb).mean() > .9
    b = a.with_weight_vector(wb)
    ra, rb = root_scores(a), root_scores(b)
    t = float(np.float32(min(ra[40], rb[40])))        # at least 40 records of each ...
    assert max((ra > t).sum(), (rb > t).sum()) < CAP // 2   # ... and well under the capacity
    a, b = copy.copy(a), copy.copy(b)
    a.thresh = b.thresh = t
    return a, b, wa, wb


def same(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, i, g.shape, w.shape)


def differ(x, y):
    return len(x[0]) != len(y[0]) or x[0].tobytes() != y[0].tobytes() or x[2].tobytes() != y[2].tobytes()


def code_of(call):
    with pytest.raises(capi.PbdError) as e:
        call()
    return e.value.code


def response(h, filt):
    h._geo = h.geometry(W, H)
    return h.level_response(1, filt)


CASES = [
    ("tree33", F32, SPLIT, 1, 0), ("tree33", F32, SPLIT, 0, 1), ("tree33", F32, EXACT, 0, 0), ("tree33", F32, MFMA, 1, 1),
    ("tree33", F32, SPLIT16, 1, 0), ("tree33", F64, EXACT, 1, 0), ("tree33", F64, MFMA, 0, 1),
    ("tree16", F32, EXACT, 1, 1), ("tree16", F32, MFMA, 0, 0), ("tree16", F32, SPLIT, 0, 0), ("tree16", F32, SPLIT16, 0, 1),
    ("tree16", F64, EXACT, 0, 0), ("tree16", F64, MFMA, 1, 0),
    ("voc", F32, EXACT, 1, 0), ("voc", F32, MFMA, 0, 1), ("voc", F32, SPLIT, 0, 0), ("voc", F32, SPLIT16, 1, 0),
    ("voc", F64, EXACT, 0, 1), ("voc", F64, MFMA, 0, 0),
]


@pytest.mark.parametrize("name,dtype,conv,graph,dp_mode", CASES,
                         ids=[f"{n}-{np.dtype(d).name}-conv{c}-graph{g}-dp{m}" for n, d, c, g, m in CASES])
def test_equals_fresh_handle(gpu_required, name, dtype, conv, graph, dp_mode):
    a, b, wa, wb = setup(name)
    kw = dict(conv_mode=conv, max_candidates=CAP, dtype=dtype, graph=graph, dp_mode=dp_mode)
    im = frame()
    fresh = capi.Handle(b, **kw)
    want_b = fresh.detect(im, CAP)
    nf = len(b.filtersw)
    want_resp = response(fresh, nf - 1)
    fresh.close()
    h = capi.Handle(a, **kw)
    first = [h.detect(im, CAP) for _ in range(3)][-1]      # (a graph handle has captured and replayed)
    assert 0 < len(first[0]) < CAP and 0 < len(want_b[0]) < CAP and differ(first, want_b)
    mode = h.conv_mode
    h.set_weights(wb)
    same(h.detect(im, CAP), want_b, "B")
    assert response(h, nf - 1).tobytes() == want_resp.tobytes()
    assert h.weights().tobytes() == np.float32(wb).astype(np.float64).tobytes()
    assert h.model.weight_vector().tobytes() == h.weights().tobytes()
    for _ in range(2):                                      # the new weights captured and replayed too
        same(h.detect(im, CAP), want_b, "B again")
    h.set_weights(wa)
    same(h.detect(im, CAP), first, "back to A")
    assert h.L.pbd_get_conv_mode(h.h) == mode == conv
    h.close()


def test_device_vector_and_rounding(gpu_required):
    """pbd_set_weights_dev reads a device vector; values between two floats round to nearest even like astype(float32)"""
    import torch
    a, b, wa, wb = setup("tree16")
    rng = np.random.default_rng(3)
    w = wb * (1.0 + rng.uniform(-1e-9, 1e-9, wb.size))        # no longer float32-representable
    w[:4] = np.float32(wb[:4]).astype(np.float64) + np.spacing(np.float32(wb[:4])).astype(np.float64) / 2   # exact ties
    assert (np.float32(w).astype(np.float64) != w).mean() > .9
    fresh = capi.Handle(a.with_weight_vector(w), max_candidates=CAP)
    want = fresh.detect(frame(), CAP)
    fresh.close()
    h = capi.Handle(a, max_candidates=CAP)
    h.detect(frame(), CAP)
    h.set_weights(torch.from_numpy(w).to("cuda:0"))
    assert h.weights().tobytes() == np.float32(w).astype(np.float64).tobytes()
    same(h.detect(frame(), CAP), want)
    h.close()


def test_threshold(gpu_required):
    a, b, _, _ = setup("tree16")
    scores = root_scores(a)
    t2 = float(np.float32(scores[10]))
    a2 = copy.copy(a)
    a2.thresh = t2
    big = 1 << 16
    fresh = capi.Handle(a2, max_candidates=big, graph=1)
    want = fresh.detect(frame(), big)
    want_arg = fresh.dp_argmin(big)
    fresh.close()
    h = capi.Handle(a, max_candidates=big, graph=1)
    before = [h.detect(frame(), big) for _ in range(3)][-1]
    assert h.threshold == np.float32(a.thresh) and 0 < len(want[0]) < len(before[0])
    h.set_threshold(t2)
    assert h.threshold == np.float32(t2) and h.model.thresh == h.threshold
    same(h.dp_argmin(big), want_arg, "argmin of the resident min()")      # thresholded again, no new min()
    for _ in range(3):
        same(h.detect(frame(), big), want, "t2")
    am = copy.copy(a)
    am.thresh = -1.0
    fresh = capi.Handle(am, max_candidates=big, graph=1)
    want = fresh.detect(frame(), big)
    fresh.close()
    h.set_threshold(-1.0)
    got = h.detect(frame(), big)
    assert len(before[0]) < len(got[0]) < big
    same(got, want, "-1")
    h.set_threshold(-np.inf)
    assert h.threshold == -np.inf
    assert code_of(lambda: h.set_threshold(np.nan)) == capi.PBD_ERR_ARG and h.threshold == -np.inf
    h.set_threshold(a.thresh)
    same(h.detect(frame(), big), before, "back")
    h.close()


def test_part_scores(gpu_required):
    a, b, _, wb = setup("tree16")
    fresh = capi.Handle(b, max_candidates=CAP)
    fresh.set_part_scores(True)
    want = fresh.detect(frame(), CAP)
    want_ps = fresh.part_scores(0)
    fresh.close()
    h = capi.Handle(a, max_candidates=CAP)
    h.set_part_scores(True)
    h.detect(frame(), CAP)
    ps_a = h.part_scores(0)
    h.set_weights(wb)
    same(h.detect(frame(), CAP), want)
    got = h.part_scores(0)
    assert got.shape == want_ps.shape and got.tobytes() == want_ps.tobytes() and got.any()
    assert ps_a.shape != got.shape or ps_a.tobytes() != got.tobytes()
    h.close()


def test_latent_detection(gpu_required):
    a, b, _, wb = setup("tree16")
    fresh = capi.Handle(b, max_candidates=CAP)
    heads, boxes, _ = fresh.detect(frame(), CAP)
    truth = boxes[int(np.argmax(heads["score"]))]
    want = fresh.detect_latent(frame(), truth, 0.5)
    fresh.close()
    assert len(want[0]) == 1
    h = capi.Handle(a, max_candidates=CAP)
    old = h.detect_latent(frame(), truth, 0.5)
    h.set_weights(wb)
    same(h.detect_latent(frame(), truth, 0.5), want)
    assert differ(old, want)
    h.close()


def test_closed_loop(gpu_required):
    """one round of train.m on a live handle: positives and negatives into the cache, solve, vec2model into the handle, mine with it"""
    a, _, wa, _ = setup("tree16")
    big, cpos, cneg, cap = 1 << 15, 0.5, 0.25, 64
    _, _, _, noneg = a.qp_vectors()
    h = capi.Handle(a, max_candidates=big)
    q = capi.QpCache(h, cap, cpos, cneg)
    boxes = np.array([[10, 8, 40, 38], [50, 20, 85, 60], [20, 30, 70, 75]], np.float64)
    npos = q.write_warped(frame(), boxes, 0, 0)[0]
    heads, _, locs = h.detect(frame(), big)
    nneg = q.write(heads[:8], locs[:8], -1, 0)
    assert npos == 3 and nneg == 8
    q.noneg(noneg); q.fix(npos); q.opt(.05, 25, 1)
    q.apply_weights()
    wq = q.weights()
    assert (np.float32(wq) != np.float32(wa)).mean() > .5
    assert h.weights().tobytes() == np.float32(wq).astype(np.float64).tobytes()
    trained = a.with_weight_vector(wq)
    assert trained.weight_vector().tobytes() == h.model.weight_vector().tobytes()
    fresh = capi.Handle(trained, max_candidates=big)
    same(h.detect(frame(), big), fresh.detect(frame(), big), "after apply_weights")
    # mine a second frame at -1 with the new model, on both
    qf = capi.QpCache(fresh, cap, cpos, cneg)
    out = []
    for hh, qq in ((h, q), (fresh, qf)):
        hh.set_threshold(-1.0)
        rec = hh.detect(frame(1), big)
        assert 8 <= len(rec[0]) < big
        n0 = qq.dims()[3]
        assert qq.write(rec[0][:8], rec[2][:8], -1, 1) == 8
        out.append((rec, qq.get(n0, 8)))
    same(out[0][0], out[1][0], "mined records")
    same(out[0][1], out[1][1], "mined columns")
    assert out[0][1][0].any()
    q.opt(.05, 25, 2)
    q.apply_weights()
    assert h.weights().tobytes() == np.float32(q.weights()).astype(np.float64).tobytes()
    qf.close(); fresh.close(); q.close(); h.close()


# ---- refusals: the code, and the handle untouched ----
def bad_nan(w, lay): w[lay["filters"][1] + 7] = np.nan
def bad_inf(w, lay): w[2] = np.inf
def bad_overflow(w, lay): w[lay["filters"][0]] = 1e39          # inf as a float32
def bad_def_zero(w, lay): w[lay["deform"] + 4 + 2] = 0.0
def bad_def_underflow(w, lay): w[lay["deform"]] = 1e-60       # 0 as a float32


REFUSALS = [("nan", bad_nan, EXACT, capi.PBD_ERR_ARG), ("inf", bad_inf, EXACT, capi.PBD_ERR_ARG),
            ("1e39", bad_overflow, SPLIT, capi.PBD_ERR_ARG), ("len+1", lambda w, lay: None, EXACT, capi.PBD_ERR_ARG),
            ("len-1", lambda w, lay: None, MFMA, capi.PBD_ERR_ARG), ("def-zero", bad_def_zero, EXACT, capi.PBD_ERR_ARG),
            ("def-underflow", bad_def_underflow, SPLIT16, capi.PBD_ERR_ARG),
            ("split-range", lambda w, lay: w.__setitem__(lay["filters"][3] + 1, -3.2e38), SPLIT, capi.PBD_ERR_UNSUPPORTED),
            ("split16-range", lambda w, lay: w.__setitem__(lay["filters"][3] + 1, 3.2e38), SPLIT16, capi.PBD_ERR_UNSUPPORTED)]


@pytest.mark.parametrize("what,spoil,conv,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_leaves_the_handle_untouched(gpu_required, what, spoil, conv, code):
    a, _, wa, wb = setup("tree16")
    h = capi.Handle(a, conv_mode=conv, max_candidates=CAP, graph=1)
    h.set_part_scores(True)                                   # (so that k_partscore's table exists and could be touched)
    before = [h.detect(frame(), CAP) for _ in range(3)][-1]
    w = wb.copy()
    spoil(w, a.feature_layout())
    if what == "len+1":
        w = np.append(w, 0.0)
    if what == "len-1":
        w = w[:-1]
    assert code_of(lambda: h.set_weights(w)) == code
    assert h.L.pbd_last_error(h.h)
    assert h.weights().tobytes() == np.float32(wa).astype(np.float64).tobytes()
    same(h.detect(frame(), CAP), before, what)
    h.close()


def test_split_range_is_the_split_banks_alone(gpu_required):
    """|w| = 3.2e38 is a float32 like any other on an MFMA handle (no frame runs on it: its responses would leave the DT's finite domain)"""
    a, _, wa, wb = setup("tree16")
    h = capi.Handle(a, conv_mode=MFMA, max_candidates=CAP)
    w = wb.copy()
    w[a.feature_layout()["filters"][3] + 1] = 3.2e38
    h.set_weights(w)
    assert h.weights().tobytes() == np.float32(w).astype(np.float64).tobytes()
    h.set_weights(wa)
    h.close()


def test_null_and_nan_arguments(gpu_required):
    a, _, wa, _ = setup("tree16")
    h = capi.Handle(a, max_candidates=CAP)
    L = h.L
    out = np.zeros(wa.size)
    assert L.pbd_set_weights(h.h, None, wa.size) == capi.PBD_ERR_ARG
    assert L.pbd_set_weights_dev(h.h, None, wa.size) == capi.PBD_ERR_ARG
    assert L.pbd_get_weights(h.h, None, wa.size) == capi.PBD_ERR_ARG
    assert L.pbd_get_weights(h.h, out.ctypes.data_as(C.c_void_p), wa.size - 1) == capi.PBD_ERR_ARG
    assert L.pbd_get_threshold(h.h, None) == capi.PBD_ERR_ARG
    assert h.weights().tobytes() == wa.tobytes()
    q = capi.QpCache(h, 4)
    q.apply_weights()                                         # a solver state of zeros: w = w0
    assert h.weights().tobytes() == np.float32(a.qp_vectors()[2]).astype(np.float64).tobytes()
    q.close(); h.close()


def test_frame_in_flight(gpu_required):
    a, _, wa, wb = setup("tree16")
    h = capi.Handle(a, max_candidates=CAP)
    before = h.detect(frame(), CAP)
    im = np.ascontiguousarray(frame())
    h.enqueue(im)
    assert code_of(lambda: h.set_weights(wb)) == capi.PBD_ERR_STATE
    assert code_of(lambda: h.set_threshold(0.5)) == capi.PBD_ERR_STATE
    same(h.collect(CAP), before, "the frame in flight is the old model's")
    assert h.weights().tobytes() == np.float32(wa).astype(np.float64).tobytes() and h.threshold == np.float32(a.thresh)
    h.set_weights(wb)                                         # collected: accepted
    assert differ(h.detect(frame(), CAP), before)
    h.close()


def test_group_member(gpu_required):
    a, _, wa, wb = setup("tree16")
    g = capi.Group(a, [0], gather=capi.PBD_GATHER_HOST, max_candidates=CAP)
    before = g.detect(frame(), CAP)
    member = C.c_void_p(g.L.pbd_group_member(g.g, 0))
    out = np.zeros(wa.size)
    assert g.L.pbd_set_weights(member, wb.ctypes.data_as(C.c_void_p), wb.size) == capi.PBD_ERR_UNSUPPORTED
    assert g.L.pbd_set_threshold(member, C.c_float(0.25)) == capi.PBD_ERR_UNSUPPORTED
    assert g.L.pbd_get_weights(member, out.ctypes.data_as(C.c_void_p), out.size) == capi.PBD_OK
    assert out.tobytes() == np.float32(wa).astype(np.float64).tobytes()
    same(g.detect(frame(), CAP), before)
    g.close()
