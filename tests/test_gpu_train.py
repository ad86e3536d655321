"""One training round on the device (include/pbd_c.h "one training round"; k_qp_thresh.hip, pbd_qp_solve.cpp, pbd_api.cpp;
partsbaseddetector_amd/train.py; host/pbd_host.hpp train): pbd_set_interval against handles created at that interval, in bits;
pbd_qp_positive_threshold against the host route it replaces, in bits; pbd_qp_clear against a new cache; train() against its sequence
of primitives written out by hand on twin handles and caches; the C++ demo; the returned model; train_model() end to end."""
import copy
import math
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import PartsBasedDetector, capi
from partsbaseddetector_amd.detector import shuffled_support
from partsbaseddetector_amd.model import (Model, build_model, data_def, init_model, make_image, make_mixed_person_model, make_tree_model_k,
                                          merge_models)
from partsbaseddetector_amd.train import point_to_box, train, train_model

pytestmark = pytest.mark.gpu

SW, SH = 100, 80
CAP = 64
MAXC = 4096
C_, WPOS = 0.002, 2
BLOCK = capi.QP_THRESH_BLOCK


def with_interval(model, iv):
    m = copy.copy(model)
    m._keep = []
    m.interval = iv
    return m


def make_model(kind):
    if kind == "person":
        return make_mixed_person_model(seed=5, K=2)
    return make_tree_model_k([-1, 0, 1, 1], [1, 3, 2, 2], seed=21)


def handle(model, dtype=np.float32, pyr=None, **kw):
    h = capi.Handle(model, dtype=dtype, max_candidates=MAXC, **kw)
    if pyr is not None:
        h.set_pyramid_kind(pyr)
    return h


def root_percentile(h, im, pct):
    h.pyramid(im); h.pdf(); h.dp_min()
    v = np.concatenate([h.root(l, c)[0].ravel() for l in range(h._geo["nlevels"]) for c in range(h.model.ncomponents)])
    return float(np.float32(np.percentile(v[np.isfinite(v)], pct)))


def same(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def snapshot(q):
    """everything of a cache a call could change, as bytes: every column of the capacity, dims, the solver's a, sv, w and stats"""
    cap = q.dims()[2]
    a, sv, w, st = q.state()
    return [v.tobytes() for v in q.get(0, cap)] + [repr(q.dims()), a.tobytes(), sv.tobytes(), w.tobytes(), st.tobytes()]


def same_caches(q, t, what=""):
    for i, (g, e) in enumerate(zip(snapshot(q), snapshot(t))):
        assert g == e, (what, ("x", "ids", "b", "d", "dims", "a", "sv", "w", "stats")[i])


# ---- 1. pbd_set_interval -----------------------------------------------------------------------------------------------------------------
def compare_with_fresh(h, model, iv, dtype, pyr, ims, truth, thr, what):
    """h, now at interval iv, against a handle created at it: geometry, a detect, a batch of two and a latent detect, in bits"""
    f = handle(with_interval(model, iv), dtype, pyr, graph=1)
    f.set_threshold(thr)
    assert h.interval == iv == h.model.interval
    ga, gb = h.geometry(SW, SH), f.geometry(SW, SH)
    assert ga["nlevels"] == gb["nlevels"] and all(ga[k].tobytes() == gb[k].tobytes() for k in ("img_w", "img_h", "cell_w", "cell_h", "scales")), what
    a, b = h.detect(ims[0], capacity=MAXC), f.detect(ims[0], capacity=MAXC)
    assert same(a, b) and len(a[0]) > 0, (what, "detect", len(a[0]), len(b[0]))
    for x, y in zip(h.detect_batch(ims, capacity=MAXC), f.detect_batch(ims, capacity=MAXC)):
        assert same(x, y), (what, "batch")
    la, lb = h.detect_latent(ims[0], truth, 0.5), f.detect_latent(ims[0], truth, 0.5)
    assert same(la, lb), (what, "latent")
    a2 = h.detect(ims[0], capacity=MAXC)                 # once more: the replayed graph of the new plan
    assert same(a2, b), (what, "second detect")
    f.close()
    return len(a[0]), len(la[0])


GRID = [(k, d, p) for k in ("tree_k", "person") for d in (np.float32, np.float64) for p in (None, capi.PBD_PYRAMID_MATLAB)]


@pytest.mark.parametrize("kind, dtype, pyr", GRID, ids=[f"{k}-{np.dtype(d).name}-{'matlab' if p else 'opencv'}" for k, d, p in GRID])
def test_set_interval_equals_a_fresh_handle(gpu_required, kind, dtype, pyr):
    model = make_model(kind)
    ims = [make_image(3, SW, SH), make_image(4, SW, SH)]
    h = handle(model, dtype, pyr, graph=1)
    thr = root_percentile(h, ims[0], 95.0)
    h.set_threshold(thr)
    first = h.detect(ims[0], capacity=MAXC)
    assert same(first, h.detect(ims[0], capacity=MAXC)) and len(first[0]) > 0      # twice: a graph exists
    i = int(np.argmax(first[0]["score"]))
    truth = np.zeros((model.max_parts, 4), np.int32)
    truth[:int(first[0]["nparts"][i])] = first[1][i][:int(first[0]["nparts"][i])]
    found = 0
    for iv in (2, 1, model.interval):
        h.set_interval(iv)
        assert not any(h.stage_state().values())          # the plan is dropped, as after pbd_set_weights
        found += compare_with_fresh(h, model, iv, dtype, pyr, ims, truth, thr, (kind, iv))[1]
    assert found >= 1                                     # (at the model's own interval the pose the truth came from is there)
    assert same(h.detect(ims[0], capacity=MAXC), first)
    h.close()


def test_set_interval_frame_too_small_for_the_new_interval(gpu_required):
    model = make_model("tree_k")
    two, ten = handle(with_interval(model, 2)), handle(model)
    side = None
    for s in range(8, 80):                                # the smallest square frame the interval-2 handle plans and the interval-10 one refuses
        try:
            two.geometry(s, s)
        except capi.PbdError:
            continue
        try:
            ten.geometry(s, s)
        except capi.PbdError:
            side = s
            break
    assert side is not None
    im = make_image(3, side, side)
    two.set_threshold(1e9); ten.set_threshold(1e9)
    assert len(two.detect(im)[0]) == 0
    with pytest.raises(capi.PbdError) as want:
        ten.detect(im)
    two.set_interval(10)
    with pytest.raises(capi.PbdError) as got:
        two.detect(im)
    assert got.value.code == want.value.code == capi.PBD_ERR_ARG and str(got.value) == str(want.value) and "interval" in str(got.value)
    two.set_interval(2)                                   # and back: the handle plans the frame again
    assert len(two.detect(im)[0]) == 0
    two.close(); ten.close()


def test_mining_after_set_interval_equals_a_twin_created_at_it(gpu_required):
    model = make_model("tree_k")
    im = make_image(3, SW, SH)
    h, g = handle(model), handle(with_interval(model, 2))
    q, t = capi.QpCache(h, CAP, C_ * WPOS, C_), capi.QpCache(g, CAP, C_ * WPOS, C_)
    thr = root_percentile(g, im, 97.0)
    h.set_threshold(thr); g.set_threshold(thr)
    assert h.detect(im, capacity=MAXC)[0].size > 0        # a plan (and resident planes) of interval 10 exists when the interval moves
    h.set_interval(2)
    got, want = q.mine(im, 7), t.mine(im, 7)
    assert got == want and 3 < got[1] <= CAP, (got, want)
    same_caches(q, t, "mined at interval 2")
    assert q.get()[1][:, 2].max() < g.geometry(SW, SH)["nlevels"] < ten_levels(model)
    h.set_interval(10)                                    # the cache stays valid across the change: its columns are features
    assert q.score(np.ones(q.dims()[0])).tobytes() == t.score(np.ones(t.dims()[0])).tobytes()
    h.close(); g.close()


def ten_levels(model):
    h = handle(model)
    n = h.geometry(SW, SH)["nlevels"]
    h.close()
    return n


def test_set_interval_refusals_change_nothing(gpu_required):
    model = make_model("tree_k")
    im = make_image(3, SW, SH)
    h = handle(model, graph=1)
    h.set_threshold(root_percentile(h, im, 99.0))
    want = h.detect(im, capacity=MAXC)
    assert same(want, h.detect(im, capacity=MAXC))
    for bad in (0, -1, 17, 1 << 20):
        with pytest.raises(capi.PbdError) as e:
            h.set_interval(bad)
        assert e.value.code == capi.PBD_ERR_ARG and h.interval == 10 == h.model.interval
        assert same(h.detect(im, capacity=MAXC), want)
    h.enqueue(im)
    with pytest.raises(capi.PbdError) as e:
        h.set_interval(2)
    assert e.value.code == capi.PBD_ERR_STATE and h.interval == 10
    assert same(h.collect(capacity=MAXC), want) and same(h.detect(im, capacity=MAXC), want)
    assert h.L.pbd_set_interval(None, 2) == capi.PBD_ERR_ARG
    st = h.stage_state()
    h.set_interval(10)                                    # the interval it has: accepted, nothing dropped
    assert h.stage_state() == st and any(st.values())
    grp = capi.Group(model, [0])
    member = capi.C.c_void_p(grp.L.pbd_group_member(grp.g, 0))
    before = grp.detect(im)
    assert grp.L.pbd_set_interval(member, 2) == capi.PBD_ERR_UNSUPPORTED and grp.L.pbd_get_interval(member) == 10
    assert same(grp.detect(im), before)
    grp.close(); h.close()


# ---- 2. pbd_qp_positive_threshold --------------------------------------------------------------------------------------------------------
SMALL = dict(parents=[-1, 0], Ks=[1, 2], seed=3)


def small_handle():
    return handle(make_tree_model_k(SMALL["parents"], SMALL["Ks"], seed=SMALL["seed"]))


def columns(q, model, n, rng, labels, dup_of=None):
    """n two-block columns for pbd_qp_put: the root bias, then 40 values from the first deformation on (across the deformations, whose
    w0 is not zero, into the first filter); labels[i] the first id word; dup_of[i] >= 0: a copy of that column"""
    length, k, _, _ = q.dims()
    lay = model.feature_layout()
    x = np.zeros((n, k), np.float32)
    for i in range(n):
        vals = rng.standard_normal(40).astype(np.float32)
        x[i, :6 + 40] = np.concatenate([[2, 1, 1, rng.standard_normal(), lay["deform"] + 1, lay["deform"] + 40], vals]).astype(np.float32)
        if dup_of is not None and dup_of[i] >= 0:
            x[i] = x[dup_of[i]]
    ids = np.stack([np.asarray(labels, np.int32), np.arange(n, dtype=np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32),
                    np.zeros(n, np.int32)], axis=1)
    return x, ids, rng.standard_normal(n).astype(np.float32), (x[:, 6:].astype(np.float64) ** 2).sum(axis=1)


def loaded_cache(h, n, labels, seed=0, dup_of=None, capacity=None):
    rng = np.random.default_rng(seed)
    size = h.model.feature_layout()["size"]
    wreg, w0 = 0.5 + rng.random(size), 0.1 * rng.standard_normal(size)
    q = capi.QpCache(h, capacity or max(n, 1), 0.004, 0.002, wreg, w0)
    if n:
        q.put(*columns(q, h.model, n, rng, labels, dup_of))
        a = rng.random(n) * (rng.random(n) < 0.7)
        a[0] = 0.5
        q.set_state(a=a, sv=np.ones(n, np.uint8))
        q.refresh()
    return q, wreg, w0


def host_route(q, wreg, w0, frac):
    """what the entry replaces: the ids home, w + w0 .* wreg on the host, pbd_qp_score, / cpos, the sort"""
    I = np.flatnonzero(q.get()[1][:, 0] == 1).astype(np.int32)
    w = q.state()[2]
    return Model.positive_threshold(q.score(w + w0 * wreg, I) / 0.004, frac), len(I)


MS = [1, 2, 20, 21, 64, 2 * BLOCK + 3]
FRACS = [.05, .5, 1, 1e-9]


@pytest.mark.parametrize("m", MS)
def test_positive_threshold_equals_the_host_route(gpu_required, m):
    h = small_handle()
    n = 2 * m                                             # labels interleaved +1 / -1
    q, wreg, w0 = loaded_cache(h, n, [1 if i % 2 == 0 else -1 for i in range(n)], seed=m)
    assert np.abs(q.state()[2]).max() > 0
    before = snapshot(q)
    for frac in FRACS:
        want, mm = host_route(q, wreg, w0, frac)
        got = q.positive_threshold(frac)
        assert mm == m and got[1] == m
        assert np.float64(got[0]).tobytes() == np.float64(want).tobytes(), (m, frac, got[0], want)
    sc = np.sort(q.score(q.state()[2] + w0 * wreg, np.arange(0, n, 2, dtype=np.int32)) / 0.004)
    assert q.positive_threshold(1)[0] == sc[-1] and q.positive_threshold(1e-9)[0] == sc[0]
    assert m < 3 or sc[0] < sc[-1]
    assert snapshot(q) == before
    h.close()


def test_positive_threshold_ties_and_last_index(gpu_required):
    h = small_handle()
    # every positive but two a copy of column 0: the selected rank falls among exact ties for every q but the extremes
    n = 42
    labels = [1 if i % 2 == 0 else -1 for i in range(n)]
    dup = [0 if (i % 2 == 0 and 0 < i < n - 4) else -1 for i in range(n)]
    q, wreg, w0 = loaded_cache(h, n, labels, seed=5, dup_of=dup)
    sc = q.score(q.state()[2] + w0 * wreg, np.arange(0, n, 2, dtype=np.int32)) / 0.004
    assert (sc == sc[0]).sum() == 19
    for frac in FRACS + [.3, .7, .95]:
        want, m = host_route(q, wreg, w0, frac)
        got = q.positive_threshold(frac)
        assert got[1] == m == 21 and np.float64(got[0]).tobytes() == np.float64(want).tobytes(), frac
    assert q.positive_threshold(.5)[0] == sc[0]
    # one positive, at the last index, behind more negatives than one workgroup ranks
    n = BLOCK + 7
    t, wreg, w0 = loaded_cache(h, n, [-1] * (n - 1) + [1], seed=6)
    before = snapshot(t)
    for frac in FRACS:
        want, m = host_route(t, wreg, w0, frac)
        got = t.positive_threshold(frac)
        assert got[1] == m == 1 and np.float64(got[0]).tobytes() == np.float64(want).tobytes()
    assert snapshot(t) == before
    h.close()


def test_positive_threshold_after_keep(gpu_required):
    """pbd_qp_keep permutes the example -> column map: the selection follows the examples, not the columns"""
    h = small_handle()
    n = 42
    q, wreg, w0 = loaded_cache(h, n, [1 if i % 2 == 0 else -1 for i in range(n)], seed=8)
    keep = np.array([i for i in range(n) if i % 3 != 1], np.int32)
    a = q.state()[0]
    q.keep(keep)
    q.set_state(a=a[keep], sv=np.ones(len(keep), np.uint8))
    q.refresh()
    for frac in FRACS:
        want, m = host_route(q, wreg, w0, frac)
        got = q.positive_threshold(frac)
        assert got[1] == m == int((keep % 2 == 0).sum()) and np.float64(got[0]).tobytes() == np.float64(want).tobytes(), frac
    h.close()


def test_positive_threshold_refusals(gpu_required):
    h = small_handle()
    empty = capi.QpCache(h, 8, 0.004, 0.002)
    with pytest.raises(capi.PbdError) as e:
        empty.positive_threshold(.05)
    assert e.value.code == capi.PBD_ERR_STATE
    q, wreg, w0 = loaded_cache(h, 12, [-1] * 12, seed=2)   # examples, none of them positive: m == 0
    before = snapshot(q)
    with pytest.raises(capi.PbdError) as e:
        q.positive_threshold(.05)
    assert e.value.code == capi.PBD_ERR_STATE and snapshot(q) == before
    p, wreg, w0 = loaded_cache(h, 12, [1, -1] * 6, seed=2, capacity=16)
    before = snapshot(p)
    for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(capi.PbdError) as e:
            p.positive_threshold(bad)
        assert e.value.code == capi.PBD_ERR_ARG, bad
    t, m = capi.C.c_double(), capi.C.c_int()
    assert p.L.pbd_qp_positive_threshold(p.q, .05, None, capi.C.byref(m)) == capi.PBD_ERR_ARG
    assert p.L.pbd_qp_positive_threshold(p.q, .05, capi.C.byref(t), None) == capi.PBD_ERR_ARG
    assert snapshot(p) == before
    want = host_route(p, wreg, w0, .05)
    assert p.positive_threshold(.05) == want
    # a score that is not finite: an infinite feature in a positive with a = 0 (the solver's w stays finite)
    rng = np.random.default_rng(4)
    x, ids, b, d = columns(p, h.model, 2, rng, [-1, 1])
    x[1, 10] = np.inf
    p.put(x, ids, b, d)
    with pytest.raises(capi.PbdError) as e:
        p.positive_threshold(.05)
    assert e.value.code == capi.PBD_ERR_ARG and "example 13" in str(e.value)
    h.close()


# ---- 3. pbd_qp_clear ---------------------------------------------------------------------------------------------------------------------
def test_clear_equals_a_new_cache(gpu_required):
    model = make_model("tree_k")
    im = make_image(3, SW, SH)
    h = handle(model)
    h.set_threshold(root_percentile(h, im, 97.0))
    _, wreg, w0, noneg = model.qp_vectors()
    q = capi.QpCache(h, CAP, C_ * WPOS, C_, wreg, w0)
    q.noneg(noneg)
    assert q.mine(im, 1)[1] > 3
    q.fix(2)
    lb, ub, passes = q.opt(max_iter=50)
    n0 = q.prune()
    assert passes > 0 and np.abs(q.state()[2]).max() > 0 and q.state()[3][1] != 0 and 0 < n0
    fp = q.footprint()
    q.clear()
    new = capi.QpCache(h, CAP, C_ * WPOS, C_, wreg, w0)
    new.noneg(noneg)
    assert q.dims() == new.dims() == (q.dims()[0], q.dims()[1], CAP, 0) and q.footprint() == fp == new.footprint()
    same_caches(q, new, "cleared")
    a, sv, w, st = q.state()
    assert not a.any() and not sv.any() and not w.any() and not st.any()
    with pytest.raises(capi.PbdError) as e:               # nfix is 0 again: fix(1) on an empty cache is refused, fix(0) is not
        q.fix(1)
    assert e.value.code == capi.PBD_ERR_ARG
    for c in (q, new):                                    # a refill and a solve: a new cache's bits
        assert c.mine(im, 2)[1] > 3
        c.fix(1)
        c.opt(max_iter=50, seed=4)
    same_caches(q, new, "refilled")
    empty = capi.QpCache(h, 4, 1.0, 1.0)                  # a cache that never held anything, never solved
    empty.clear()
    assert empty.dims()[3] == 0
    h.close()


# ---- 4. train() is its sequence of primitives ----------------------------------------------------------------------------------------------
def by_hand(det, q, positives, negatives, warp, overlap, tol, max_iter, seed):
    """train.m:73-121 from the calls that existed plus the three primitives, one round -> the report's numbers"""
    model = det.handle.model
    q.noneg(model.qp_vectors()[3])
    q.clear()
    if warp:
        for i, (im, box) in enumerate(positives):
            det.writeWarped(im, [box], q, ids=[i + 1])
    else:
        det.latentPositives(positives, q, overlap)
    n = q.dims()[3]
    q.fix(n)
    q.prune()
    q.opt(tol, max_iter, seed)
    q.apply_weights()
    interval0 = det.handle.interval
    det.handle.set_interval(2)
    det.handle.set_threshold(-1)
    mined = []
    for i, im in enumerate(negatives):
        rec, wr, act = q.mine(im, 1 + i)
        mined.append((rec, wr, act))
        if act == capi.PBD_MINE_OPT:
            q.opt(tol, max_iter, seed)
            q.prune()
        elif act == capi.PBD_MINE_ONE:
            q.one(shuffled_support(q, seed))
        if act != capi.PBD_MINE_NONE:
            q.apply_weights()
        if int(q.support().sum()) == q.dims()[2]:
            break
    lb, ub, passes = q.opt(tol, max_iter, seed)
    q.apply_weights()
    thresh, m = q.positive_threshold(.05)
    det.handle.set_threshold(float(np.float32(thresh)))
    det.handle.set_interval(interval0)
    return dict(n=n, mined=mined, lb=lb, ub=ub, thresh=float(np.float32(thresh)), m=m)


def twins(model, dtype, capacity=CAP):
    out = []
    for _ in range(2):
        d = PartsBasedDetector(device=0, max_candidates=MAXC, dtype=dtype)
        d.distributeModel(model)
        _, wreg, w0, _ = model.qp_vectors()
        out.append((d, capi.QpCache(d.handle, capacity, C_ * WPOS, C_, wreg, w0)))
    return out


def latent_items(model, dtype=np.float32):
    """three latent positives on 100 x 80 frames: the best pose of a plain detect as the truth (every part box 20 pixels or more a side)"""
    items = []
    h = handle(model, dtype)
    for seed in (3, 4, 5):
        im = make_image(seed, SW, SH)
        h.set_threshold(root_percentile(h, im, 90.0))
        heads, boxes, _ = h.detect(im, capacity=MAXC)
        i = int(np.argmax(heads["score"]))
        items.append((im, boxes[i][:int(heads["nparts"][i])].copy()))
    h.close()
    return items


def check_round(rep, want, ta, tb, positives):
    da, qa = ta
    db, qb = tb
    same_caches(qa, qb, "train() against the sequence by hand")
    assert da.handle.weights().tobytes() == db.handle.weights().tobytes()
    assert np.float32(da.handle.threshold).tobytes() == np.float32(db.handle.threshold).tobytes() == np.float32(rep["thresh"]).tobytes()
    assert da.handle.interval == db.handle.interval == da.model.interval == 10
    assert rep["n"][0] == want["n"] == sum(rep["numpositives"]) > 0 and rep["mined"] == want["mined"] and len(rep["mined"]) >= 1
    assert (rep["lb"], rep["ub"], rep["thresh"]) == (want["lb"], want["ub"], want["thresh"]) and rep["lb"] <= rep["ub"]
    assert rep["n"][2] == qa.dims()[3] and rep["sv"][2] == int(qa.support().sum()) and len(rep["passes"]) == 2
    assert sum(w for _, w, _ in rep["mined"]) > 0 and math.isfinite(rep["thresh"])
    ids = qa.get()[1]
    assert want["m"] == int((ids[:, 0] == 1).sum()) == want["n"] and (ids[:, 0] == -1).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_train_latent_round_equals_the_sequence_by_hand(gpu_required, dtype):
    model = make_model("tree_k")
    positives = latent_items(model, dtype)
    negatives = [make_image(s, SW, SH) for s in (11, 12)]
    ta, tb = twins(model, dtype)
    got_model, report = train(None, positives, negatives, 0, overlap=0.6, max_iter=200, seed=3, detector=ta[0], cache=ta[1])
    want = by_hand(tb[0], tb[1], positives, negatives, 0, 0.6, .05, 200, 3)
    assert len(report) == 1 and got_model is ta[0].model
    check_round(report[0], want, ta, tb, positives)
    # the returned model on a fresh handle detects with the bits of the trained live handle
    fresh = capi.Handle(got_model, dtype=dtype, max_candidates=MAXC)
    assert got_model.thresh == report[0]["thresh"] and got_model.interval == 10
    for im in negatives[:1] + [positives[0][0]]:
        live = ta[0].handle.detect(im, capacity=MAXC)
        assert same(live, fresh.detect(im, capacity=MAXC))
    fresh.close()
    for d, _ in (ta, tb):
        d.handle.close()


def test_train_warped_round_equals_the_sequence_by_hand(gpu_required):
    model = init_model(None, None, 4, tsize=(5, 5))
    positives = [(make_image(s, SW, SH), box) for s, box in ((3, (10.0, 8.0, 49.0, 47.0)), (4, (30.5, 20.0, 75.0, 66.5)), (5, (1.0, 1.0, 12.0, 12.0)),
                                                           (6, (40.0, 30.0, 95.0, 78.0)))]      # the third is below 20 x 20: skipped
    negatives = [make_image(s, SW, SH) for s in (11, 12)]
    ta, tb = twins(model, np.float32)
    _, report = train(None, positives, negatives, 1, max_iter=200, seed=1, detector=ta[0], cache=ta[1])
    want = by_hand(tb[0], tb[1], positives, negatives, 1, 0.6, .05, 200, 1)
    assert report[0]["numpositives"] == [3] and ta[1].get()[1][:3, 1].tolist() == [1, 2, 4]
    check_round(report[0], want, ta, tb, positives)
    for d, _ in (ta, tb):
        d.handle.close()


def test_train_creates_and_closes_its_own_detector(gpu_required):
    """the one-call form: model in, model out, with the defaults (capacity 10 * (wpos + 1) * positives) and a detector option"""
    model = make_model("tree_k")
    positives = latent_items(model)
    negatives = [make_image(11, SW, SH)]
    m1, r1 = train(model, positives, negatives, 0, max_iter=200, seed=3, conv_mode=capi.PBD_CONV_EXACT, max_candidates=MAXC)
    d = PartsBasedDetector(device=0, conv_mode=capi.PBD_CONV_EXACT, max_candidates=MAXC)
    d.distributeModel(model)
    _, wreg, w0, _ = model.qp_vectors()
    q = capi.QpCache(d.handle, 10 * (WPOS + 1) * len(positives), C_ * WPOS, C_, wreg, w0)
    want = by_hand(d, q, positives, negatives, 0, 0.6, .05, 200, 3)
    assert (r1[0]["lb"], r1[0]["ub"], r1[0]["thresh"], r1[0]["mined"]) == (want["lb"], want["ub"], want["thresh"], want["mined"])
    assert m1.weight_vector().tobytes() == d.handle.weights().tobytes() and m1.thresh == d.handle.threshold and m1.interval == 10
    assert model.weight_vector().tobytes() != m1.weight_vector().tobytes()      # the model given is not touched
    d.handle.close()


def test_cpp_demo_trains(gpu_required, tmp_path):
    """host/demo.cpp --train (pbd::PartsBasedDetector::train): the report's lines are the binding's for the same inputs"""
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "host", "pbd_demo")
    assert os.path.exists(exe), "build() did not produce the C++ demo"
    model = make_model("tree_k")
    positives = latent_items(model)
    negatives = [make_image(s, SW, SH) for s in (11, 12)]
    model.save(str(tmp_path / "model.bin"))
    args = [exe, str(tmp_path / "model.bin"), str(tmp_path / "p0.raw"), str(SW), str(SH), "3", "--train"]
    for i, (im, truth) in enumerate(positives):
        im.tofile(str(tmp_path / f"p{i}.raw"))
        args += ["--poslatent", str(tmp_path / f"p{i}.raw"), ";".join(",".join(str(int(v)) for v in row) for row in truth)]
    for i, im in enumerate(negatives):
        im.tofile(str(tmp_path / f"n{i}.raw"))
        args += ["--mine", str(tmp_path / f"n{i}.raw")]
    out = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    _, report = train(model, positives, negatives, 0, conv_mode=capi.PBD_CONV_EXACT)      # (the demo's detector: the exact bank, the defaults)
    r = report[0]
    g = "%.17g"
    want = ["Train 0 numpositives: " + " ".join(str(c) for c in r["numpositives"]),
            "Train 0 n: " + " ".join(str(v) for v in r["n"]), "Train 0 sv: " + " ".join(str(v) for v in r["sv"]),
            "Train 0 lb: " + g % r["lb"], "Train 0 ub: " + g % r["ub"], "Train 0 thresh: " + g % r["thresh"],
            "Train 0 mined: " + " ".join(",".join(str(v) for v in m) for m in r["mined"]),
            "Train 0 passes: " + " ".join(str(v) for v in r["passes"]), "Interval: 10", "Threshold: " + g % r["thresh"]]
    assert [l for l in out.stdout.splitlines() if l.startswith(("Train ", "Interval", "Threshold"))] == want, out.stdout


# ---- 5. train_model() end to end -----------------------------------------------------------------------------------------------------------
PARENTS, KS, SIDE = [-1, 0, 0], [1, 2, 2], 96


def synthetic():
    """ten 96 x 96 positives: one fixed textured 24 x 24 patch per part pasted at its keypoint on noise; part 1 right of or below the
    root, part 2 left of or above it — two clusters each —; two noise negatives.  Keypoints are 1-based pixel coordinates."""
    rng = np.random.default_rng(2024)
    patches = [rng.integers(0, 2, (6, 6, 1)).repeat(4, 0).repeat(4, 1).repeat(3, 2).astype(np.uint8) * 200 + 20 * (p + 1) for p in range(3)]
    offs = {1: [(26, 0), (0, 26)], 2: [(-26, 0), (0, -26)]}
    positives = []
    for i in range(10):
        root = np.array([48 + rng.integers(-4, 5), 48 + rng.integers(-4, 5)])
        pts = np.stack([root, root + offs[1][i % 2] + rng.integers(-1, 2, 2), root + offs[2][(i // 2) % 2] + rng.integers(-1, 2, 2)]).astype(np.float64)
        im = rng.integers(90, 130, (SIDE, SIDE, 3)).astype(np.uint8)
        for p in range(3):
            x, y = int(pts[p, 0]) - 12, int(pts[p, 1]) - 12
            im[y - 1:y + 23, x - 1:x + 23] = patches[p]          # (the 1-based point is the patch's centre)
        positives.append((im, pts))
    negatives = [rng.integers(90, 130, (SIDE, SIDE, 3)).astype(np.uint8) for _ in range(2)]
    return positives, negatives


def test_train_model_end_to_end(gpu_required):
    positives, negatives = synthetic()
    kept = {}

    def keeping_train(model, pos, neg, warp, **kw):
        """train() on a detector and a cache the test can look at afterwards (the last round's stay open)"""
        for d, q in kept.pop("last", []):
            d.handle.close()
        d = PartsBasedDetector(device=0, conv_mode=capi.PBD_CONV_EXACT, max_candidates=MAXC)
        d.distributeModel(model)
        _, wreg, w0, _ = model.qp_vectors()
        q = capi.QpCache(d.handle, 10 * (WPOS + 1) * max(len(pos), 1), C_ * WPOS, C_, wreg, w0)
        kept["last"] = [(d, q)]
        kept["pos"] = pos
        return train(None, pos, neg, warp, detector=d, cache=q, **kw)

    model, reports = train_model(positives, negatives, KS, PARENTS, 4, tsize=(5, 5), R=4, _train=keeping_train, max_iter=200)
    # structure: the counts follow from K and the tree, the anchors are build_model's on the same idx
    idx = reports["idx"]
    assert idx.shape == (3, 10) and [int(idx[p].max()) + 1 for p in range(3)] == KS
    assert len(model.filtersw) == sum(KS) and len(model.defw) == KS[1] + KS[2] and len(model.biasw) == 1 + KS[1] * KS[0] + KS[2] * KS[0]
    assert model.parentid == [PARENTS] and model.interval == 10 and model.sbin == 4
    points = np.stack([p[1] for p in positives])
    boxes = point_to_box(points, PARENTS)
    w, hgt = boxes[:, 0, 2] - boxes[:, 0, 0] + 1, boxes[:, 0, 3] - boxes[:, 0, 1] + 1
    init = init_model(w, hgt, 4, (5, 5))
    joint = build_model([merge_models([init, init])] * 3, data_def(points, w, hgt, (5, 5)), idx, PARENTS)
    assert np.asarray(model.anchors).tolist() == np.asarray(joint.anchors).tolist()
    # numbers: a finite threshold, lb <= ub in every round
    rounds = [r for rep in reports["parts"].values() for r in rep] + reports["final1"] + reports["final"]
    assert len(rounds) == sum(KS) + 2 and all(r["lb"] <= r["ub"] for r in rounds) and math.isfinite(model.thresh)
    assert model.thresh == reports["final"][0]["thresh"]
    # detection.  The cache holds every latent positive's column x' = cpos x / wreg; (w + w0 .* wreg) . x' / cpos is weights . x, the pose's
    # score under the trained weights in double.  A fresh handle of the returned model scores that same pose — it is in the crop's search
    # space at the model's interval — through the exact float32 bank and the float32 DP: a sum of the column's n non-zero products, each
    # rounded to float32, accumulated in float32 in some order, so within (n + 7) 2^-24 sum|terms| of the exact value (the form of the
    # bound DESIGN §5.15's tests hold w . x against a record's score to), plus 2^-24 |score| for the record's float32 head.  A positive
    # whose cached score clears the threshold by more than that must come back from detect(); by the threshold's definition at most
    # ceil(.05 m) positives sit at or below it, and no more than those may be exempt.
    d, q = kept["last"][0]
    _, wreg, w0, _ = model.qp_vectors()
    x, ids, _, _ = q.get()
    pos = np.flatnonzero(ids[:, 0] == 1)
    m = len(pos)
    assert m == reports["final"][0]["n"][0] >= 8
    w_eff = q.state()[2] + w0 * wreg
    scores = q.score(w_eff, pos.astype(np.int32)) / (C_ * WPOS)
    assert Model.positive_threshold(scores, .05) == q.positive_threshold(.05)[0]
    fresh = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, max_candidates=MAXC)
    assert fresh.threshold == model.thresh
    exempt = 0
    for e, sc in zip(pos, scores):
        col = x[e]
        terms, at = [], 1
        for _ in range(int(col[0])):
            i1, i2 = int(col[at]), int(col[at + 1])
            terms += list(np.abs(w_eff[i1 - 1:i2] * col[at + 2:at + 2 + i2 - i1 + 1].astype(np.float64)) / (C_ * WPOS))
            at += 2 + i2 - i1 + 1
        nz = sum(1 for t in terms if t != 0)
        margin = (nz + 7) * 2.0 ** -24 * math.fsum(terms) + 2.0 ** -24 * abs(sc)
        im, truth = kept["pos"][int(ids[e, 1]) - 1][:2]
        (cx, cy, cw, ch), _ = capi.croppos(truth, len(truth), im.shape[1], im.shape[0])
        found = len(fresh.detect(im[cy:cy + ch, cx:cx + cw], capacity=MAXC)[0])
        print(f"TRAIN-MODEL positive {int(ids[e, 1])}: cached score {sc:.9g} threshold {model.thresh:.9g} margin {margin:.3e} candidates {found}")
        if sc > model.thresh + margin:
            assert found >= 1, (int(ids[e, 1]), sc, model.thresh)
        else:
            exempt += 1
    assert exempt <= math.ceil(.05 * m), (exempt, m)
    fresh.close()
    d.handle.close()
