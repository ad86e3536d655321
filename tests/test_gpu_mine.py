"""Hard-negative mining on the device (k_qp_mine.hip, k_qp.hip's write, pbd_qp_mine.cpp; include/pbd_c.h "hard-negative mining"):
pbd_qp_mine_* against the route it replaces — a plain detect, then pbd_qp_write of every record it returned — on twin handles and twin
caches, in bits; the upper bound against tests/mine_ref.py's restated block sum; the action; the capacity cut; batches; a weight
update between two calls; every refusal with the cache untouched; the C++ demo."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import PartsBasedDetector, capi
from partsbaseddetector_amd.detector import shuffled_support
from partsbaseddetector_amd.model import make_image, make_mixed_person_model, make_tree_model, make_tree_model_k, make_voc_like_model
from tests import mine_ref

pytestmark = pytest.mark.gpu

SW, SH = 100, 80
CAP = 64            # examples of a cache
MAXC = 4096
CPOS, CNEG = 0.002, 0.004
RAW = None
SORT = (capi.PBD_CAND_SORT, 0.0)
SORT_NMS = (capi.PBD_CAND_SORT_NMS, 0.95)   # (a 26-part pose covers most of a 100 x 80 frame: at .5 one record survives)
PARTS = (capi.PBD_NMS_PARTS, 1000)


def make_model(kind):
    if kind == "tree_k":
        return make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21)
    if kind == "multi":
        return make_voc_like_model(seed=11)
    return make_mixed_person_model(seed=5, K=2)


def handle(model, dtype=np.float32, mode=RAW, nms=None, pad=0, maxc=MAXC, **kw):
    h = capi.Handle(model, dtype=dtype, max_candidates=maxc, cand_filter=mode, cand_nms=nms, **kw)
    if pad:
        h.set_boundary_pad(pad)
    return h


def root_scores(h, im):
    """every finite root score of the frame on this handle, ascending"""
    h.pyramid(im); h.pdf(); h.dp_min()
    v = np.concatenate([h.root(l, c)[0].ravel() for l in range(h._geo["nlevels"]) for c in range(h.model.ncomponents)])
    return np.sort(v[np.isfinite(v)].astype(np.float64))


def set_threshold(handles, im, lo=4, hi=MAXC, also=()):
    """a percentile of the first handle's own root scores, the highest of the list at which its plain detect returns at least `lo`
    records (for the frames `also` too); set on all handles -> the plain detect's records of `im`"""
    vals = root_scores(handles[0], im)
    for pct in (99.0, 97.0, 90.0, 75.0, 50.0, 10.0):
        t = float(np.float32(np.percentile(vals, pct)))
        handles[0].set_threshold(t)
        try:
            got = handles[0].detect(im, capacity=MAXC)
        except capi.PbdError:                            # (more raw records than max_candidates: no lower threshold will do)
            break
        if len(got[0]) >= lo and all(len(handles[0].detect(f, capacity=MAXC)[0]) >= lo for f in also):
            break
    assert 3 < len(got[0]) < hi, len(got[0])
    for h in handles[1:]:
        h.set_threshold(t)
    return got


def pick_frame(handles, lo=4):
    """the first of the frames make_image(3 ..) on which set_threshold finds a threshold with at least `lo` records (the NMS modes keep
    a handful of the person model's poses on a frame this small, on some frames fewer than four) -> (frame, its records)"""
    for seed in (3, 4, 5, 6, 7, 8):
        im = make_image(seed, SW, SH)
        try:
            return im, set_threshold(handles, im, lo)
        except AssertionError:
            continue
    raise AssertionError("no frame with more than 3 records")


def snapshot(q):
    """everything of a cache a call could change, as bytes: every column of the capacity, dims, the solver's a, sv and stats"""
    cap = q.dims()[2]
    a, sv, _, st = q.state()
    return [v.tobytes() for v in q.get(0, cap)] + [repr(q.dims()), a.tobytes(), sv.tobytes(), st.tobytes()]


def same_caches(q, t, what=""):
    for i, (g, e) in enumerate(zip(snapshot(q), snapshot(t))):
        assert g == e, (what, ("x", "ids", "b", "d", "dims", "a", "sv", "stats")[i])


def host_route(h, q, im, id):
    """what mining replaces: the plain detect, every record home, and back into pbd_qp_write; ub grown as detect.m:135 has it is not
    part of that route (the library had no counterpart) -> (records, written, heads)"""
    heads, _, locs = h.detect(im, capacity=MAXC)
    return len(heads), q.write(heads, locs, -1, id), heads


# ---- 1. the mined examples are the host route's, in bits -------------------------------------------------------------------------
MODES = {"raw": (RAW, None), "sort": (SORT, None), "sort_nms": (SORT_NMS, None), "nms_parts": (SORT_NMS, PARTS)}
# scalar type x filter x pad in full on the small tree; the person and the multi-component model float32 unpadded and float64 padded
GRID = [("tree_k", d, p, m) for d in (np.float32, np.float64) for p in (0, 3) for m in MODES] + \
       [(k, d, p, m) for k in ("person", "multi") for d, p in ((np.float32, 0), (np.float64, 3)) for m in MODES]


@pytest.mark.parametrize("kind, dtype, pad, filt", GRID, ids=[f"{k}-{np.dtype(d).name}-pad{p}-{m}" for k, d, p, m in GRID])
def test_equals_the_host_route(gpu_required, kind, dtype, pad, filt):
    mode, nms = MODES[filt]
    model = make_model(kind)
    h, g = (handle(model, dtype, mode, nms, pad) for _ in range(2))
    im, want = pick_frame([g, h])
    q, t = capi.QpCache(h, CAP, CPOS, CNEG), capi.QpCache(g, CAP, CPOS, CNEG)
    nrec, nwr, heads = host_route(g, t, im, 5)
    assert nrec == len(want[0]) and nwr == min(nrec, CAP)
    rec, wr, act = q.mine(im, 5)
    assert (rec, wr) == (nrec, nwr)
    st = q.state()[3]
    assert st[3] == mine_ref.ub_term_sum(heads["score"], CNEG) and act == mine_ref.action(st[1], st[3], q.dims()[3], CAP)
    t.state()                                            # (the twin's solver state is allocated like the mined cache's: a = 0, sv = 1)
    for name, a, b in zip(("x", "ids", "b", "d"), q.get(0, CAP), t.get(0, CAP)):
        assert a.tobytes() == b.tobytes(), (name, np.argwhere(a != b)[:5])
    assert q.dims() == t.dims()
    for name, a, b in zip(("a", "sv"), q.state()[:2], t.state()[:2]):
        assert a.tobytes() == b.tobytes(), name
    ids = q.get()[1]
    assert (ids[:, 0] == -1).all() and (ids[:, 1] == 5).all() and (ids[:, 2] == heads["level"][:nwr]).all()
    # the frame's feature planes are resident, no frame is pending: the handle detects again, and the same
    again = h.detect(im, capacity=MAXC)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, want))
    h.close(); g.close()


def test_mine_dev_from_a_torch_tensor(gpu_required):
    import torch
    model = make_model("tree_k")
    im = make_image(3, SW, SH)
    h, g = handle(model), handle(model)
    set_threshold([g, h], im)
    q, t = capi.QpCache(h, CAP, CPOS, CNEG), capi.QpCache(g, CAP, CPOS, CNEG)
    d_im = torch.from_numpy(im).cuda()
    torch.cuda.synchronize()
    got = q.mine_dev(d_im.data_ptr(), SW, SH, 3, 11)
    assert got == t.mine(im, 11)
    same_caches(q, t, "device frame")
    nrec, nwr, _ = host_route(g, capi.QpCache(g, CAP, CPOS, CNEG), im, 11)
    assert got[:2] == (nrec, nwr)
    h.close(); g.close()


# ---- 2. the upper bound and the action ---------------------------------------------------------------------------------------------
def test_upper_bound_and_action(gpu_required):
    model = make_model("tree_k")
    im = make_image(3, SW, SH)
    h, g = handle(model), handle(model)
    vals = root_scores(g, im)
    # the root bias moved so that the 99th percentile of the root scores sits at -1, the threshold at the 98th: records on both sides
    shift = -1.0 - float(np.percentile(vals, 99.0))
    w = g.weights()
    w[model.biasid[0][0][0]] += shift
    t0 = float(np.float32(np.percentile(vals, 98.0) + shift))
    for x in (h, g):
        x.set_weights(w)
        x.set_threshold(t0)
    heads = g.detect(im, capacity=MAXC)[0]
    sc = heads["score"]
    assert 3 < len(sc) < MAXC and (sc < -1).any() and (sc > -1).any(), (len(sc), sc.min(), sc.max())
    S = mine_ref.ub_term_sum(sc, CNEG)
    assert S > 0
    cap = 1024
    q = capi.QpCache(h, cap, CPOS, CNEG)
    seen = []

    def check(rec, wr, act, ub_before, S_f):
        st, n = q.state()[3], q.dims()[3]
        assert st[3].tobytes() == np.float64(ub_before + S_f).tobytes(), (st[3], ub_before, S_f)
        assert act == mine_ref.action(st[1], st[3], n, cap) and n < cap
        seen.append(act)

    # a fresh cache: lb = 0, ub = S: 1 - 0 > .05
    rec, wr, act = q.mine(im, 1)
    assert (rec, wr) == (len(sc), len(sc))
    check(rec, wr, act, np.float64(0.0), S)
    assert act == capi.PBD_MINE_ONE
    # a state with lb < 0 put by the test: large multipliers, so w'w / 2 outweighs l
    q.set_state(a=np.full(rec, 1e6))
    q.refresh()
    st = q.state()[3]
    assert st[1] < 0
    rec2, wr2, act = q.mine(im, 2)
    assert (rec2, wr2) == (rec, rec)
    check(rec2, wr2, act, st[3], S)
    assert act == capi.PBD_MINE_OPT
    # a state with lb > 0 within .01 of ub — the solver's own, on a cache of the frame's few best records —, then a frame without
    # records: ub stays, the bounds agree
    q.close()
    q = capi.QpCache(h, cap, CPOS, CNEG)
    h.set_threshold(float(np.sort(sc)[-6]))
    rec3 = q.mine(im, 3)[0]
    assert 0 < rec3 <= 6
    lb, ub, passes = q.opt(tol=.01, max_iter=3000, seed=0)
    assert lb > 0 and 1 - lb / ub < .01, (lb, ub, passes)
    st = q.state()[3]
    h.set_threshold(1e9)
    rec4, wr4, act = q.mine(im, 4)
    assert (rec4, wr4) == (0, 0)
    check(rec4, wr4, act, st[3], np.float64(0.0))
    assert act == capi.PBD_MINE_NONE and sorted(seen) == [capi.PBD_MINE_NONE, capi.PBD_MINE_ONE, capi.PBD_MINE_OPT]
    h.close(); g.close()


# ---- 3. a cache with room for fewer records than the frame has -------------------------------------------------------------------
@pytest.mark.parametrize("mode", [RAW, SORT], ids=["raw", "sort"])
def test_capacity_cut(gpu_required, mode):
    model = make_model("multi")
    im = make_image(3, SW, SH)
    h, g = handle(model, mode=mode), handle(model, mode=mode)
    heads = set_threshold([g, h], im, lo=8)[0]
    r = len(heads)
    cap = r - 3                                          # room for all but the last three
    q, t = capi.QpCache(h, cap, CPOS, CNEG), capi.QpCache(g, cap, CPOS, CNEG)
    assert host_route(g, t, im, 4)[:2] == (r, cap)
    S = mine_ref.ub_term_sum(heads["score"], CNEG)
    rec, wr, act = q.mine(im, 4)
    assert (rec, wr, act) == (r, cap, capi.PBD_MINE_OPT) and q.dims()[3] == cap
    assert q.state()[3][3].tobytes() == np.float64(S).tobytes()          # every record's term, the refused ones' too
    t.state()
    for name, a, b in zip(("x", "ids", "b", "d"), q.get(0, cap), t.get(0, cap)):
        assert a.tobytes() == b.tobytes(), name
    before = snapshot(q)
    rec, wr, act = q.mine(im, 5)                         # the full cache: nothing written, ub grows again
    assert (rec, wr, act) == (r, 0, capi.PBD_MINE_OPT) and q.dims()[3] == cap
    after = snapshot(q)
    assert after[:7] == before[:7]
    assert q.state()[3][3].tobytes() == np.float64(np.float64(S) + S).tobytes()
    h.close(); g.close()


def test_room_ends_inside_the_frame_behind_other_examples(gpu_required):
    """examples already there: the frame's first records go behind them, the columns behind n (none are left) and in front stay"""
    model = make_model("tree_k")
    im = make_image(3, SW, SH)
    h, g = handle(model), handle(model)
    heads = set_threshold([g, h], im, lo=8)[0]
    r = len(heads)
    cap = 2 * r - 2
    q, t = capi.QpCache(h, cap, CPOS, CNEG), capi.QpCache(g, cap, CPOS, CNEG)
    assert q.mine(im, 1)[:2] == (r, r) and q.mine(im, 2)[:2] == (r, r - 2)
    assert host_route(g, t, im, 1)[1] == r and host_route(g, t, im, 2)[1] == r - 2
    t.state()
    for name, a, b in zip(("x", "ids", "b", "d"), q.get(0, cap), t.get(0, cap)):
        assert a.tobytes() == b.tobytes(), name
    h.close(); g.close()


# ---- 4. no records -------------------------------------------------------------------------------------------------------------------
def test_no_records(gpu_required):
    model = make_model("person")
    im = make_image(3, SW, SH)
    h = handle(model)
    want = set_threshold([h], im)
    t0 = h.threshold
    q = capi.QpCache(h, CAP, CPOS, CNEG)
    q.mine(im, 1)
    before = snapshot(q)
    h.set_threshold(1e9)
    rec, wr, act = q.mine(im, 2)
    assert (rec, wr) == (0, 0) and snapshot(q) == before
    st = q.state()[3]
    assert act == mine_ref.action(st[1], st[3], q.dims()[3], CAP)
    h.set_threshold(t0)                                  # the handle takes a plain detect afterwards
    got = h.detect(im, capacity=MAXC)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    h.close()


# ---- 5. batches ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [RAW, SORT_NMS], ids=["raw", "sort_nms"])
def test_batch_equals_the_frames_one_by_one(gpu_required, mode):
    model = make_model("tree_k")
    ims = [make_image(s, SW, SH) for s in (3, 4, 5)]
    h, g = handle(model, mode=mode), handle(model, mode=mode)
    set_threshold([g, h], ims[0], also=ims[1:])
    counts = [len(g.detect(im, capacity=MAXC)[0]) for im in ims]
    assert min(counts[:2]) >= 2, counts
    for cap in (sum(counts) + 7, counts[0] + counts[1] // 2):
        q, t = capi.QpCache(h, cap, CPOS, CNEG), capi.QpCache(g, cap, CPOS, CNEG)
        one = [t.mine(im, 7 + i) for i, im in enumerate(ims)]
        rec, wr, act = q.mine_batch(ims, [7, 8, 9])
        assert list(rec) == counts == [o[0] for o in one] and list(wr) == [o[1] for o in one] and act == one[-1][2]
        if cap < sum(counts):
            assert list(wr) == [counts[0], counts[1] // 2, 0]
        same_caches(q, t, f"capacity {cap}")
        ids = q.get()[1]
        assert set(ids[:, 1]) <= {7, 8, 9} and (np.diff(ids[:, 1]) >= 0).all()
        q.close(); t.close()
    h.close(); g.close()


# ---- 6. after a weight update --------------------------------------------------------------------------------------------------------
def test_after_a_weight_update(gpu_required):
    model = make_model("tree_k")
    im, im2 = make_image(3, SW, SH), make_image(6, SW, SH)
    h, g = handle(model), handle(model)
    set_threshold([g, h], im)
    q, t = capi.QpCache(h, 256, CPOS, CNEG), capi.QpCache(g, 256, CPOS, CNEG)
    r1 = q.mine(im, 1)
    assert host_route(g, t, im, 1)[:2] == r1[:2]
    for c in (q, t):
        c.opt(tol=.05, max_iter=50, seed=3)
        c.apply_weights()
    assert h.weights().tobytes() == g.weights().tobytes() and h.weights().tobytes() != model.weight_vector().astype(np.float64).tobytes()
    set_threshold([g, h], im2)                           # (the new weights' scores: a threshold that yields records again)
    r2 = q.mine(im2, 2)                                  # the re-planned frame's planes, the new weights' detections
    assert host_route(g, t, im2, 2)[:2] == r2[:2] and r2[0] > 3
    t.state()
    for name, a, b in zip(("x", "ids", "b", "d"), q.get(0, 256), t.get(0, 256)):
        assert a.tobytes() == b.tobytes(), name
    for name, a, b in zip(("a", "sv", "w"), q.state()[:3], t.state()[:3]):
        assert a.tobytes() == b.tobytes(), name
    h.close(); g.close()


def test_mine_negatives_is_the_loop_of_primitives(gpu_required):
    model = make_model("tree_k")
    ims = [make_image(s, SW, SH) for s in (3, 4, 5, 6)]
    dets = []
    for _ in range(2):
        d = PartsBasedDetector(device=0, max_candidates=MAXC)
        d.distributeModel(model)
        dets.append(d)
    set_threshold([dets[0].handle, dets[1].handle], ims[0])
    q, t = capi.QpCache(dets[0].handle, CAP, CPOS, CNEG), capi.QpCache(dets[1].handle, CAP, CPOS, CNEG)
    got = dets[0].mineNegatives(ims, q, first_id=10, tol=.05, max_iter=40, seed=2)
    want = []
    for i, im in enumerate(ims):                         # train.m:99-108, written out
        rec, wr, act = t.mine(im, 10 + i)
        want.append((rec, wr, act))
        if act == capi.PBD_MINE_OPT:
            t.opt(.05, 40, 2)
            t.prune()
        elif act == capi.PBD_MINE_ONE:
            t.one(shuffled_support(t, 2))
        if act != capi.PBD_MINE_NONE:
            t.apply_weights()
        if int(t.state()[1][:t.dims()[3]].sum()) == CAP:
            break
    assert got == want and len(got) >= 1 and all(a in (0, 1, 2) for _, _, a in got)
    same_caches(q, t, "mineNegatives")
    assert dets[0].handle.weights().tobytes() == dets[1].handle.weights().tobytes()
    other = capi.QpCache(dets[1].handle, CAP, CPOS, CNEG)
    with pytest.raises(ValueError):
        dets[0].mineNegatives(ims, other)
    for d in dets:
        d.handle.close()


# ---- 7. refusals leave nothing behind -------------------------------------------------------------------------------------------------
def refused(q, im, code, what):
    before = snapshot(q)
    with pytest.raises(capi.PbdError) as e:
        q.mine(im, 9)
    assert e.value.code == code, (what, str(e.value))
    assert snapshot(q) == before, what
    return e.value


def good_mine_equals_host_route(h, q, im, model_handle_kw):
    """on the handle that just refused: a mine that is not refused gives what the host route gives on a twin with the same examples"""
    g = handle(h.model, **model_handle_kw)
    g.set_threshold(h.threshold)
    n0 = q.dims()[3]
    t = capi.QpCache(g, q.dims()[2], CPOS, CNEG)
    if n0:
        t.put(*q.get(0, n0))
    rec, wr, _ = q.mine(im, 6)
    assert host_route(g, t, im, 6)[:2] == (rec, wr) and rec > 0
    for name, a, b in zip(("x", "ids", "b", "d"), q.get(0, q.dims()[2]), t.get(0, q.dims()[2])):
        assert a.tobytes() == b.tobytes(), name
    g.close()


def test_refused_repeated_dense_start(gpu_required):
    """two parts that share their only filter: every record of every frame repeats a dense start (qp_write.m:34-35), so the only mine
    this handle accepts is one without records; a refusal followed by a mine WITH records: test_ids_shared_only_in_unpicked_mixtures"""
    model = make_tree_model([-1, 0], 1, seed=3)
    model.filterid = [[[0], [0]]]
    model.filtersw = model.filtersw[:1]
    im = make_image(3, SW, SH)
    h = handle(model)
    heads, _, locs = set_threshold([h], im)
    q = capi.QpCache(h, CAP, CPOS, CNEG)
    with pytest.raises(capi.PbdError) as e:              # the host route refuses the same records
        q.write(heads, locs, -1, 9)
    assert e.value.code == capi.PBD_ERR_ARG
    err = refused(q, im, capi.PBD_ERR_ARG, "shared filter")
    assert "record 0 of frame 0" in str(err) and "qp_write.m:34-35" in str(err)
    h.set_threshold(1e9)
    assert q.mine(im, 9)[:2] == (0, 0) and q.dims()[3] == 0
    h.close()


def test_filter_shared_between_components_is_accepted(gpu_required):
    model = make_voc_like_model(seed=11, roots=((5, 5), (5, 5)), part_size=(5, 5), nparts=(3, 3))
    model.filterid[1][1] = list(model.filterid[0][1])
    im = make_image(3, SW, SH)
    h, g = handle(model), handle(model)
    for lo in (4, 16, 64, 256):                          # a threshold at which both components detect
        heads = set_threshold([g, h], im, lo)[0]
        if {0, 1} <= set(heads["component"]):
            break
    assert {0, 1} <= set(heads["component"]), "both components detect"
    q, t = capi.QpCache(h, CAP, CPOS, CNEG), capi.QpCache(g, CAP, CPOS, CNEG)
    assert q.mine(im, 5)[:2] == host_route(g, t, im, 5)[:2]
    t.state()
    for name, a, b in zip(("x", "ids", "b", "d"), q.get(0, CAP), t.get(0, CAP)):
        assert a.tobytes() == b.tobytes(), name
    h.close(); g.close()


def test_ids_shared_only_in_unpicked_mixtures(gpu_required):
    """the repeat test is exact: parts 1 and 2 share a filter in their mixture 1 only.  A frame on which some pose picks both is refused,
    naming that record, as the host route refuses it; a frame on which poses pick the shared filter for one of the two parts only — the
    other holds it in a mixture the pose did not pick — is accepted and equals the host route, on the handle that just refused"""
    model = make_tree_model_k([-1, 0, 0], [1, 2, 2], seed=8)
    model.filterid[0][2][1] = model.filterid[0][1][1]
    h, g = handle(model), handle(model)
    bad = good = None
    for seed in range(3, 15):                            # the first frame and threshold of either kind
        im = make_image(seed, SW, SH)
        vals = root_scores(g, im)
        for pct in (99.8, 99.5, 99.0, 98.0, 97.0, 95.0):
            thr = float(np.float32(np.percentile(vals, pct)))
            g.set_threshold(thr)
            heads, _, locs = g.detect(im, capacity=MAXC)
            m1, m2 = locs[:, 1, 2] == 1, locs[:, 2, 2] == 1
            if len(heads) >= 2 and (m1 & m2).any() and bad is None:
                bad = (im, thr, int(np.argmax(m1 & m2)))
            if len(heads) >= 2 and not (m1 & m2).any() and (m1 ^ m2).any() and good is None:
                good = (im, thr, int((m1 ^ m2).sum()))
        if bad and good:
            break
    assert bad and good, (bad is not None, good is not None)
    q, t = capi.QpCache(h, CAP, CPOS, CNEG), capi.QpCache(g, CAP, CPOS, CNEG)
    im, thr, first = bad
    for x in (h, g):
        x.set_threshold(thr)
    heads, _, locs = g.detect(im, capacity=MAXC)
    with pytest.raises(capi.PbdError) as e:
        t.write(heads, locs, -1, 5)
    assert e.value.code == capi.PBD_ERR_ARG
    err = refused(q, im, capi.PBD_ERR_ARG, "a pose picks the shared mixtures")
    assert f"record {first} of frame 0" in str(err) and "qp_write.m:34-35" in str(err)
    im, thr, unpicked = good
    for x in (h, g):
        x.set_threshold(thr)
    heads, _, locs = g.detect(im, capacity=MAXC)
    assert unpicked > 0 and q.mine(im, 5)[:2] == (len(heads), t.write(heads, locs, -1, 5)) and q.dims()[3] == len(heads) >= 2
    assert snapshot(q)[:7] == snapshot(t)[:7]            # (all but the stats: the host route does not grow ub)
    h.close(); g.close()


def test_shuffle_is_the_librarys_draw(gpu_required):
    """detector.shuffled_support restates pbd_qp_opt's shuffle: one pass of opt (refresh, every sv set, the shuffled pass) leaves the
    multipliers that refresh + one(shuffled_support) leaves — the pass's result depends on its order"""
    model = make_model("tree_k")
    im = make_image(3, SW, SH)
    h = handle(model)
    set_threshold([h], im, lo=12)
    q, t = capi.QpCache(h, CAP, CPOS, CNEG), capi.QpCache(h, CAP, CPOS, CNEG)
    n = q.mine(im, 1)[1]
    assert t.mine(im, 1)[1] == n >= 12
    for seed in (0, 7):
        q.set_state(a=np.zeros(n), sv=np.ones(n, np.uint8)); t.set_state(a=np.zeros(n), sv=np.ones(n, np.uint8))
        order = shuffled_support(t, seed)                # (of the state just put: every example a support vector)
        assert sorted(int(i) for i in order) == list(range(n)) and list(order) != list(range(n))
        q.opt(tol=-1.0, max_iter=1, seed=seed)
        t.refresh()
        t.one(order)
        for name, a, b in zip(("a", "sv", "w"), q.state()[:3], t.state()[:3]):
            assert a.tobytes() == b.tobytes(), (seed, name)
        t.set_state(a=np.zeros(n), sv=np.ones(n, np.uint8))
        t.refresh()
        t.one(np.arange(n, dtype=np.int32))          # (another order gives other multipliers: the comparison above can tell)
        assert t.state()[0].tobytes() != q.state()[0].tobytes()
    h.close()


def test_refused_capacity(gpu_required):
    model = make_model("tree_k")
    im = make_image(3, SW, SH)
    big = handle(model)
    need = len(set_threshold([big], im, lo=12)[0])
    vals = root_scores(big, im)
    h = handle(model, maxc=8)
    h.set_threshold(big.threshold)
    q = capi.QpCache(h, CAP, CPOS, CNEG)
    err = refused(q, im, capi.PBD_ERR_CAPACITY, "max_candidates")
    assert err.records == [need] and need > 8
    h.set_threshold(float(np.float32(vals[-6])))         # at most five records pass
    good_mine_equals_host_route(h, q, im, dict(maxc=8))
    big.close(); h.close()


def test_refused_pending_and_settings(gpu_required):
    model = make_model("tree_k")
    im = make_image(3, SW, SH)
    h = handle(model)
    set_threshold([h], im)
    q = capi.QpCache(h, 256, CPOS, CNEG)
    q.mine(im, 1)                                        # (a cache that holds examples and solver state)
    h.enqueue(im)
    refused(q, im, capi.PBD_ERR_STATE, "a frame pending")
    h.collect(capacity=MAXC)
    good_mine_equals_host_route(h, q, im, {})
    h.set_depth_filter(True)
    refused(q, im, capi.PBD_ERR_UNSUPPORTED, "depth pruning on")
    h.set_depth_filter(False)
    good_mine_equals_host_route(h, q, im, {})
    h.set_part_scores(True)
    refused(q, im, capi.PBD_ERR_UNSUPPORTED, "part scores on")
    h.set_part_scores(False)
    good_mine_equals_host_route(h, q, im, {})
    h.close()
    c = handle(model, dp_mode=2)                         # the compact memory plan, on every frame: no mine of this handle is accepted
    c.set_threshold(1e9)
    qc = capi.QpCache(c, CAP, CPOS, CNEG)
    err = refused(qc, im, capi.PBD_ERR_UNSUPPORTED, "compact plan")
    assert "compact" in str(err)
    assert len(c.detect(im)[0]) == 0                     # nothing pending: the handle takes a plain detect
    c.close()


# ---- 8. the C++ host layer -----------------------------------------------------------------------------------------------------------
def test_cpp_demo_mines(gpu_required, tmp_path):
    """host/demo.cpp --mine FILE... (pbd::ExampleCache::mineNegatives): the triples are the binding's for the same frames"""
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "host", "pbd_demo")
    assert os.path.exists(exe), "build() did not produce the C++ demo"
    model = make_model("tree_k")
    ims = [make_image(s, SW, SH) for s in (3, 4, 5)]
    det = PartsBasedDetector(device=0, conv_mode=capi.PBD_CONV_EXACT)
    det.distributeModel(model)
    set_threshold([det.handle], ims[0])
    model.thresh = det.handle.threshold
    model.save(str(tmp_path / "model.bin"))
    args = [exe, str(tmp_path / "model.bin"), str(tmp_path / "f0.raw"), str(SW), str(SH), "3"]
    for i, im in enumerate(ims):
        im.tofile(str(tmp_path / f"f{i}.raw"))
        args += ["--mine", str(tmp_path / f"f{i}.raw")]
    out = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    q = capi.QpCache(det.handle, 256, 1.0, 1.0)
    want = det.mineNegatives(ims, q)
    lines = [l for l in out.stdout.splitlines() if l.startswith("Mine ")]
    assert lines == [f"Mine {i}: records {r} written {w} action {a}" for i, (r, w, a) in enumerate(want)], out.stdout
    assert f"Cache: {q.dims()[3]} of 256 examples, ub {'%.17g' % q.state()[3][3]}" in out.stdout
    det.handle.close()
