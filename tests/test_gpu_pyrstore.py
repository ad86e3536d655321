"""The pyramid store on the device (include/pbd_c.h "pyramid store"; k_pyrstore.hip, pbd_pyrstore.cpp): a frame detected, batched,
mined and trained on from a stored feature pyramid against the same handle's image entry with the image that was put.  Every
comparison is bit equality — the store holds the very elements k_hog wrote, and everything behind the front end is the plain frame's
code — so no tolerance appears anywhere in this file."""
import copy
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import init_model, make_image
from partsbaseddetector_amd.train import train, train_model
from tests.test_gpu_train import (KS, PARENTS, latent_items, make_model, root_percentile, same, same_caches, synthetic, twins, with_interval)

pytestmark = pytest.mark.gpu

MAXC = 4096
SMALL, ODD = (64, 48), (97, 75)                             # (w, h): a multiple of the cell size, and no multiple of anything
MIN_RECORDS = 20
KIND_NAMES = {capi.PBD_PYRAMID_OPENCV: "cv", capi.PBD_PYRAMID_MATLAB: "matlab"}


def tree():
    """the small tree model of tests/test_gpu_train.py: four parts, 1 + 3 + 2 + 2 mixtures"""
    return make_model("tree_k")


def one_filter(seed=7):
    """init_model's one-filter model of tests/test_gpu_train.py (5 x 5 cells, sbin 4), its zero filter given random weights so that a
    frame's records depend on its features"""
    m = init_model(None, None, 4, tsize=(5, 5))
    m.filtersw[0][:] = np.random.default_rng(seed).standard_normal(m.filtersw[0].shape).astype(np.float32) * 0.1
    return m


def new_handle(model, iv=10, dtype=np.float32, kind=capi.PBD_PYRAMID_OPENCV, pad=0, maxc=MAXC, **kw):
    h = capi.Handle(with_interval(model, iv), dtype=dtype, max_candidates=maxc, **kw)
    if kind != capi.PBD_PYRAMID_OPENCV:
        h.set_pyramid_kind(kind)
    if pad:
        h.set_boundary_pad(pad)
    return h


def frame(seed, wh):
    return make_image(seed, wh[0], wh[1])


def low_threshold(h, im, pct=80.0):
    """a threshold under which the frame has at least MIN_RECORDS records on this handle (a fifth of its root scores), set on it"""
    h.set_threshold(root_percentile(h, im, pct))


def planes(h, im, res):
    """what the issue compares beside the records: every level's feature plane and the records' feature vectors, as bytes"""
    n = h.geometry(im.shape[1], im.shape[0])["nlevels"]
    h._geo, h._cn = h.geometry(im.shape[1], im.shape[0]), 3
    blocks, windows = h.candidates_features(res[0], res[2])
    return [h.level_features(l).tobytes() for l in range(n)] + [blocks.tobytes(), windows.tobytes()]


# ---- 1. a stored detect is the plain detect, in bits -------------------------------------------------------------------------------------------
BANKS = [(np.float32, capi.PBD_CONV_EXACT), (np.float32, capi.PBD_CONV_MFMA), (np.float32, capi.PBD_CONV_SPLIT), (np.float32, capi.PBD_CONV_SPLIT_F16),
         (np.float64, capi.PBD_CONV_EXACT), (np.float64, capi.PBD_CONV_MFMA)]
BANK_NAMES = {capi.PBD_CONV_EXACT: "exact", capi.PBD_CONV_MFMA: "mfma", capi.PBD_CONV_SPLIT: "split", capi.PBD_CONV_SPLIT_F16: "split_f16"}


@pytest.mark.parametrize("dtype, bank", BANKS, ids=[f"{np.dtype(d).name}-{BANK_NAMES[b]}" for d, b in BANKS])
def test_stored_detect_equals_plain_detect(gpu_required, dtype, bank):
    ims = [frame(3, SMALL), frame(4, ODD)]
    for kind in (capi.PBD_PYRAMID_OPENCV, capi.PBD_PYRAMID_MATLAB):
        for pad in (0, 2):
            for iv in (2, 10):
                what = (KIND_NAMES[kind], pad, iv)
                prod = new_handle(one_filter(), iv, dtype, kind, pad, conv_mode=capi.PBD_CONV_EXACT)      # the producer: ANOTHER model, another bank
                cons = new_handle(tree(), iv, dtype, kind, pad, conv_mode=bank)
                assert cons.conv_mode == bank
                store = capi.PyramidStore(prod, 2, ODD[0], ODD[1])
                own = capi.PyramidStore(cons, 1, ODD[0], ODD[1])                                          # ... and the consumer as its own producer
                d = store.dims()
                assert (d["slots"], d["sbin"], d["interval"], d["kind"], d["pad"], d["scalar_bytes"]) == (2, 4, iv, kind, pad, np.dtype(dtype).itemsize)
                assert d["slot_bytes"] == capi.pyrstore_layout(ODD[0], ODD[1], 4, iv, kind, pad)[2] * np.dtype(dtype).itemsize
                for slot, im in enumerate(ims):
                    sf = store.put(slot, im)
                    assert (sf.slot, store.slot(slot)[:3]) == (slot, (im.shape[1], im.shape[0], 3))
                    low_threshold(cons, im)
                    want = cons.detect(im, capacity=MAXC)
                    assert MIN_RECORDS <= len(want[0]) < MAXC, (what, slot, len(want[0]))
                    want_planes = planes(cons, im, want)
                    got = cons.detect_stored(store, slot, capacity=MAXC)
                    assert same(got, want), (what, slot, "records")
                    st = cons.stage_state()
                    assert st == dict(pyramid=False, features=True, responses=True, dp=True), (what, st)
                    with pytest.raises(capi.PbdError) as e:                                              # the level images are not the frame's
                        cons.level_image(0)
                    assert e.value.code == capi.PBD_ERR_STATE
                    assert planes(cons, im, got) == want_planes, (what, slot, "feature planes / feature vectors")
                    assert same(cons.detect_stored(sf, None, capacity=MAXC), want)                        # a StoredFrame names the slot too
                    assert same(cons.detect(im, capacity=MAXC), want), (what, slot, "plain detect afterwards")
                own.put(0, ims[1])
                assert same(cons.detect_stored(own, 0, capacity=MAXC), want), (what, "own producer")
                assert same(cons.detect(ims[1], capacity=MAXC), want)
                own.close(); store.close(); prod.close(); cons.close()


# ---- 2. batches ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bank", [capi.PBD_CONV_EXACT, capi.PBD_CONV_SPLIT], ids=["exact", "split"])
def test_stored_batches_equal_image_batches(gpu_required, bank):
    ims = [frame(s, SMALL) for s in (3, 4, 5)]
    prod = new_handle(one_filter(), conv_mode=capi.PBD_CONV_EXACT)
    cons = new_handle(tree(), conv_mode=bank)
    store = capi.PyramidStore(prod, 3, *SMALL)
    stored = store.put_batch([0, 1, 2], ims)                                                              # one batch through the producer
    assert [s.slot for s in stored] == [0, 1, 2] and [s.slot for s in store.frames()] == [0, 1, 2]
    low_threshold(cons, ims[0])
    singles = [cons.detect(im, capacity=MAXC) for im in ims]
    assert all(len(s[0]) >= MIN_RECORDS for s in singles)
    for slots in ([2, 0, 2], [1]):                                                                        # unordered with a repeat; a batch of one
        want = cons.detect_batch([ims[i] for i in slots], capacity=MAXC)
        got = cons.detect_batch_stored(store, slots, capacity=MAXC)
        assert len(got) == len(slots) and all(same(g, w) and same(g, singles[i]) for g, w, i in zip(got, want, slots)), slots
    # the largest batch: 64 frames in one plan, every slot many times over (the hit list is one for the batch: keep it under max_candidates)
    cons.set_threshold(root_percentile(cons, ims[0], 95.0))
    slots = [i % 3 for i in range(64)]
    want = cons.detect_batch([ims[i] for i in slots], capacity=MAXC)
    got = cons.detect_batch_stored(store, slots, capacity=MAXC)
    assert len(got) == 64 and all(same(g, w) for g, w in zip(got, want)) and sum(len(g[0]) for g in got) >= 64 * 4
    # slots that hold frames of different sizes are no batch; neither are none or 65
    big = capi.PyramidStore(prod, 2, *ODD)
    big.put(0, ims[0]); big.put(1, frame(4, ODD))
    for bad, code in (([0, 1], capi.PBD_ERR_ARG), ([0] * 65, capi.PBD_ERR_ARG), ([0, 2], capi.PBD_ERR_ARG), ([-1], capi.PBD_ERR_ARG)):
        with pytest.raises(capi.PbdError) as e:
            cons.detect_batch_stored(big, bad, capacity=MAXC)
        assert e.value.code == code, bad
    assert same(cons.detect_batch([ims[0]], capacity=MAXC)[0], want[0])
    big.close(); store.close(); prod.close(); cons.close()


# ---- 3. a stored frame leaves the captured graph alone ---------------------------------------------------------------------------------------------
def test_stored_frames_leave_the_graph_alone(gpu_required):
    im, other = frame(3, ODD), frame(4, ODD)
    prod = new_handle(one_filter())
    cons = new_handle(tree(), graph=1)
    store = capi.PyramidStore(prod, 1, *ODD)
    store.put(0, other)
    low_threshold(cons, im)
    first = cons.detect(im, capacity=MAXC)
    for _ in range(2):                                                                                    # eager, captured, replayed
        assert same(cons.detect(im, capacity=MAXC), first)
    want_other = None
    for _ in range(2):
        got = cons.detect_stored(store, 0, capacity=MAXC)
        want_other = want_other or got
        assert same(got, want_other) and len(got[0]) >= MIN_RECORDS and not same(got, first)
    with pytest.raises(capi.PbdError):
        cons.level_image(0)
    last = cons.detect(im, capacity=MAXC)                                                                 # the replayed graph again
    assert same(last, first)
    cons._geo, cons._cn = cons.geometry(*ODD), 3
    assert cons.level_image(0).shape == (ODD[1], ODD[0], 3) and cons.stage_state()["pyramid"]
    assert same(cons.detect(other, capacity=MAXC), want_other)
    store.close(); prod.close(); cons.close()


# ---- 4. the life of a slot -------------------------------------------------------------------------------------------------------------------------
def test_slot_lifecycle(gpu_required):
    a, b, odd = frame(3, SMALL), frame(4, SMALL), frame(5, ODD)
    prod = new_handle(one_filter())
    cons = new_handle(tree())
    low_threshold(cons, a)
    want_a, want_b = cons.detect(a, capacity=MAXC), cons.detect(b, capacity=MAXC)
    small = capi.PyramidStore(prod, 2, *SMALL)
    assert small.slot(0) == (0, 0, 0, 0) and small.frames() == []
    with pytest.raises(capi.PbdError) as e:                                                               # an empty slot
        cons.detect_stored(small, 0)
    assert e.value.code == capi.PBD_ERR_STATE and "empty" in str(e.value)
    small.put(0, a)
    assert same(cons.detect_stored(small, 0, capacity=MAXC), want_a)
    small.put(0, b)                                                                                       # a put overwrites
    assert same(cons.detect_stored(small, 0, capacity=MAXC), want_b) and not same(want_a, want_b)
    with pytest.raises(capi.PbdError) as e:                                                               # a frame over max_w x max_h
        small.put(0, odd)
    assert e.value.code == capi.PBD_ERR_CAPACITY and "exceeds the slot" in str(e.value)
    assert small.slot(0)[:2] == SMALL and same(cons.detect_stored(small, 0, capacity=MAXC), want_b)       # ... the old content is still there
    for bad in (-1, 2):
        with pytest.raises(capi.PbdError) as e:
            small.put(bad, a)
        assert e.value.code == capi.PBD_ERR_ARG
        with pytest.raises(capi.PbdError) as e:
            cons.detect_stored(small, bad)
        assert e.value.code == capi.PBD_ERR_ARG
    big = capi.PyramidStore(prod, 1, *ODD)                                                                # a smaller frame in a larger slot
    big.put(0, a)
    assert big.slot(0)[:3] == SMALL + (3,) and same(cons.detect_stored(big, 0, capacity=MAXC), want_a)
    big.put(0, odd)
    low_threshold(cons, odd)
    assert same(cons.detect_stored(big, 0, capacity=MAXC), cons.detect(odd, capacity=MAXC))
    # a slot's levels are the producer's feature planes of the frame; pbd_pyrstore_layout's offsets are where they start
    prod.pyramid(odd)
    n = big.slot(0)[3]
    assert n == prod._geo["nlevels"] == capi.pyrstore_layout(ODD[0], ODD[1], 4, 10)[0]
    for l in range(n):
        lv = big.level(0, l)
        assert lv.shape == prod.level_features(l).shape and lv.tobytes() == prod.level_features(l).tobytes(), l
    with pytest.raises(capi.PbdError) as e:
        big.level(0, n)
    assert e.value.code == capi.PBD_ERR_ARG
    # a frame pending on the producer refuses a put; one pending on the consumer refuses a stored detect
    prod.enqueue(a)
    with pytest.raises(capi.PbdError) as e:
        big.put(0, a)
    assert e.value.code == capi.PBD_ERR_STATE
    prod.collect()
    cons.enqueue(odd)
    with pytest.raises(capi.PbdError) as e:
        cons.detect_stored(big, 0)
    assert e.value.code == capi.PBD_ERR_STATE
    pending = cons.collect(capacity=MAXC)
    assert same(pending, cons.detect_stored(big, 0, capacity=MAXC))
    big.close(); small.close(); prod.close(); cons.close()


# ---- 5. signature refusals ------------------------------------------------------------------------------------------------------------------------
def test_signature_refusals_change_nothing(gpu_required):
    im = frame(3, ODD)
    prod = new_handle(one_filter())
    store = capi.PyramidStore(prod, 1, *ODD)
    store.put(0, im)
    sbin8 = copy.copy(tree()); sbin8._keep = []; sbin8.sbin = 8
    big = make_image(5, 200, 150)                                                                         # (a frame an sbin-8 handle can plan)
    cases = {"interval": (new_handle(tree(), 5), im), "sbin": (capi.Handle(sbin8, max_candidates=MAXC), big),
             "kind": (new_handle(tree(), kind=capi.PBD_PYRAMID_MATLAB), im), "pad": (new_handle(tree(), pad=2), im),
             "scalar": (new_handle(tree(), dtype=np.float64), im)}
    for field, (h, own) in cases.items():
        low_threshold(h, own)
        want = h.detect(own, capacity=MAXC)
        with pytest.raises(capi.PbdError) as e:
            h.detect_stored(store, 0)
        assert e.value.code == capi.PBD_ERR_ARG and field in str(e.value) and "store has" in str(e.value), (field, str(e.value))
        assert same(h.detect(own, capacity=MAXC), want), field
        h.close()
    # the signature is read at the time of the call: set_interval away and back
    cons = new_handle(tree(), graph=1)
    low_threshold(cons, im)
    want = cons.detect(im, capacity=MAXC)
    assert same(cons.detect_stored(store, 0, capacity=MAXC), want)
    cons.set_interval(3)
    with pytest.raises(capi.PbdError) as e:
        cons.detect_stored(store, 0)
    assert e.value.code == capi.PBD_ERR_ARG and "interval" in str(e.value) and "10" in str(e.value) and "3" in str(e.value)
    cons.set_interval(10)
    assert same(cons.detect_stored(store, 0, capacity=MAXC), want) and same(cons.detect(im, capacity=MAXC), want)
    # the producer's interval moved: a put is refused and the slot keeps its frame
    prod.set_interval(2)
    with pytest.raises(capi.PbdError) as e:
        store.put(0, frame(4, ODD))
    assert e.value.code == capi.PBD_ERR_STATE and "interval" in str(e.value)
    assert same(cons.detect_stored(store, 0, capacity=MAXC), want)
    prod.set_interval(10)
    store.put(0, frame(4, ODD))
    assert same(cons.detect_stored(store, 0, capacity=MAXC), cons.detect(frame(4, ODD), capacity=MAXC))
    # depth stages on the consumer
    cons.set_depth_filter(True)
    with pytest.raises(capi.PbdError) as e:
        cons.detect_stored(store, 0)
    assert e.value.code == capi.PBD_ERR_UNSUPPORTED
    cons.set_depth_filter(False)
    assert same(cons.detect(im, capacity=MAXC), want)
    store.close(); prod.close(); cons.close()


# ---- 6. mining ---------------------------------------------------------------------------------------------------------------------------------------
CPOS, CNEG = 0.004, 0.002


def mining_twins(model, capacity, maxc=MAXC, **kw):
    out = []
    for _ in range(2):
        h = new_handle(model, maxc=maxc, **kw)
        out.append((h, capi.QpCache(h, capacity, CPOS, CNEG)))
    return out


@pytest.mark.parametrize("which", ["tree", "one_filter"])
def test_mine_stored_equals_mine(gpu_required, which):
    model = tree() if which == "tree" else one_filter()
    ims = [frame(s, ODD) for s in (3, 4, 5)]
    prod = new_handle(one_filter(11) if which == "tree" else tree())
    store = capi.PyramidStore(prod, 3, *ODD)
    for i, im in enumerate(ims):
        store.put(i, im)
    (h, q), (g, t) = mining_twins(model, 4096)
    thr = root_percentile(g, ims[0], 90.0)
    h.set_threshold(thr); g.set_threshold(thr)
    r1, r2 = len(g.detect(ims[0], capacity=MAXC)[0]), len(g.detect(ims[1], capacity=MAXC)[0])
    assert r1 >= MIN_RECORDS and r2 >= MIN_RECORDS
    q.close(); t.close()
    # a cache that fills in the middle of the second frame; the third finds it full
    cap = r1 + r2 // 2
    q, t = capi.QpCache(h, cap, CPOS, CNEG), capi.QpCache(g, cap, CPOS, CNEG)
    for i, im in enumerate(ims):
        got, want = q.mine_stored(store, i, 7 + i), t.mine(im, 7 + i)
        assert got == want, (i, got, want)
        same_caches(q, t, f"frame {i}")
    assert q.dims()[3] == cap and want[1] == 0 and want[0] > 0
    assert h.stage_state() == dict(pyramid=False, features=True, responses=True, dp=True)
    # the batch entry on the same slots, repeated and out of order
    q2, t2 = capi.QpCache(h, 4096, CPOS, CNEG), capi.QpCache(g, 4096, CPOS, CNEG)
    got, want = q2.mine_batch_stored(store, [2, 0, 2], [5, 6, 7]), t2.mine_batch([ims[2], ims[0], ims[2]], [5, 6, 7])
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2] == want[2] and got[0].min() >= MIN_RECORDS
    same_caches(q2, t2, "batch")
    got, want = q2.mine_stored(capi.StoredFrame(store, 1), None, 9), t2.mine(ims[1], 9)                   # behind examples, a StoredFrame
    assert got == want
    same_caches(q2, t2, "single behind a batch")
    for c in (q, t, q2, t2):
        c.close()
    h.close(); g.close(); store.close(); prod.close()


def test_mine_stored_refusals_are_mines(gpu_required):
    model = tree()
    im = frame(3, ODD)
    prod = new_handle(one_filter())
    store = capi.PyramidStore(prod, 2, *ODD)
    store.put(0, im)
    # max_candidates overflow: the same code, the same needed count in records[0], nothing written
    (h, q), (g, t) = mining_twins(model, 64, maxc=8)
    full = new_handle(model)
    thr = root_percentile(full, im, 80.0)
    need = None
    for hh in (h, g):
        hh.set_threshold(thr)
    errs = []
    for call in (lambda: q.mine_stored(store, 0, 1), lambda: t.mine(im, 1)):
        with pytest.raises(capi.PbdError) as e:
            call()
        assert e.value.code == capi.PBD_ERR_CAPACITY
        errs.append(e.value)
    assert errs[0].records == errs[1].records and errs[0].records[0] > 8 and str(errs[0]) == str(errs[1])
    same_caches(q, t, "after the overflow")
    full.pyramid(im); full.pdf(); full.dp_min()
    roots = np.sort(np.concatenate([full.root(l, 0)[0].ravel() for l in range(full._geo["nlevels"])]))
    thr_hi = float(np.float32(roots[np.isfinite(roots)][-6]))                                             # at most five records: the handle still mines
    for hh in (h, g):
        hh.set_threshold(thr_hi)
    assert q.mine_stored(store, 0, 2) == t.mine(im, 2)
    same_caches(q, t, "after the overflow, mined")
    # an empty slot, a pending frame
    with pytest.raises(capi.PbdError) as e:
        q.mine_stored(store, 1, 3)
    assert e.value.code == capi.PBD_ERR_STATE
    h.enqueue(im)
    with pytest.raises(capi.PbdError) as e:
        q.mine_stored(store, 0, 3)
    assert e.value.code == capi.PBD_ERR_STATE
    h.collect()
    same_caches(q, t, "after the refusals")
    # the compact plan
    c = new_handle(model, dp_mode=2)
    c.set_threshold(1e9)
    qc = capi.QpCache(c, 64, CPOS, CNEG)
    for call in (lambda: qc.mine_stored(store, 0, 1), lambda: c.detect_stored(store, 0)):
        with pytest.raises(capi.PbdError) as e:
            call()
        assert e.value.code == capi.PBD_ERR_UNSUPPORTED and "compact" in str(e.value)
    assert len(c.detect(im)[0]) == 0
    cp = capi.PyramidStore(c, 1, *ODD)                                                                     # ... as a producer too
    with pytest.raises(capi.PbdError) as e:
        cp.put(0, im)
    assert e.value.code == capi.PBD_ERR_UNSUPPORTED and cp.slot(0)[0] == 0
    cp.close()
    # pbd_group members: neither producers nor consumers
    grp = capi.Group(model, [0])
    member = C.c_void_p(grp.L.pbd_group_member(grp.g, 0))
    before = grp.detect(im)
    cnt, out = C.c_int(-1), C.c_void_p()
    heads = np.zeros(MAXC, capi.HEAD_DTYPE)
    assert grp.L.pbd_detect_stored(member, store.s, 0, heads.ctypes.data_as(C.c_void_p), None, None, MAXC, C.byref(cnt)) == capi.PBD_ERR_UNSUPPORTED
    assert grp.L.pbd_pyrstore_create(member, 1, ODD[0], ODD[1], C.byref(out)) == capi.PBD_ERR_UNSUPPORTED and not out.value
    assert same(grp.detect(im), before)
    grp.close()
    for x in (q, t, qc):
        x.close()
    for x in (store,):
        x.close()
    for x in (h, g, c, full, prod):
        x.close()


# ---- 7. training ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_train_with_stored_negatives_equals_train_with_images(gpu_required, dtype):
    model = tree()
    positives = latent_items(model, dtype)
    negatives = [make_image(s, 100, 80) for s in (11, 12)]
    ta, tb = twins(model, dtype)
    prod = new_handle(one_filter(), 2, dtype)                                                             # train() mines at interval 2
    store = capi.PyramidStore(prod, 2, 100, 80)
    stored = [store.put(i, im) for i, im in enumerate(negatives)]
    ma, ra = train(None, positives, stored, 0, overlap=0.6, max_iter=200, seed=3, detector=ta[0], cache=ta[1])
    mb, rb = train(None, positives, negatives, 0, overlap=0.6, max_iter=200, seed=3, detector=tb[0], cache=tb[1])
    assert ra == rb and len(ra) == 1 and sum(w for _, w, _ in ra[0]["mined"]) > 0
    same_caches(ta[1], tb[1], "train() on stored negatives")
    assert ta[0].handle.weights().tobytes() == tb[0].handle.weights().tobytes()
    assert np.float32(ta[0].handle.threshold).tobytes() == np.float32(tb[0].handle.threshold).tobytes()
    assert ta[0].handle.interval == tb[0].handle.interval == 10 == ma.interval and ma.thresh == mb.thresh
    # a mixed list: an image still goes where it goes today
    for d in (ta[0], tb[0]):                                                                              # (the store's interval again, as train() mines)
        d.setInterval(2)
        d.setThresh(-1)
    mixed = ta[0].mineNegatives([negatives[0], stored[1]], ta[1], 1)
    plain = tb[0].mineNegatives(negatives, tb[1], 1)
    assert mixed == plain
    same_caches(ta[1], tb[1], "a mixed list")
    store.close(); prod.close()
    for d, _ in (ta, tb):
        d.handle.close()


def test_train_model_with_shared_pyramids_equals_train_model(gpu_required):
    positives, negatives = synthetic()
    kw = dict(tsize=(5, 5), R=4, max_iter=200, conv_mode=capi.PBD_CONV_EXACT, max_candidates=MAXC)
    shared, rs = train_model(positives, negatives, KS, PARENTS, 4, share_pyramids=True, **kw)
    plain, rp = train_model(positives, negatives, KS, PARENTS, 4, **kw)
    assert shared.weight_vector().tobytes() == plain.weight_vector().tobytes() and np.abs(plain.weight_vector()).max() > 0
    assert shared.thresh == plain.thresh and shared.interval == plain.interval == 10
    assert rs["idx"].tolist() == rp["idx"].tolist() and rs["final"] == rp["final"] and rs["final1"] == rp["final1"] and rs["parts"] == rp["parts"]
    assert all(sum(w for _, w, _ in rep[0]["mined"]) > 0 for rep in (rp["final"], rp["final1"]))
