"""Hard-negative mining (k_qp_mine.hip, k_qp.hip's write through perm) at record counts past one trip of its loops: k_qp_mine_rank's
tiles of 256 keys (a second tile, the padding of the last one, ranks across tiles), k_qp_mine_scan's 256-strided validation, its
four-loads block sum (from 193 records on), the per-frame binary search of a RAW batch, the perm of filtered records beyond one stride.

One 100 x 80 frame of the small tree has a record per finite root cell (2757 on the oracle), so a threshold at the handle's own
(n + 1)-th largest root score reaches every count n.  Every comparison is in bits: the ids rows against the order BY DEFINITION (an
np.lexsort made here, not an order some entry of the library returned), the columns against the host route on a twin and against
tests/qp_ref.py's write of the handle's own feature vectors, ub against tests/mine_ref.py's block sum."""
import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_tree_model_k
from tests import mine_ref
from tests.test_gpu_mine import CNEG, CPOS, RAW, SORT, SH, SW, host_route, refused, root_scores, same_caches
from tests.test_gpu_qp import expect

pytestmark = pytest.mark.gpu

MAXC = 8192
ALL = "all"


def tree():
    return make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21)


def handle(model, dtype=np.float32, mode=RAW):
    return capi.Handle(model, dtype=dtype, max_candidates=MAXC, cand_filter=mode)


def cut(vals, n):
    """vals: the finite root scores, ascending, the handle's own values held in float64 -> the float32 threshold above which exactly n of them lie
    under the detect rule (double)score > (double)thresh (src k_root, :208 strict): the (n + 1)-th largest score, rounded UP to float32
    for a double handle; the scores next to the cut are distinct"""
    if n == len(vals):
        return -1e30
    assert 0 < n < len(vals)
    below, above = vals[-(n + 1)], vals[-n]
    t = np.float32(below)
    if np.float64(t) < below:
        t = np.nextafter(t, np.float32(np.inf))
    assert below <= np.float64(t) < above, (n, below, t, above)
    return float(t)


def by_definition(heads, locs, mode):
    """the records' order: (level, component, root y, root x); with the sort filter (score descending, then that key)"""
    keys = [locs[:, 0, 0], locs[:, 0, 1], heads["component"], heads["level"]]
    if mode is not RAW:
        keys.append(-heads["score"].astype(np.float64))
    return np.lexsort(keys)


def sampled(n):
    """every position up to 257 records; beyond, the positions next to the tiles' and strides' edges"""
    if n <= 257:
        return list(range(n))
    at = [0, 63, 64, 191, 192, 193, 255, 256, 257, 1023, 1024, 1025, n - 1]
    return sorted({i for i in at if i < n})


def centred(handles, im, n):
    """the root bias moved so that the middle of the n best root scores sits at -1 (terms 1 + score on both sides of zero), then the
    threshold that keeps n records -> (n, the threshold); n = ALL: every finite root"""
    g = handles[0]
    vals = root_scores(g, im)
    m = len(vals) if n == ALL else n
    shift = -1.0 - float(vals[-(m // 2)])
    w = g.weights()
    w[g.model.biasid[0][0][0]] += shift
    for x in handles:
        x.set_weights(w)
    vals = root_scores(g, im)                            # (the new weights' scores: the shift is rounded into every one of them)
    t = cut(vals, m)
    for x in handles:
        x.set_threshold(t)
    return m, t


COUNTS = [(n, np.float32, "raw") for n in (192, 193, 255, 256, 257, 1024, 1025, ALL)] + \
         [(n, d, m) for n in (257, 1025) for d, m in ((np.float64, "raw"), (np.float32, "sort"), (np.float64, "sort"))]


@pytest.mark.parametrize("n, dtype, filt", COUNTS, ids=[f"{n}-{np.dtype(d).name}-{m}" for n, d, m in COUNTS])
def test_counts_past_the_tiles(gpu_required, n, dtype, filt):
    mode = RAW if filt == "raw" else SORT
    model = tree()
    im = make_image(3, SW, SH)
    h, g = handle(model, dtype, mode), handle(model, dtype, mode)
    n, thr = centred([g, h], im, n)
    heads, _, locs = g.detect(im, capacity=MAXC)
    print(f"records reached: {len(heads)} (threshold {thr!r})")
    assert len(heads) == n                               # the plain detect returns exactly the count asked for
    if filt == "raw" and dtype == np.float32:
        assert n in (192, 193, 255, 256, 257, 1024, 1025) or n > 2048
    sc = heads["score"]
    assert (sc < -1).any() and (sc > -1).any()
    order = by_definition(heads, locs, mode)
    heads_d, locs_d = heads[order], locs[order]
    cap = n + 7
    q, t = capi.QpCache(h, cap, CPOS, CNEG), capi.QpCache(g, cap, CPOS, CNEG)
    rec, wr, act = q.mine(im, 5)
    assert (rec, wr) == (n, min(n, cap))
    got = q.get(0, cap)
    # ids: by definition
    want_ids = np.zeros((cap, 5), np.int32)
    want_ids[:n] = np.stack([np.full(n, -1), np.full(n, 5), heads_d["level"], locs_d[:, 0, 0], locs_d[:, 0, 1]], axis=1)
    assert got[1].tobytes() == want_ids.tobytes(), np.argwhere(got[1] != want_ids)[:5]
    # the host route on the twin, every column of the capacity
    assert host_route(g, t, im, 5)[:2] == (n, n)
    t.state()
    for name, a, b in zip(("x", "ids", "b", "d"), got, t.get(0, cap)):
        assert a.tobytes() == b.tobytes(), (name, np.argwhere(a != b)[:5])
    # the definition of the write over the handle's own feature vectors, records in the order by definition
    at = sampled(n)
    exp = expect(h, h.model, heads_d[at], locs_d[at], -1, 5, q.dims()[1])
    for name, a, e in zip(("x", "ids", "b", "d"), got, exp):
        assert a[at].tobytes() == e.tobytes(), (name, [at[i] for i in np.flatnonzero((a[at] != e).reshape(len(at), -1).any(axis=1))][:5])
    # ub: the block sum of the terms in record order
    st = q.state()[3]
    assert st[3].tobytes() == np.float64(mine_ref.ub_term_sum(heads_d["score"], CNEG)).tobytes()
    assert act == mine_ref.action(st[1], st[3], q.dims()[3], cap)
    h.close(); g.close()


@pytest.mark.parametrize("filt", ["raw", "sort"])
def test_capacity_cut_inside_a_later_tile(gpu_required, filt):
    """1025 records into a cache that holds 7 examples and has room for 300: the cut falls inside the second tile of 256"""
    mode = RAW if filt == "raw" else SORT
    model = tree()
    im = make_image(3, SW, SH)
    h, g = handle(model, mode=mode), handle(model, mode=mode)
    n, thr = centred([g, h], im, 1025)
    vals = root_scores(g, im)
    cap = 307
    q, t = capi.QpCache(h, cap, CPOS, CNEG), capi.QpCache(g, cap, CPOS, CNEG)
    for x in (h, g):
        x.set_threshold(cut(vals, 7))
    assert q.mine(im, 1)[:2] == (7, 7) and t.mine(im, 1)[:2] == (7, 7)
    ub7 = q.state()[3][3]
    front = [v.tobytes() for v in q.get(0, 7)]
    for x in (h, g):
        x.set_threshold(thr)
    heads, _, locs = g.detect(im, capacity=MAXC)
    assert len(heads) == 1025
    order = by_definition(heads, locs, mode)
    rec, wr, act = q.mine(im, 2)
    print(f"records {rec}, written {wr}")
    assert (rec, wr, act) == (1025, 300, capi.PBD_MINE_OPT) and q.dims()[3] == cap
    assert host_route(g, t, im, 2)[:2] == (1025, 300)
    t.state()
    got = q.get(0, cap)
    for name, a, b in zip(("x", "ids", "b", "d"), got, t.get(0, cap)):
        assert a.tobytes() == b.tobytes(), (name, np.argwhere(a != b)[:5])
    assert [v.tobytes() for v in q.get(0, 7)] == front    # the examples in front stay
    lv, x0, y0 = heads["level"][order][:300], locs[order][:300, 0, 0], locs[order][:300, 0, 1]
    assert got[1][7:].tobytes() == np.stack([np.full(300, -1), np.full(300, 2), lv, x0, y0], axis=1).astype(np.int32).tobytes()
    # ub holds every record's term, the 725 refused ones' too
    S = mine_ref.ub_term_sum(heads["score"][order], CNEG)
    assert q.state()[3][3].tobytes() == np.float64(ub7 + S).tobytes()
    h.close(); g.close()


# ---- the first refused record far down the list ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lowered, least", [(True, 1024), (False, 256)], ids=["one-bad-record", "many-bad-records"])
def test_first_refused_record_far_down_the_list(gpu_required, lowered, least):
    """parts 1 and 2 share a filter in their mixture 1: a record whose pose picks both is refused.  The first such record of 2000 lies
    behind the scan's first trips (with the shared mixture's bias lowered it is the only one, behind position 1024): the smallest bad
    position over all threads and trips is the one named"""
    model = make_tree_model_k([-1, 0, 0], [1, 2, 2], seed=8)
    model.filterid[0][2][1] = model.filterid[0][1][1]
    if lowered:
        model.biasw = np.array(model.biasw, np.float32)
        model.biasw[model.biasid[0][2][1]] -= np.float32(0.5)
    im = make_image(3, SW, SH)
    h, g = handle(model), handle(model)
    vals = root_scores(g, im)
    thr = cut(vals, 2000)
    for x in (h, g):
        x.set_threshold(thr)
    heads, _, locs = g.detect(im, capacity=MAXC)
    assert len(heads) == 2000
    order = by_definition(heads, locs, RAW)
    assert (order == np.arange(2000)).all()              # the plain detect's RAW order is the order by definition
    both = (locs[:, 1, 2] == 1) & (locs[:, 2, 2] == 1)
    first = int(np.argmax(both))
    print(f"records 2000, {int(both.sum())} pick both shared mixtures, the first at position {first}")
    assert both.any() and first >= least
    q, t = capi.QpCache(h, 64, CPOS, CNEG), capi.QpCache(g, 64, CPOS, CNEG)
    with pytest.raises(capi.PbdError) as e:              # the host route refuses the same records
        t.write(heads, locs, -1, 9)
    assert e.value.code == capi.PBD_ERR_ARG
    err = refused(q, im, capi.PBD_ERR_ARG, "a pose picks the shared mixtures")
    assert f"record {first} of frame 0" in str(err) and "qp_write.m:34-35" in str(err)
    h.close(); g.close()


# ---- a batch of three frames --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ["raw", "sort"])
def test_batch_of_three_frames(gpu_required, filt):
    """[a frame, a black frame, a frame] at the black frame's largest root score: about 2000 / 0 / 2000 records; the frames' spans in a
    RAW batch come from a binary search over the ranked records' (virtual) levels"""
    mode = RAW if filt == "raw" else SORT
    model = tree()
    ims = [make_image(3, SW, SH), np.zeros((SH, SW, 3), np.uint8), make_image(4, SW, SH)]
    h, g = handle(model, mode=mode), handle(model, mode=mode)
    thr = float(np.float32(root_scores(g, ims[1])[-1]))
    for x in (h, g):
        x.set_threshold(thr)
    plain = [g.detect(im, capacity=MAXC) for im in ims]
    counts = [len(p[0]) for p in plain]
    print("records per frame", counts)
    assert counts[0] > 256 and counts[1] == 0 and counts[2] > 256
    for cap in (sum(counts) + 7, counts[0] + counts[2] // 2):      # room for all; room that ends inside the third frame
        q, t = capi.QpCache(h, cap, CPOS, CNEG), capi.QpCache(g, cap, CPOS, CNEG)
        one = [t.mine(im, 7 + i) for i, im in enumerate(ims)]
        rec, wr, act = q.mine_batch(ims, [7, 8, 9])
        room = [min(counts[0], cap), 0, min(counts[2], cap - min(counts[0], cap))]
        assert list(rec) == counts == [o[0] for o in one] and list(wr) == room == [o[1] for o in one] and act == one[-1][2]
        if cap < sum(counts):
            assert list(wr) == [counts[0], 0, counts[2] // 2]
        same_caches(q, t, f"capacity {cap}")
        ids = q.get()[1]
        want = []
        for f, (heads, _, locs) in enumerate(plain):     # the frame's id, the frame's own level, the root: in the order by definition
            o = by_definition(heads, locs, mode)[:room[f]]
            want.append(np.stack([np.full(len(o), -1), np.full(len(o), 7 + f), heads["level"][o], locs[o, 0, 0], locs[o, 0, 1]], axis=1))
        assert ids.tobytes() == np.concatenate(want).astype(np.int32).tobytes()
        q.close(); t.close()
    h.close(); g.close()
