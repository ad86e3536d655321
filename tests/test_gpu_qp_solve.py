"""The QP solver on the device (k_qp_solve.hip, pbd_qp_solve.cpp; include/pbd_c.h "QP solver") against tests/qp_solve_ref.py in the
library's order (block sums, complete dot), bit for bit: the pass after every pass of every case, refresh / loss / one / prune / opt,
the same at 77 blocks a column, 1200 ids and 1600 noneg entries (qp_solve_cases.LARGE_CASES), columns written by pbd_qp_write
(non-ascending blocks; the small tree's and the person model's 77), the state of appended examples, qp_w.m, and every refusal with the state
untouched.  tests/test_qp_solve_cpu.py ties the same restatement, summing left to right, to the compiled reference file; the two
orders meet again here through weak duality: each run's lower bound stays under the other's upper bound."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_mixed_person_model, make_tree_model_k
from tests import qp_ref
from tests import qp_solve_cases as sc
from tests import qp_solve_ref as sr

pytestmark = pytest.mark.gpu

MAXC = 4096
SW, SH = 100, 80
KEYS = ("loss", "a", "w", "sv", "l")


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, make in sc.CASES.items()}


@pytest.fixture(scope="module")
def large():
    return {name: make() for name, make in sc.LARGE_CASES.items()}


@pytest.fixture(scope="module")
def handle(gpu_required):
    h = capi.Handle(make_mixed_person_model(seed=5, K=2), max_candidates=MAXC)
    yield h
    h.close()


def padded(c, k):
    x = np.zeros((len(c["x"]), k), np.float32)
    x[:, :c["x"].shape[1]] = c["x"]
    return x


def load(h, c, capacity, junk=0):
    """a cache holding the case's examples, brought to the case's starting state by set_state and refresh; junk > 0: that many other
    examples are put between them first and removed by keep, so that example i is not column i"""
    q = capi.QpCache(h, capacity)
    length, k, _, _ = q.dims()
    x, n = padded(c, k), len(c["x"])
    if junk:
        rng = np.random.default_rng(junk)
        at = np.sort(rng.choice(n + junk, junk, replace=False))          # positions of the junk examples
        mask = np.ones(n + junk, bool)
        mask[at] = False
        allx = np.zeros((n + junk, k), np.float32)
        allx[mask], allx[~mask] = x, x[rng.integers(0, n, junk)]
        ids, b, d = (np.zeros((n + junk,) + v.shape[1:], v.dtype) for v in (c["ids"], c["b"], c["d"]))
        ids[mask], b[mask], d[mask] = c["ids"], c["b"], c["d"]
        q.put(allx, ids, b, d)
        q.keep(np.flatnonzero(mask))
    else:
        q.put(x, c["ids"], c["b"], c["d"])
    assert q.dims()[3] == n
    q.noneg(c["noneg"])
    sv = np.zeros(capacity, np.uint8)
    sv[:n] = 1
    a = np.zeros(capacity)
    a[:n] = c["a"]
    q.set_state(a, sv)
    q.refresh()
    ga, gsv, gw, gst = q.state()
    assert gw[:len(c["w"])].tobytes() == c["w"].tobytes() and not gw[len(c["w"]):].any() and gst[0] == c["l"]
    return q


def check(q, want, what):
    a, sv, w, st = q.state()
    got = dict(a=a, sv=sv, w=w, l=np.array([st[0]]))
    for key in ("a", "sv", "w", "l"):
        assert got[key].tobytes() == want[key].tobytes(), (what, key, np.argwhere(got[key] != want[key])[:5])


def run_case(h, c, capacity, junk=0, reload=False):
    q = load(h, c, capacity, junk)
    length = q.dims()[0]
    want, _ = sr.run_passes(c, "strided", "complete", capacity, length)
    for p in range(c["passes"]):
        order = sc.next_order(c, p, q.state()[1])
        assert order.tobytes() == want[p]["order"].tobytes()
        loss = q.solve_pass(order)
        assert np.array([loss]).tobytes() == want[p]["loss"].tobytes(), (p, loss, want[p]["loss"])
        check(q, want[p], (capacity, junk, reload, p))
        if reload:
            a, sv, _, _ = q.state()
            q.set_state(a, sv)
    out = q.state()
    q.close()
    return out


# ---- 1. the pass -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["free", "binding"])
def test_pass_equals_the_restatement(handle, cases, name):
    c = cases[name]
    first = run_case(handle, c, 128)
    again = run_case(handle, c, 128)                                          # two runs are identical
    for u, v in zip(first, again):
        assert u.tobytes() == v.tobytes()


# ---- 2. invariance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,junk,reload", [(160, 23, False), (301, 0, False), (128, 0, True)])
def test_pass_is_invariant(handle, cases, capacity, junk, reload):
    """other columns (examples removed by keep first), another capacity, the state reloaded between passes: run_case compares with
    the same restatement every time"""
    run_case(handle, cases["binding"], capacity, junk, reload)


# ---- 3. refresh, loss, one, prune, opt ---------------------------------------------------------------------------------------------------
def test_one_loss_prune_and_opt_equal_the_restatement(handle, cases):
    one_loss_prune_and_opt(handle, cases["binding"], 128)


def one_loss_prune_and_opt(handle, c, cap, junk=0):
    n = len(c["x"])
    cache = (c["x"], c["ids"], c["b"], c["d"])
    q = load(handle, c, cap, junk)
    length = q.dims()[0]
    st = sr.start_state(c, cap, length)
    sr.refresh_ref(cache, st, "strided")              # (load's refresh)
    q.fix(3)
    st.nfix = 3

    def same(what):
        a, sv, w, stats = q.state()
        for g, e, key in ((a, st.a, "a"), (sv, st.sv, "sv"), (w, st.w, "w"), (stats, st.stats(), "l lb lb_old ub")):
            assert g.tobytes() == e.tobytes(), (what, key, g[:4], e[:4])
    same("refresh")
    for p in range(2):
        order = sc.next_order(c, p, st.sv)
        q.one(order)
        sr.one_ref(cache, st, order, "strided", "complete")
        same(("one", p))
        assert np.array([q.loss()]).tobytes() == np.array([sr.loss_ref(cache, st, n)]).tobytes()
    m = q.prune()
    pruned, m_ref = sr.prune_ref(cache, st, n, "strided")
    assert m == m_ref == q.dims()[3] and m < n
    same("prune")
    gx, gids, gb, gd = q.get()
    K = pruned[0].shape[1]
    assert gx[:, :K].tobytes() == pruned[0].tobytes() and not gx[:, K:].any()
    assert (gids.tobytes(), gb.tobytes(), gd.tobytes()) == tuple(v.tobytes() for v in pruned[1:])
    q.close()
    # qp_opt from a = 0
    q = capi.QpCache(handle, cap)
    q.put(padded(c, q.dims()[1]), c["ids"], c["b"], c["d"])
    q.noneg(c["noneg"])
    lb, ub, passes = q.opt(.05, 1000, 11)
    rlb, rub, rpasses, st = sr.opt_run(c, "strided", "complete", 11, .05, cap, length)
    assert (passes, np.array([lb, ub]).tobytes()) == (rpasses, np.array([rlb, rub]).tobytes()), (lb, ub, passes, rlb, rub, rpasses)
    assert 0 < passes < 1000 and 1 - lb / ub < .05
    same("opt")
    # weak duality against the run in the reference's order
    slb, sub, _, _ = sr.opt_run(c, "sequential", "merge", 11, .05)
    assert sub - lb > 1e-6 * sub and ub - slb > 1e-6 * ub                 # separated by far more than rounding: no slack needed
    assert lb <= sub and slb <= ub
    q.close()


# ---- 3b. beyond one trip of the kernels' loops: 77-block columns, 1200 ids, a noneg list of 1600 entries ---------------------------------
def test_manyblock_passes_one_loss_prune_and_opt(handle, large):
    """columns of 77 blocks (k_qp_pass's 16 wavefronts take five trips over them in the score, the axpy and the pair dot; k_qp_score and
    k_qp_lincomb walk them in loss, refresh, prune and opt), behind junk columns in a cache of another capacity"""
    c = large["manyblock"]
    _, cnt = sr.run_passes(c, "strided", "complete")
    print("manyblock counters", cnt)
    assert cnt["pair"] > 0 and cnt["single"] > 0 and cnt["clamp"] > 0
    assert {int(col[0]) for col in c["x"]} == {77}
    run_case(handle, c, 301, junk=23)
    one_loss_prune_and_opt(handle, c, 301, junk=23)


def test_manyids_passes_refresh_and_loss(handle, large):
    """1200 ids (the pass's loss is summed in chunks of 1024), a noneg list of 1600 entries (the clamp strides by the block size: 1024
    in the pass, 256 in refresh), 2400 examples in loss and refresh"""
    c = large["manyids"]
    n, cap = len(c["x"]), 2500
    cache = (c["x"], c["ids"], c["b"], c["d"])
    q = load(handle, c, cap)
    length = q.dims()[0]
    st, cnt = sr.start_state(c, cap, length), sr.new_counters()
    sr.refresh_ref(cache, st, "strided")              # (load's refresh: lb, which the refresh below moves to lb_old)
    for p in range(c["passes"]):
        order = sc.next_order(c, p, st.sv)
        rloss = sr.pass_ref(cache, st, order, "strided", "complete", cnt)
        loss = q.solve_pass(order)
        assert np.array([loss]).tobytes() == np.array([rloss]).tobytes(), (p, loss, rloss)
        check(q, dict(a=st.a, sv=st.sv, w=st.w, l=np.array([st.l])), ("manyids", p))
    print("manyids counters", cnt, "noneg", len(c["noneg"]))
    assert cnt["pair"] > 0 and cnt["single"] > 0 and cnt["clamp"] > 0 and cnt["err_past_1024"] > 0 and len(c["noneg"]) > 1024
    # a state in which refresh has entries to clamp behind the first 256 and 1024 of the list
    a = st.a.copy()
    a[:n] = np.random.default_rng(9).uniform(0, 1, n) * (np.arange(n) % 3 > 0)
    q.set_state(a, st.sv)
    st.a = a.copy()
    raw = qp_lincomb_sorted(cache, st)
    neg = raw[c["noneg"]] < 0
    assert neg[256:1024].any() and neg[1024:].any()
    q.refresh()
    sr.refresh_ref(cache, st, "strided")
    ga, gsv, gw, gst = q.state()
    assert gw.tobytes() == st.w.tobytes() and gst.tobytes() == st.stats().tobytes() and ga.tobytes() == st.a.tobytes()
    assert np.array([q.loss()]).tobytes() == np.array([sr.loss_ref(cache, st, n)]).tobytes()
    q.close()


def qp_lincomb_sorted(cache, st):
    """refresh's w before its clamp"""
    I = np.flatnonzero(st.a > 0)
    return qp_ref.lincomb_ref(cache[0], st.a, I[np.argsort(st.a[I], kind="stable")], len(st.w))


# ---- 4. columns written by pbd_qp_write --------------------------------------------------------------------------------------------------
def test_written_columns_two_passes_and_a_refresh(gpu_required):
    model = make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21)
    h = capi.Handle(model, max_candidates=MAXC)
    h.pyramid(make_image(3, SW, SH))
    g = h.geometry(SW, SH)
    rng = np.random.default_rng(4)
    level = 1
    cw, ch = int(g["cell_w"][level]), int(g["cell_h"][level])
    n = 12
    heads = np.zeros(n, capi.HEAD_DTYPE)
    locs = np.zeros((n, model.max_parts, 3), np.int32)
    roots = [(int(rng.integers(0, cw)), int(rng.integers(0, ch))) for _ in range(2)]
    for i in range(n):
        heads[i] = (0.0, 0, level, model.nparts(0))
        for p in range(model.nparts(0)):
            x, y = roots[i % 2] if p == 0 else (int(rng.integers(0, cw)), int(rng.integers(0, ch)))   # two roots: ids are shared
            locs[i, p] = (x, y, int(rng.integers(0, len(model.filterid[0][p]))))
    _, wreg, w0, noneg = model.qp_vectors()
    q = capi.QpCache(h, 32, 2e-5, 2e-5)
    assert q.write(heads[:6], locs[:6], 1, 7) == 6 and q.write(heads[6:], locs[6:], -1, 8) == 6
    q.noneg(noneg)
    cache = q.get()
    length, k, cap, _ = q.dims()
    starts = [[s for s, _, _ in sr.parse(col)] for col in cache[0]]
    assert any(s != sorted(s) for s in starts)                                # detect.m's block order is not ascending
    assert len(np.unique(cache[1], axis=0)) == 4                              # 2 labels x 2 roots: three examples per id
    st = sr.State(cap, length, n, noneg)
    cnt = sr.new_counters()
    for p in range(2):
        order = np.random.default_rng(p).permutation(n).astype(np.int32)
        loss = q.solve_pass(order)
        rloss = sr.pass_ref(cache, st, order, "strided", "complete", cnt)
        a, sv, w, stats = q.state()
        assert np.array([loss, stats[0]]).tobytes() == np.array([rloss, st.l]).tobytes(), (p, loss, rloss)
        assert a.tobytes() == st.a.tobytes() and sv.tobytes() == st.sv.tobytes() and w.tobytes() == st.w.tobytes(), p
    assert cnt["pair"] > 0, cnt                                               # the complete dot ran on non-ascending columns
    q.refresh()
    sr.refresh_ref(cache, st, "strided")
    a, sv, w, stats = q.state()
    assert w.tobytes() == st.w.tobytes() and stats.tobytes() == st.stats().tobytes()
    # examples written once the state exists start at a = 0, sv = 1; qp_w.m
    sv0 = np.zeros(cap, np.uint8)
    q.set_state(sv=sv0)
    assert q.write(heads[:3], locs[:3], -1, 9) == 3
    a, sv, _, _ = q.state()
    assert not a[n:].any() and sv[n:n + 3].all() and not sv[n + 3:].any() and not sv[:n].any()
    assert q.weights().tobytes() == (w / wreg + w0).tobytes()
    q.close()
    h.close()


def test_written_person_columns_two_passes_and_a_refresh(handle):
    """what pbd_qp_write makes of poses of the person model: columns of 3 * 26 - 1 = 77 blocks in detect.m's (non-ascending) order.  C is
    the restatement's choice: the largest of 2e-5, 1e-5, 5e-6, ... at which its two passes over the written columns run both the pair
    and the single branch (2e-5, the first, on an MI355X; the test prints the one it used with the counters)"""
    model, h = handle.model, handle
    h.pyramid(make_image(3, SW, SH))
    g = h.geometry(SW, SH)
    rng = np.random.default_rng(4)
    level = 1
    cw, ch = int(g["cell_w"][level]), int(g["cell_h"][level])
    n, np_ = 24, model.nparts(0)
    assert np_ == 26
    heads = np.zeros(n, capi.HEAD_DTYPE)
    locs = np.zeros((n, model.max_parts, 3), np.int32)
    roots = [(int(rng.integers(0, cw)), int(rng.integers(0, ch))) for _ in range(2)]
    for i in range(n):
        heads[i] = (0.0, 0, level, np_)
        for p in range(np_):
            x, y = roots[i % 2] if p == 0 else (int(rng.integers(0, cw)), int(rng.integers(0, ch)))   # two roots: ids are shared
            locs[i, p] = (x, y, int(rng.integers(0, len(model.filterid[0][p]))))
    _, wreg, w0, noneg = model.qp_vectors()
    orders = [np.random.default_rng(p).permutation(n).astype(np.int32) for p in range(2)]
    used = None
    for C in [2e-5 / 2 ** t for t in range(10)]:
        q = capi.QpCache(h, 32, C, C)
        assert q.write(heads[:12], locs[:12], 1, 7) == 12 and q.write(heads[12:], locs[12:], -1, 8) == 12
        q.noneg(noneg)
        cache = q.get()
        length, k, cap, _ = q.dims()
        st, cnt = sr.State(cap, length, n, noneg), sr.new_counters()
        for order in orders:
            sr.pass_ref(cache, st, order, "strided", "complete", cnt)
        if cnt["pair"] > 0 and cnt["single"] > 0:
            used = C
            break
        q.close()
    print("C used", used, "counters", cnt)
    assert used is not None, cnt
    assert (cache[0][:, 0] == 77).all() and len(np.unique(cache[1], axis=0)) == 4
    starts = [[s for s, _, _ in sr.parse(col)] for col in cache[0]]
    assert any(s != sorted(s) for s in starts)
    st = sr.State(cap, length, n, noneg)
    for p, order in enumerate(orders):
        loss = q.solve_pass(order)
        rloss = sr.pass_ref(cache, st, order, "strided", "complete")
        a, sv, w, stats = q.state()
        assert np.array([loss, stats[0]]).tobytes() == np.array([rloss, st.l]).tobytes(), (p, loss, rloss)
        assert a.tobytes() == st.a.tobytes() and sv.tobytes() == st.sv.tobytes() and w.tobytes() == st.w.tobytes(), p
    q.refresh()
    sr.refresh_ref(cache, st, "strided")
    a, sv, w, stats = q.state()
    assert w.tobytes() == st.w.tobytes() and stats.tobytes() == st.stats().tobytes()
    q.close()


# ---- 5. appended examples, the footprint ---------------------------------------------------------------------------------------------------
def test_state_of_appended_examples_and_footprint(handle, cases):
    c = cases["free"]
    q = capi.QpCache(handle, 96)
    x = padded(c, q.dims()[1])
    before = q.footprint()
    q.put(x[:5], c["ids"][:5], c["b"][:5], c["d"][:5])
    q.score(np.zeros(q.dims()[0]))
    assert q.footprint() == before                                            # a cache that never solves holds no solver state
    q.set_state(a=np.full(5, .25), sv=np.array([1, 0, 1, 0, 1], np.uint8))
    assert q.footprint() > before
    q.put(x[5:9], c["ids"][5:9], c["b"][5:9], c["d"][5:9])
    a, sv, w, st = q.state()
    assert a[:9].tolist() == [.25] * 5 + [0.0] * 4 and sv[:9].tolist() == [1, 0, 1, 0, 1, 1, 1, 1, 1] and not sv[9:].any()
    assert not w.any() and not st.any()
    _, wreg, w0, _ = handle.model.qp_vectors()
    q.refresh()
    w = q.state()[2]
    assert w.any() and q.weights().tobytes() == (w / wreg + w0).tobytes()
    q.close()


# ---- 6. refusals leave the state untouched ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_untouched(handle, cases):
    L = capi.lib()
    c = cases["binding"]
    q = load(handle, c, 128)
    length, k, cap, n = q.dims()
    q.solve_pass(sc.next_order(c, 0, q.state()[1]))
    before = [v.tobytes() for v in q.state()]
    loss = C.c_double(-3.0)

    def run(order):
        o = np.asarray(order, np.int32)
        return L.pbd_qp_pass(q.q, o.ctypes.data, len(o), C.byref(loss))

    def untouched():
        return [v.tobytes() for v in q.state()] == before and loss.value == -3.0
    assert run([0, 1, 2, 1]) == capi.PBD_ERR_ARG and untouched()                  # a duplicate
    assert run([0, n]) == capi.PBD_ERR_ARG and untouched()                        # out of range
    assert run([-1]) == capi.PBD_ERR_ARG and untouched()
    assert L.pbd_qp_pass(q.q, None, 3, C.byref(loss)) == capi.PBD_ERR_ARG and untouched()
    assert L.pbd_qp_one(q.q, np.array([2, 2], np.int32).ctypes.data, 2) == capi.PBD_ERR_ARG and untouched()
    bad = np.array([0, length], np.int32)
    assert L.pbd_qp_noneg(q.q, bad.ctypes.data, 2) == capi.PBD_ERR_ARG and untouched()   # a noneg index >= len
    assert L.pbd_qp_noneg(q.q, np.array([-1], np.int32).ctypes.data, 1) == capi.PBD_ERR_ARG and untouched()
    assert L.pbd_qp_fix(q.q, n + 1) == capi.PBD_ERR_ARG and L.pbd_qp_fix(q.q, -1) == capi.PBD_ERR_ARG and untouched()
    assert L.pbd_qp_state_put(q.q, None, None, cap + 1) == capi.PBD_ERR_ARG and untouched()
    # a column of put whose blocks overlap each other: accepted by put, refused by a pass that would add it into w
    col = np.zeros((1, k), np.float32)
    col[0, :1 + 2 * 7] = [2, 11, 15, 1, 1, 1, 1, 1, 13, 17, 1, 1, 1, 1, 1]
    q.put(col)
    before = [v.tobytes() for v in q.state()]
    assert run([3, n, 5]) == capi.PBD_ERR_UNSUPPORTED and untouched()
    assert b"overlap" in L.pbd_last_error(handle.h)
    assert run([3, 5]) == capi.PBD_OK and loss.value != -3.0                      # the other examples still solve
    q.close()
    # an empty cache
    q = capi.QpCache(handle, 8)
    before = [v.tobytes() for v in q.state()]
    loss.value = -3.0
    n_out = C.c_int(-2)
    assert L.pbd_qp_pass(q.q, np.zeros(1, np.int32).ctypes.data, 1, C.byref(loss)) == capi.PBD_ERR_STATE and untouched()
    assert L.pbd_qp_refresh(q.q) == capi.PBD_ERR_STATE and L.pbd_qp_loss(q.q, C.byref(loss)) == capi.PBD_ERR_STATE
    assert L.pbd_qp_opt(q.q, .05, 10, 0, None, None, None) == capi.PBD_ERR_STATE
    assert L.pbd_qp_prune(q.q, C.byref(n_out)) == capi.PBD_ERR_STATE and n_out.value == -2 and untouched()
    q.close()
