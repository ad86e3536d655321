"""The QP solver's chain of evidence on the CPU (include/pbd_c.h "QP solver"): tests/qp_solve_ref.py summing strictly left to right
with the reference's merge-walk dot IS the compiled matlab/mex/qp_one_sparse.cc (tests/golden/ref_qp_one_v1.npz) in bits, over
consecutive passes, and so on the large cases (ref_qp_one_v2.npz); the cases run every branch they claim; the library's order (block sums, complete dot) is told apart from it by the
fixture; the complete dot is the right one where the merge walk is not; refresh / loss / prune / opt restated; and the entry points are
declared, exported and bound.  tests/test_gpu_qp_solve.py closes the chain: library == strided / complete restatement in bits."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from tests import qp_solve_cases as sc
from tests import qp_solve_ref as sr
from tests.qp_cases import LEN

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ref_qp_one_v1.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pbd_qp_noneg", "pbd_qp_fix", "pbd_qp_state_put", "pbd_qp_state_get", "pbd_qp_pass", "pbd_qp_one", "pbd_qp_refresh",
       "pbd_qp_loss", "pbd_qp_opt", "pbd_qp_prune", "pbd_qp_weights"]
KEYS = ("loss", "a", "w", "sv", "l")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, make in sc.CASES.items()}


@pytest.fixture(scope="module")
def runs(cases):
    return {(name, s, d): sr.run_passes(c, s, d) for name, c in cases.items() for s, d in (("sequential", "merge"), ("strided", "complete"))}


# ---- 1. sequential / merge is the compiled reference file ---------------------------------------------------------------------------
def test_sequential_restatement_equals_the_compiled_reference(golden, cases, runs):
    for name, c in cases.items():
        assert 40 <= len(c["x"]) <= 130 and 4 <= c["passes"] <= 6
        out, _ = runs[name, "sequential", "merge"]
        for p, r in enumerate(out):
            for key in KEYS:
                g = golden[f"{name}_{p}_{key}"]
                assert r[key].dtype == g.dtype and r[key].tobytes() == g.tobytes(), (name, p, key)


# ---- 2. the cases cover what they claim -----------------------------------------------------------------------------------------------
def test_cases_run_every_branch(cases, runs):
    free, binding = runs["free", "strided", "complete"][1], runs["binding", "strided", "complete"][1]
    assert free["pair"] == 0 and free["single"] > 0            # the per-id constraint never binds there
    for key in ("pair", "clip_C_minus_Ai", "clip_Ai2", "clip_minus_Ai", "clip_Ai2_minus_C", "sv_clear", "pg_zero", "clamp", "err"):
        assert binding[key] > 0, key
        assert runs["binding", "sequential", "merge"][1][key] > 0, key
    c = cases["binding"]
    lens = {n for col in c["x"] for _, n, _ in sr.parse(col)}
    assert {1, 63, 64, 65} <= lens and max(lens) > 4096
    assert any(col[0] == 0 for col in c["x"]) and (c["d"] == 0).sum() == 1
    # same-id pairs whose blocks intersect partially
    partial = 0
    for i in range(len(c["x"])):
        for j in np.flatnonzero((c["ids"] == c["ids"][i]).all(axis=1)):
            if j > i:
                for s, n, _ in sr.parse(c["x"][i]):
                    for s2, n2, _ in sr.parse(c["x"][j]):
                        lo, hi = max(s, s2), min(s + n, s2 + n2)
                        partial += lo < hi and (hi - lo) < min(n, n2)
    assert partial > 0
    # orders: permutations of find(sv) and of a subset
    sv = np.ones(len(c["x"]), np.uint8)
    assert sorted(sc.next_order(c, 0, sv)) == list(range(len(sv))) and len(sc.next_order(c, 1, sv)) < len(sv)
    # memcmp order of the ids differs from their numeric order
    by_bytes = sorted(range(len(sv)), key=lambda i: c["ids"][i].tobytes())
    assert [tuple(c["ids"][i]) for i in by_bytes] != sorted(tuple(r) for r in c["ids"])


# ---- 2b. the large cases: 77-block columns; 1200 ids under a noneg list of 1600 entries ------------------------------------------------
GOLDEN_V2 = os.path.join(os.path.dirname(__file__), "golden", "ref_qp_one_v2.npz")


@pytest.fixture(scope="module")
def large():
    cases = {name: make() for name, make in sc.LARGE_CASES.items()}
    return cases, {(name, s): sr.run_passes(c, s, d) for name, c in cases.items() for s, d in (("sequential", "merge"), ("strided", "complete"))}


def test_large_cases_sequential_restatement_equals_the_compiled_reference(large):
    golden = np.load(GOLDEN_V2)
    cases, runs = large
    assert os.path.getsize(GOLDEN_V2) <= max(os.path.getsize(os.path.join(os.path.dirname(GOLDEN_V2), f))
                                             for f in os.listdir(os.path.dirname(GOLDEN_V2)) if f.endswith("_v1.npz"))
    assert len(golden.files) == sum(5 * c["passes"] for c in cases.values())
    for name, c in cases.items():
        out, _ = runs[name, "sequential"]
        assert len(out) == c["passes"]
        for p, r in enumerate(out):
            for key in KEYS:
                g = golden[f"{name}_{p}_{key}"]
                assert r[key].dtype == g.dtype and r[key].tobytes() == g.tobytes(), (name, p, key)
        # and the fixture tells the library's order from it
        lib = runs[name, "strided"][0]
        assert any(r[key].tobytes() != golden[f"{name}_{p}_{key}"].tobytes() for p, r in enumerate(lib) for key in KEYS), name


def test_large_cases_run_what_they_claim(large):
    cases, runs = large
    clips = ("clip_C_minus_Ai", "clip_Ai2", "clip_minus_Ai", "clip_Ai2_minus_C")
    for name, c in cases.items():
        for s in ("sequential", "strided"):
            cnt = runs[name, s][1]
            print(name, s, cnt)
            assert cnt["pair"] > 0 and cnt["single"] > 0 and cnt["clamp"] > 0 and sum(cnt[k] for k in clips) > 0, (name, s, cnt)
        # ascending blocks inside K / LEN: the merge walk is complete on them
        for col in c["x"][:200]:
            blocks = sr.parse(col)
            assert all(s0 + n0 <= s1 for (s0, n0, _), (s1, _, _) in zip(blocks, blocks[1:])) and blocks[-1][0] + blocks[-1][1] <= LEN
    mb, mi = cases["manyblock"], cases["manyids"]
    assert len(mb["x"]) == 48 and mb["passes"] == 4 and {int(col[0]) for col in mb["x"]} == {77}         # 3 * 26 - 1 blocks, > 4 x 16
    lens = [n for col in mb["x"] for _, n, _ in sr.parse(col)]
    assert set(lens) == {1, 4, 63, 64, 65, 70} and lens.count(1) == 48 * 26 and lens.count(4) == 48 * 25
    assert all(len(np.flatnonzero((mb["ids"] == r).all(axis=1))) == 4 for r in mb["ids"])
    partial = 0                                      # same-id pairs whose windows intersect partially
    for i in range(len(mb["x"])):
        for j in np.flatnonzero((mb["ids"] == mb["ids"][i]).all(axis=1)):
            if j > i:
                for s, n, _ in sr.parse(mb["x"][i]):
                    for s2, n2, _ in sr.parse(mb["x"][j]):
                        lo, hi = max(s, s2), min(s + n, s2 + n2)
                        partial += lo < hi and (hi - lo) < min(n, n2)
    assert partial > 0
    assert len(mi["x"]) == 2400 and mi["passes"] == 2 and len(np.unique(mi["ids"], axis=0)) == 1200
    assert {int(col[0]) for col in mi["x"]} == {2} and {n for col in mi["x"] for _, n, _ in sr.parse(col)} == {1} | set(range(3, 40))
    assert len(mi["noneg"]) >= 1500 and len(mi["noneg"]) > 1024 and len(np.unique(mi["noneg"])) == len(mi["noneg"])
    for s in ("sequential", "strided"):
        assert runs["manyids", s][1]["err_past_1024"] > 0              # the loss has terms beyond its first 1024 ids
        # entries of noneg beyond the first 1024 are clamped: some w there is 0 after a pass and was not before it
        w0, w1 = mi["w"][mi["noneg"][1024:]], runs["manyids", s][0][0]["w"][mi["noneg"][1024:]]
        assert (w1 >= 0).all() and ((w1 == 0) & (w0 != 0)).any()


# ---- 3. the fixture tells the two orders apart ------------------------------------------------------------------------------------------
def test_library_order_differs_from_the_reference_in_bits(golden, cases, runs):
    for name, c in cases.items():
        out, _ = runs[name, "strided", "complete"]
        differ = [key for p, r in enumerate(out) for key in KEYS if r[key].tobytes() != golden[f"{name}_{p}_{key}"].tobytes()]
        assert differ, name


# ---- 4. merge versus complete dot ---------------------------------------------------------------------------------------------------------
def test_complete_dot_is_right_where_the_merge_walk_is_not(cases):
    x1, x2 = sc.nonascending_pair()
    exact = math.fsum(sc.dense(x1) * sc.dense(x2))
    merge, complete = sr.dot_merge(x1, x2, "sequential"), sr.dot_complete(x1, x2, "strided")
    assert merge != complete
    assert abs(merge - exact) > 1e-6 * abs(exact)                                 # the walk misses intersections
    assert abs(complete - exact) <= 1e-12 * abs(exact)
    # on ascending pairs the two visit the same products: equal exactly when summed exactly
    c = cases["binding"]
    for i, j in ((0, 1), (2, 7), (14, 3), (9, 5), (20, 21)):
        got = []
        for f in (sr.dot_merge, sr.dot_complete):
            terms = []
            f(c["x"][i], c["x"][j], "sequential", terms)
            got.append(math.fsum(terms))
        assert got[0] == got[1] == math.fsum(sc.dense(c["x"][i]) * sc.dense(c["x"][j])), (i, j)


# ---- 5. refresh, loss, prune and opt ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def opts(cases):
    return {s: sr.opt_run(cases["binding"], s, d) for s, d in (("sequential", "merge"), ("strided", "complete"))}


def test_opt_converges_and_weak_duality_holds_across_orders(cases, opts):
    for s, (lb, ub, t, st) in opts.items():
        assert 0 < t < 1000 and lb > 0 and 1 - lb / ub < .05, (s, lb, ub, t)
        assert st.ub == ub and (st.a >= 0).all() and (st.a <= 1).all()
    (lbs, ubs, _, _), (lbt, ubt, _, _) = opts["sequential"], opts["strided"]
    # the two sides are separated by far more than rounding, so the inequalities need no slack
    assert ubs - lbt > 1e-6 * ubs and ubt - lbs > 1e-6 * ubt
    assert lbt <= ubs and lbs <= ubt


def test_refresh_loss_and_prune_restated(cases, opts):
    c = cases["binding"]
    n = len(c["x"])
    cache = (c["x"], c["ids"], c["b"], c["d"])
    st = opts["strided"][3].copy()
    # refresh: w is the sorted lincomb, clamped; l and lb follow
    before = st.copy()
    sr.refresh_ref(cache, st, "strided")
    assert st.lb_old == before.lb and (st.w[c["noneg"]] >= 0).all()
    dense = np.stack([sc.dense(col) for col in c["x"]])
    assert np.allclose(st.w, np.maximum(st.a @ dense, np.where(np.isin(np.arange(LEN), c["noneg"]), 0.0, -np.inf)), rtol=1e-9, atol=1e-12)
    assert abs(st.l - float(c["b"].astype(np.float64) @ st.a)) < 1e-12 * n
    assert st.lb == st.l - st.ww * .5 and abs(st.ww - float(st.w @ st.w)) <= 1e-12 * st.ww
    # loss: per id the largest positive slack
    slack = c["b"].astype(np.float64) - dense @ st.w
    want = sum(max(0.0, slack[(c["ids"] == g).all(axis=1)].max()) for g in np.unique(c["ids"], axis=0))
    assert abs(sr.loss_ref(cache, st, n) - want) <= 1e-9 * max(want, 1.0)
    # prune: the support vectors move to the front, w is rebuilt in index order
    st.nfix = 2
    st.sv[:] = 1
    pruned, m = sr.prune_ref(cache, st.copy(), n, "strided")
    keep = np.flatnonzero((st.a > 0) | (np.arange(n) < 2))
    assert m == len(keep) < n and pruned[0].tobytes() == c["x"][keep].tobytes()
    st2 = st.copy()
    st2.sv[:] = 0
    st2.sv[[3, 4, 50]] = 1                                                        # not all set: sv is taken as it is
    pruned, m = sr.prune_ref(cache, st2, n, "strided")
    assert m == 3 and st2.a[:3].tobytes() == st.a[[3, 4, 50]].tobytes() and not st2.a[3:].any() and st2.sv.sum() == 3
    assert st2.lb_old == st.lb_old and st2.lb == st2.l - st2.ww * .5


def test_shuffle_generator_is_the_stated_one():
    nxt = sr.splitmix64(0)
    assert [nxt() for _ in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]   # splitmix64's published vector
    assert sorted(sr.shuffle(range(10), sr.splitmix64(5))) == list(range(10))
    assert list(sr.shuffle([4], sr.splitmix64(5))) == [4]


# ---- 6. declared, exported, bound -----------------------------------------------------------------------------------------------------
def test_solver_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"\b(pbd_[a-z0-9_]+)\s*\(", hdr))
    L = capi.lib()
    for name in NEW:
        assert name in declared and name in capi.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    for m in ("noneg", "fix", "state", "set_state", "solve_pass", "one", "refresh", "loss", "opt", "prune", "weights"):
        assert callable(getattr(capi.QpCache, m)), m
    assert L.pbd_abi_version() == 5
    host = open(os.path.join(ROOT, "partsbaseddetector_amd", "host", "pbd_host.hpp")).read()
    for name in NEW:
        assert name + "(" in host, f"{name} is not used by pbd::ExampleCache"


def test_null_handles_are_refused():
    L = capi.lib()
    v = C.c_double()
    n = C.c_int()
    assert L.pbd_qp_noneg(None, None, 0) == capi.PBD_ERR_ARG
    assert L.pbd_qp_fix(None, 0) == capi.PBD_ERR_ARG
    assert L.pbd_qp_state_put(None, None, None, 0) == capi.PBD_ERR_ARG
    assert L.pbd_qp_state_get(None, None, None, None, None) == capi.PBD_ERR_ARG
    assert L.pbd_qp_pass(None, None, 0, C.byref(v)) == capi.PBD_ERR_ARG
    assert L.pbd_qp_one(None, None, 0) == capi.PBD_ERR_ARG
    assert L.pbd_qp_refresh(None) == capi.PBD_ERR_ARG
    assert L.pbd_qp_loss(None, C.byref(v)) == capi.PBD_ERR_ARG
    assert L.pbd_qp_opt(None, .05, 10, 0, C.byref(v), C.byref(v), C.byref(n)) == capi.PBD_ERR_ARG
    assert L.pbd_qp_prune(None, C.byref(n)) == capi.PBD_ERR_ARG
    assert L.pbd_qp_weights(None, C.byref(v)) == capi.PBD_ERR_ARG
