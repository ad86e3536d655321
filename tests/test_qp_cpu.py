"""The training example cache without a GPU: tests/qp_ref.py (the contract of include/pbd_c.h in numpy) against the compiled
matlab/mex/score.cc and lincomb.cc (tests/golden/ref_qp_v1.npz, recorded by tests/golden/make_ref_qp.py), the stated order of d and
b against exact sums, the tie between a written example and the dense feature vector, Model.qp_vectors() against a hand-written
model2vec.m case, and the new entry points' presence and NULL refusals (the library loads without a GPU)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import dense_feature_vectors, make_tree_model_k, make_voc_like_model
from tests import qp_cases, qp_ref
from tests.feature_vector_ref import feature_vector_ref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ref_qp_v1.npz")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, make in qp_cases.CASES.items()}


# ---- score and lincomb against the compiled reference files -----------------------------------------------------------------
def test_score_and_lincomb_equal_the_compiled_reference_bit_for_bit(golden, cases):
    seen = 0
    for name, c in cases.items():
        for iname, inds in c["inds"].items():
            s = qp_ref.score_ref(c["x"], c["w"], inds)
            w = qp_ref.lincomb_ref(c["x"], c["a"], inds, qp_cases.LEN)
            assert s.tobytes() == golden[f"{name}_score_{iname}"].tobytes(), (name, iname)
            assert w.tobytes() == golden[f"{name}_lincomb_{iname}"].tobytes(), (name, iname)
            seen += 1
    assert seen == sum(len(c["inds"]) for c in cases.values()) == len(golden.files) // 2


def test_the_cases_cover_what_they_claim(golden, cases):
    m = cases["mixed"]
    lens = [[n for _, n, _ in qp_cases.parse(col)] for col in m["x"]]
    assert lens[0] == [1] and lens[4] == []                                       # one block of length 1; no block at all
    assert any(n > 4096 for l in lens for n in l) and any(n % 64 for l in lens for n in l)
    assert len(m["inds"]["empty"]) == 0 and len(golden["mixed_score_empty"]) == 0 and not golden["mixed_lincomb_empty"].any()
    u = m["inds"]["unsorted"]
    assert (np.diff(u) < 0).any() and len(set(u.tolist())) < len(u)               # unsorted, with repeats
    assert (m["a"] == 0).any() and (m["a"] < 0).any()
    vals = np.abs(np.concatenate([col[xo:xo + n] for col in m["x"] for _, n, xo in qp_cases.parse(col)] + [m["w"]]))
    assert np.log10(vals.max() / vals[vals > 0].min()) > 11                       # about 12 decades
    # cancellation: example 2's score is far below the sum of its products' magnitudes
    col = m["x"][2]
    mag = sum(float(np.abs(m["w"][s:s + n] * col[xo:xo + n].astype(np.float64)).sum()) for s, n, xo in qp_cases.parse(col))
    assert abs(golden["mixed_score_all"][2]) < 1e-3 * mag
    assert len(cases["overlap"]["x"]) > 64                                        # more examples than a wavefront


def test_the_fixture_tells_a_sequential_sum_from_a_tree(golden, cases):
    """a pairwise and a 64-lane-strided summation of the SAME products differ in bits from the recorded results"""
    c = cases["mixed"]
    for how in ("pairwise", "strided"):
        assert qp_ref.score_ref(c["x"], c["w"], c["inds"]["all"], how).tobytes() != golden["mixed_score_all"].tobytes(), how
    c = cases["overlap"]
    got = qp_ref.lincomb_ref(c["x"], c["a"], c["inds"]["all"], qp_cases.LEN, "pairwise")
    assert got.tobytes() != golden["overlap_lincomb_all"].tobytes()
    # ... and lincomb's order matters: the same examples in another order give other bits (qp_refresh.m:16-17 sorts for a reason)
    assert golden["overlap_lincomb_all"].tobytes() != golden["overlap_lincomb_sorted_by_a"].tobytes()


# ---- the write ----------------------------------------------------------------------------------------------------------------
def written(model, label, dtype=np.float32, seed=3, n=6, cpos=0.002, cneg=0.004):
    """records at random places of random planes (some windows cross the edge), their feature vectors by the numpy definition, and
    qp_ref's write of them"""
    rng = np.random.default_rng(seed)
    planes = {l: rng.uniform(0.0, 0.4, (9 + l, 11 + l, 32)).astype(dtype) for l in range(3)}
    heads = np.zeros(n, capi.HEAD_DTYPE)
    locs = np.zeros((n, model.max_parts, 3), np.int32)
    for i in range(n):
        c = i % model.ncomponents
        l = i % 3
        heads[i] = (0.0, c, l, model.nparts(c))
        for p in range(model.nparts(c)):
            locs[i, p] = (rng.integers(0, 11 + l), rng.integers(0, 9 + l), rng.integers(0, len(model.filterid[c][p])))
    blocks, windows = feature_vector_ref(model, lambda l: planes[l], heads, locs, dtype)
    w, wreg, w0, _ = model.qp_vectors()
    k = qp_ref.sparselen(model)
    return heads, locs, blocks, windows, qp_ref.write_ref(model, heads, locs, blocks, windows, label, 7, cpos, cneg, wreg, w0, k)


MODELS = {"tree_k": lambda: make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21), "multi": lambda: make_voc_like_model(seed=11)}


@pytest.mark.parametrize("label", [1, -1])
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_column_format_and_ids(kind, label):
    model = MODELS[kind]()
    heads, locs, blocks, windows, (x, ids, b, d) = written(model, label)
    lay = model.feature_layout()
    assert x.dtype == np.float32 and x.shape[1] == qp_ref.sparselen(model) and lay["size"] < 2 ** 24
    for i in range(len(heads)):
        np_ = int(heads["nparts"][i])
        bl = qp_cases.parse(x[i])
        assert x[i, 0] == 3 * np_ - 1 == len(bl)
        # detect.m:272-308: root bias, root window; then bias, deformation, window per part
        kinds = ["b", "f"] + ["b", "d", "f"] * (np_ - 1)
        for (s, n, xo), kd in zip(bl, kinds):
            if kd == "b":
                assert n == 1 and lay["bias"] <= s < lay["deform"]
            elif kd == "d":
                assert n == 4 and lay["deform"] <= s < lay["filters"][0] and (s - lay["deform"]) % 4 == 0
            else:
                assert s in set(int(v) for v in lay["filters"])
        end = bl[-1][2] + bl[-1][1]
        assert not x[i, end:].any()                                               # the tail is zero
        assert ids[i].tolist() == [label, 7, int(heads["level"][i]), int(locs[i, 0, 0]), int(locs[i, 0, 1])]


@pytest.mark.parametrize("label", [1, -1])
def test_d_and_b_against_exact_sums(label):
    """d and b are sums of n rounded terms in a fixed order — one summation tree over the n terms (the partials' +0.0 starts add
    nothing: 0 + t is exact): any such order is within (n - 1) u sum |terms| of the exact sum (Higham, Accuracy and Stability, (4.4),
    to first order; the terms themselves are the same rounded numbers on both sides).  n = the squares for d; the 1 and the products
    for b"""
    model = MODELS["tree_k"]()
    cpos, cneg = 0.002, 0.004
    heads, locs, blocks, windows, (x, ids, b, d) = written(model, label, cpos=cpos, cneg=cneg)
    _, wreg, w0, _ = model.qp_vectors()
    C = cpos if label > 0 else cneg
    for i in range(len(heads)):
        sq, bt = [], [1.0]
        for s, v in qp_ref.example_blocks(model, blocks[i], windows[i]):
            v = v if label > 0 else -v
            xs = (np.float64(C) * v) / wreg[s:s + len(v)]
            sq += (xs * xs).tolist()
            bt += (-(w0[s:s + len(v)] * v)).tolist()
        assert abs(d[i] - math.fsum(sq)) <= (len(sq) - 1) * U * math.fsum(np.abs(sq).tolist())
        bias = math.fsum(bt)
        bound = (len(bt) - 1) * U * math.fsum(np.abs(bt).tolist())
        # b = (float)(C * bias): one double product and one float rounding on top
        exact = C * bias
        assert abs(float(b[i]) - exact) <= abs(C) * bound + abs(exact) * (U + 2.0 ** -24)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("label", [1, -1])
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_a_written_example_scores_like_the_dense_feature_vector(kind, label, dtype):
    """(w - w0) . wreg scored against the written example equals C (w . x_dense - w0 . x_dense) (sign of the label).  Per term:
    (w - w0) wreg carries two roundings, the stored value C v / wreg two and its float32 rounding (2^-24), their product one, the
    serial sum at most n - 1; the expected side's terms C (w - w0) v carry three: (2^-24 + (n + 7) u) sum |terms| to first order."""
    model = MODELS[kind]()
    cpos, cneg = 0.002, 0.004
    heads, locs, blocks, windows, (x, ids, b, d) = written(model, label, dtype)
    w, wreg, w0, _ = model.qp_vectors()
    C = cpos if label > 0 else cneg
    got = qp_ref.score_ref(x, (w - w0) * wreg, np.arange(len(x)))
    dense = dense_feature_vectors(model, blocks, windows)
    for i in range(len(x)):
        nz = np.flatnonzero(dense[i])
        terms = (C * (1 if label > 0 else -1)) * ((w - w0)[nz] * dense[i, nz])
        n = len(nz)
        bound = (2.0 ** -24 + (n + 7) * U) * math.fsum(np.abs(terms).tolist()) * (1 + 1e-6)
        assert abs(got[i] - math.fsum(terms.tolist())) <= bound, (i, got[i], math.fsum(terms.tolist()), bound)


def test_write_ref_refuses_repeated_blocks():
    from partsbaseddetector_amd.model import make_face_like_model
    model = make_face_like_model(seed=77, ncomp=3, nfilters=40, part_counts=(9, 12))   # one dummy bias shared by all children
    with pytest.raises(AssertionError, match="repeats"):
        written(model, 1)


# ---- model2vec.m -----------------------------------------------------------------------------------------------------------------
def test_qp_vectors_against_a_hand_written_case():
    """two components: (root + 1 part), (root + 2 parts); 1 x 1 filters.  biasw: [r0, c01, r1, c11, c12], 3 deformations"""
    from partsbaseddetector_amd.model import Model
    filt = [np.full((1, 32), float(i + 1), np.float32) for i in range(5)]
    biasw = np.array([.5, .25, -.5, .125, .0625], np.float32)
    defw = np.array([[.01, 0, .02, 0], [.03, .1, .04, .2], [.05, 0, .06, 0]], np.float32)
    m = Model(filt, biasw, np.zeros((3, 2), np.int32), defw, [[[0], [1]], [[2], [3], [4]]], [[[0], [1]], [[2], [3], [4]]],
              [[[], [0]], [[], [1], [2]]], [[-1, 0], [-1, 0, 0]])
    w, wreg, w0, noneg = m.qp_vectors()
    n = 5 + 12 + 5 * 32
    assert w.shape == wreg.shape == w0.shape == (n,) and w.dtype == wreg.dtype == w0.dtype == np.float64
    exp_w = np.concatenate([biasw, defw.ravel()] + [f.ravel() for f in filt]).astype(np.float64)
    assert w.tobytes() == exp_w.tobytes()
    exp_reg = np.ones(n)
    exp_reg[[0, 2]] = .01                                                         # the two root biases
    assert wreg.tobytes() == exp_reg.tobytes()
    exp_w0 = np.zeros(n)
    exp_w0[[5, 7, 9, 11, 13, 15]] = .01                                           # elements 0 and 2 of every deformation
    assert w0.tobytes() == exp_w0.tobytes()
    assert noneg.dtype == np.uint32 and noneg.tolist() == [5, 7, 9, 11, 13, 15]


# ---- the C ABI, no GPU -------------------------------------------------------------------------------------------------------------
QP_ENTRIES = ["pbd_qp_create", "pbd_qp_destroy", "pbd_qp_dims", "pbd_qp_footprint", "pbd_qp_write", "pbd_qp_score", "pbd_qp_score_dev",
              "pbd_qp_lincomb", "pbd_qp_lincomb_dev", "pbd_qp_keep", "pbd_qp_get", "pbd_qp_put"]


def test_exports_and_null_refusals():
    L = capi.lib()
    assert L.pbd_abi_version() == 5 == capi.PBD_ABI_VERSION
    for name in QP_ENTRIES:
        assert name in capi.EXPORTS and getattr(L, name)
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "pbd_c.h")).read()
    for name in QP_ENTRIES:
        assert name + "(" in header
    q = C.c_void_p()
    assert L.pbd_qp_create(None, 4, 1.0, 1.0, None, None, C.byref(q)) == capi.PBD_ERR_ARG and not q
    L.pbd_qp_destroy(None)                                                         # a no-op
    n = C.c_int(-5)
    assert L.pbd_qp_dims(None, None, None, None, C.byref(n)) == capi.PBD_ERR_ARG and n.value == -5
    assert L.pbd_qp_footprint(None, None) == capi.PBD_ERR_ARG
    assert L.pbd_qp_write(None, None, None, 0, 1, 0, C.byref(n)) == capi.PBD_ERR_ARG and n.value == -5
    for name in ("pbd_qp_score", "pbd_qp_score_dev", "pbd_qp_lincomb", "pbd_qp_lincomb_dev"):
        assert getattr(L, name)(None, None, None, 0, None) == capi.PBD_ERR_ARG
    assert L.pbd_qp_keep(None, None, 0) == capi.PBD_ERR_ARG
    assert L.pbd_qp_get(None, 0, 0, None, None, None, None) == capi.PBD_ERR_ARG
    assert L.pbd_qp_put(None, 0, None, None, None, None) == capi.PBD_ERR_ARG
