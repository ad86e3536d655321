"""Feature vectors of detections (pbd_feature_block): the definition of tests/feature_vector_ref.py checked on the CPU oracle — the
window's geometry against orc_pdf_one, the ancestor's self-check w . x = score, five slips that must each show — and the
interface's presence.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import dense_feature_vectors, make_image, make_tree_model_k
from tests import exact_bank_cases as xb
from tests.feature_vector_ref import (SLIPS, dot64, feature_vector_ref, unit_roundoff, window_bound, window_bounds, window_ref, wx)
from tests.part_scores_ref import bound, part_scores_ref, totals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbd_feature_window_max", "pbd_candidates_features", "pbd_candidates_features_f64", "pbd_candidates_features_dev")
LEVELS = [(3, 3), (5, 7), (12, 9)]                      # (ch, cw)
FILTERS = [(3, 3), (5, 5), (9, 9), (3, 7), (6, 4)]      # (kh, kw)


def random_operands(dtype, seed=3):
    rng = np.random.default_rng(seed)
    feats = [rng.uniform(0.0, 0.4, (ch, cw, 32)).astype(dtype) for ch, cw in LEVELS]
    filters = {s: rng.normal(0.0, 0.05, (s[0], s[1] * 32)).astype(np.float32) for s in FILTERS}
    return feats, filters


def geometry_errors(orc, feats, filters, dtype, slip=None):
    """(|dot64(filter, window_ref) - orc_pdf_one|, bound) over every cell of every level, every filter"""
    err, bnd = [], []
    for feat in feats:
        H, W, _ = feat.shape
        for (kh, kw), filt in filters.items():
            resp = orc.pdf_level(feat, [filt], dtype=dtype)[0]
            for y in range(H):
                for x in range(W):
                    win = window_ref(feat, x, y, kh, kw, slip)
                    err.append(abs(dot64(filt, win) - float(resp[y, x])))
                    bnd.append(window_bound(filt, win, dtype))
    return np.array(err), np.array(bnd)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_window_geometry_against_the_oracle(orc, dtype):
    feats, filters = random_operands(dtype)
    err, bnd = geometry_errors(orc, feats, filters, dtype)
    print(f"{np.dtype(dtype).name}: {len(err)} cells x filters, worst error / bound = {(err / bnd).max():.3f}")
    assert (err <= bnd).all()
    # exactly representable operands (family B of tests/exact_bank_cases.py): equality, which pins the anchor of the even sizes
    # and the 1 in the last channel of the border
    for kh, kw in FILTERS:
        for case in xb.family_b(LEVELS, [(kh, kw)] * 2):
            for feat in case.feats:
                feat = feat.astype(dtype)
                resp = orc.pdf_level(feat, case.filters, dtype=dtype)
                for n, filt in enumerate(case.filters):
                    for y in range(feat.shape[0]):
                        for x in range(feat.shape[1]):
                            assert dot64(filt, window_ref(feat, x, y, kh, kw)) == float(resp[n, y, x]), (case.name, kh, kw, n, y, x)


# ---- the self-check ------------------------------------------------------------------------------------------------------------
class ExactResponses:
    """resp[filter, y, x] = dot64(filter, window_ref): the response planes part_scores_ref reads, one exact value at a time"""

    def __init__(self, model, feat):
        self.model, self.feat, self.sizes = model, feat, model.filter_sizes()

    def __getitem__(self, k):
        f, y, x = k
        return dot64(self.model.filtersw[f], window_ref(self.feat, x, y, int(self.sizes[f, 0]), int(self.sizes[f, 1])))


def tree_k():
    return make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21)


def oracle_detections(orc, model, dtype, correct_ptr=1, q=99.0):
    """(heads, locs, feats by level, root scores in T) of the oracle on a 100 x 80 frame, at the q-th percentile of its root values"""
    im = make_image(5, 100, 80)
    model.thresh = -1e30
    _, _, _, _, fr = orc.detect(model, im, capacity=1, keep=True, correct_ptr=correct_ptr, dtype=dtype)
    vals = np.concatenate([fr.root(l)[0].ravel() for l in range(fr.nlevels)])
    fr.free()
    model.thresh = float(np.float32(np.percentile(vals, q)))
    heads, _, locs, _, fr = orc.detect(model, im, capacity=8192, keep=True, correct_ptr=correct_ptr, dtype=dtype)
    assert 5 < len(heads) < 8192
    feats = {l: fr.feat(l) for l in sorted(set(int(v) for v in heads["level"]))}
    roots = {l: fr.root(l)[0] for l in feats}
    rootv = np.array([roots[int(heads["level"][i])][heads["component"][i], locs[i, 0, 1], locs[i, 0, 0]] for i in range(len(heads))],
                     np.float64)
    fr.free()
    return heads, locs, feats, rootv


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["float32", "float64"])
def detections(request, orc):
    model = tree_k()
    return (model, request.param) + oracle_detections(orc, model, request.param)


def test_wx_equals_the_rescored_total(detections):
    model, dtype, heads, locs, feats, _ = detections
    blocks, windows = feature_vector_ref(model, feats.__getitem__, heads, locs, dtype)
    got, mag = wx(model.weight_vector(), dense_feature_vectors(model, blocks, windows))
    exact = {l: ExactResponses(model, f) for l, f in feats.items()}
    total = totals(part_scores_ref(model, exact.__getitem__, heads, locs))
    r = np.abs(got - total) / (2.0 * 2.0 ** -53 * mag)
    print(f"{np.dtype(dtype).name}: {len(heads)} detections, worst |w.x - total| / (2 u64 sum |terms|) = {r.max():.3f}")
    assert (r <= 1.0).all()


def test_wx_equals_the_oracles_root_score(detections):
    """the ancestor's "Crucial DEBUG assertion" (detect.m:139-145), on the oracle's arg-max pointers"""
    model, dtype, heads, locs, feats, rootv = detections
    blocks, windows = feature_vector_ref(model, feats.__getitem__, heads, locs, dtype)
    got, _ = wx(model.weight_vector(), dense_feature_vectors(model, blocks, windows))
    exact = {l: ExactResponses(model, f) for l, f in feats.items()}
    ps = part_scores_ref(model, exact.__getitem__, heads, locs)
    B = bound(ps, heads["nparts"], dtype) + window_bounds(model, blocks, windows, dtype)
    r = np.abs(got - rootv) / B
    print(f"{np.dtype(dtype).name}: {len(heads)} detections, worst |w.x - rootv| / bound = {r.max():.3f}")
    assert (r <= 1.0).all()


# ---- slips ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_slips_change_a_result(orc, detections, slip):
    model, dtype, heads, locs, feats, rootv = detections
    good = feature_vector_ref(model, feats.__getitem__, heads, locs, dtype)
    bad = feature_vector_ref(model, feats.__getitem__, heads, locs, dtype, slip)
    if slip in ("anchor", "border", "swap"):   # the geometry test notices it
        feats_r, filters = random_operands(dtype)
        err, bnd = geometry_errors(orc, feats_r, filters, dtype, slip)
        assert (err > bnd).any()
    else:                                      # the blocks differ
        assert good[0].tobytes() != bad[0].tobytes()
    # and w . x leaves the root score — but for the two slips these detections cannot show: their filters are 5 x 5, where
    # (k - 1) // 2 = k // 2, and no window of theirs need leave its plane
    if slip not in ("anchor", "border"):
        got, _ = wx(model.weight_vector(), dense_feature_vectors(model, *bad))
        exact = {l: ExactResponses(model, f) for l, f in feats.items()}
        B = bound(part_scores_ref(model, exact.__getitem__, heads, locs), heads["nparts"], dtype) + window_bounds(model, *good, dtype)
        assert (np.abs(got - rootv) > B).any()


def test_dense_vectors_refuse_a_repeated_block():
    """qp_write.m:34-35: a model that uses one filter id for two parts of a component cannot be written as sparse blocks"""
    model = make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21)
    heads = np.zeros(1, capi.HEAD_DTYPE)
    heads[0] = (0.0, 0, 0, 5)
    locs = np.zeros((1, 5, 3), np.int32)
    locs[0, :, :2] = 4
    feat = np.random.default_rng(1).uniform(0, 0.4, (9, 9, 32)).astype(np.float32)
    blocks, windows = feature_vector_ref(model, lambda l: feat, heads, locs, np.float32)
    x = dense_feature_vectors(model, blocks, windows)
    assert x.shape == (1, model.feature_layout()["size"]) == (1, len(model.weight_vector()))
    blocks[0, 2]["filter_id"] = blocks[0, 1]["filter_id"]
    with pytest.raises(AssertionError, match="repeats"):
        dense_feature_vectors(model, blocks, windows)


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"\b(pbd_[a-z0-9_]+)\s*\(", hdr))
    tune = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libpbd_hip_tune.so"))
    for name in NAMES:
        assert name in declared and name in capi.EXPORTS
        assert hasattr(capi.lib(), name) and hasattr(tune, name)
    for m in ("feature_window_max", "candidates_features", "candidates_features_dev"):
        assert hasattr(capi.Handle, m)
    assert "typedef struct pbd_feature_block" in hdr and "#define PBD_FEATVEC_STAGING_BYTES" in hdr
    assert C.sizeof(capi.pbd_feature_block) == capi.FEATURE_BLOCK_DTYPE.itemsize == 56
    assert int(re.search(r"#define PBD_FEATVEC_STAGING_BYTES \(\(size_t\)(\d+) << 20\)", hdr).group(1)) << 20 == capi.PBD_FEATVEC_STAGING_BYTES
    assert capi.lib().pbd_abi_version() == capi.PBD_ABI_VERSION == 5
    assert "the per-part\n * scores are the detection's feature vector" not in hdr


def test_argument_errors_before_any_hip_call():
    L = capi.lib()
    assert L.pbd_feature_window_max(None) == -capi.PBD_ERR_ARG
    assert L.pbd_candidates_features(None, None, None, 0, None, None) == capi.PBD_ERR_ARG
    assert L.pbd_candidates_features_f64(None, None, None, 0, None, None) == capi.PBD_ERR_ARG
    assert L.pbd_candidates_features_dev(None, None, None, 0, None, None) == capi.PBD_ERR_ARG
