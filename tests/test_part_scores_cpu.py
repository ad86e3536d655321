"""Per-part scores (pbd_part_score): the definition checked on the CPU oracle, and the interface's presence.

Every comparison is between the oracle's own planes and its own part locations, so no candidate is excused as a near tie."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_face_like_model, make_image, make_person_model, make_tree_model_k
from tests.part_scores_ref import bound, part_scores_ref, totals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbd_set_part_scores", "pbd_get_part_scores", "pbd_candidates_part_scores")
CAPACITY = 8192


def models():
    return {"person": make_person_model(seed=1234, K=3),
            "tree_k": make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21),
            "multi": make_face_like_model(seed=77, ncomp=3, nfilters=40, part_counts=(9, 12))}


def rescored(orc, model, im, dtype, correct_ptr, q=99.5):
    """(total, rootv, B) of every detection of the oracle at the q-th percentile of its root values"""
    model.thresh = -1e30
    _, _, _, _, fr = orc.detect(model, im, capacity=1, keep=True, correct_ptr=correct_ptr, dtype=dtype)
    vals = np.concatenate([fr.root(l)[0].ravel() for l in range(fr.nlevels)])
    fr.free()
    model.thresh = float(np.float32(np.percentile(vals, q)))
    heads, _, locs, _, fr = orc.detect(model, im, capacity=CAPACITY, keep=True, correct_ptr=correct_ptr, dtype=dtype)
    assert 5 < len(heads) < CAPACITY
    ps = part_scores_ref(model, fr.resp, heads, locs)
    roots = {}
    rootv = np.zeros(len(heads), np.float64)
    for i in range(len(heads)):
        l = int(heads["level"][i])
        if l not in roots:
            roots[l] = fr.root(l)[0]
        rootv[i] = roots[l][heads["component"][i], locs[i, 0, 1], locs[i, 0, 0]]
    fr.free()
    if np.dtype(dtype) == np.dtype(np.float32):
        np.testing.assert_array_equal(rootv.astype(np.float32), heads["score"])
    return totals(ps), rootv, bound(ps, heads["nparts"], dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["person", "tree_k", "multi"])
def test_definition_reproduces_the_root_score(orc, kind, dtype):
    total, rootv, B = rescored(orc, models()[kind], make_image(5, 320, 240), dtype, correct_ptr=1)
    r = np.abs(total - rootv) / B
    print(f"{kind} {np.dtype(dtype).name}: {len(total)} detections, worst |total - rootv| / B = {r.max():.3f}")
    assert (np.abs(total - rootv) <= B).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["person", "tree_k", "multi"])
def test_reference_pointer_composition_scores_below_its_root(orc, kind, dtype):
    total, rootv, B = rescored(orc, models()[kind], make_image(5, 320, 240), dtype, correct_ptr=0)
    below = int((total < rootv - B).sum())
    print(f"{kind} {np.dtype(dtype).name}: {below} of {len(total)} detections re-score below rootv - B")
    assert (total <= rootv + B).all()
    assert 2 * below >= len(total)


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"\b(pbd_[a-z0-9_]+)\s*\(", hdr))
    tune = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libpbd_hip_tune.so"))
    for name in NAMES:
        assert name in declared
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name) and hasattr(tune, name)
    for m in ("set_part_scores", "part_scores", "candidates_part_scores"):
        assert hasattr(capi.Handle, m)
    assert "typedef struct pbd_part_score" in hdr
    assert capi.lib().pbd_abi_version() == capi.PBD_ABI_VERSION


def test_argument_errors_before_any_hip_call():
    L = capi.lib()
    out = (C.c_double * 3)()
    cnt = C.c_int(-1)
    assert L.pbd_set_part_scores(None, 1) == capi.PBD_ERR_ARG
    assert L.pbd_get_part_scores(None, 0, out, 1, C.byref(cnt)) == capi.PBD_ERR_ARG
    assert L.pbd_candidates_part_scores(None, None, None, 0, out) == capi.PBD_ERR_ARG
    assert cnt.value == -1


def test_host_layer_fills_confidences():
    """detector.Candidate: confidence()[p] = (float)score_p for p >= 1 with the step on, the root score at 0; zeros with it off"""
    from partsbaseddetector_amd.detector import Candidate
    ps = np.array([[1.0, 0.0, 0.5], [2.0, -0.25, 0.125], [0.0, 0.0, 0.0]])
    heads = np.zeros(1, capi.HEAD_DTYPE)
    heads[0] = (7.0, 0, 3, 2)
    boxes, locs = np.zeros((1, 3, 4), np.int32), np.zeros((1, 3, 3), np.int32)
    on = Candidate._unpack(heads, boxes, locs, ps[None])[0]
    assert on.confidence.tolist() == [7.0, 1.875] and on.confidence.dtype == np.float32 and on.score() == 7.0
    np.testing.assert_array_equal(on.partScores(), ps[:2])
    off = Candidate._unpack(heads, boxes, locs)[0]
    assert off.confidence.tolist() == [7.0, 0.0] and off.partScores() is None
