"""The best pose per ground-truth box (include/pbd_c.h: pbd_candidates_best_overlap), without a GPU: the definition (tests/bestoverlap_ref.py)
against a line-by-line matlab/detection/bestoverlap.m, the library's host function against the definition — index and overlap bit
for bit — on random records and on the hand-made cases every clause of the definition needs, and every refusal."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from tests import bestoverlap_ref as ref

NEW = ("pbd_candidates_best_overlap", "pbd_candidates_select_gt", "pbd_detect_gtbox_u8", "pbd_detect_gtbox_dev_u8",
       "pbd_detect_batch_gtbox_u8")


def _same(got, exp, what=""):
    assert np.array_equal(got[0], exp[0]), (what, got[0], exp[0])
    assert np.asarray(got[1], np.float64).tobytes() == np.asarray(exp[1], np.float64).tobytes(), (what, got[1], exp[1])


def _rec(items, mp=3):
    """items: (score, [(cx, cy), ...] part centres as unit boxes, or None for nparts = 0) -> records"""
    heads = np.zeros(len(items), capi.HEAD_DTYPE)
    boxes = np.full((len(items), mp, 4), 123456789, np.int32)   # junk beyond nparts
    for i, (s, cs) in enumerate(items):
        heads["score"][i] = s
        heads["nparts"][i] = 0 if cs is None else len(cs)
        for p, (x, y) in enumerate(cs or []):
            boxes[i, p] = (x, y, 1, 1)
    return heads, boxes


SQUARE = [(1, 1), (2, 2)]    # centre box 1..2 x 1..2: inter 4 with any gt box around it


@pytest.mark.parametrize("n", [300, 1100])
@pytest.mark.parametrize("P", [1, 5])
def test_definition_is_bestoverlap_m_and_the_host_function_is_the_definition(P, n):
    heads, boxes = ref.records(100 * P + n, n, P)
    assert len(np.unique(heads["score"])) == n
    cx2 = 2 * boxes[:, :, 0] + boxes[:, :, 2] - 1                  # twice the centre: odd = a half-integer centre
    assert (cx2 % 2 == 0).any() and (cx2 % 2 == 1).any()
    gts = ref.gt_boxes(7 * P + n, 12)
    m = ref.to_matrix(heads, boxes, P)
    hits = 0
    for ov in (0.0, 5e-5, 0.3, 0.6):                               # (one part: the centre box is a point, o = 1 / area)
        best, o = ref.best_overlap_def(heads, boxes, gts, ov)
        for g, gt in enumerate(gts):
            pick = ref.bestoverlap_m(m, gt, ov)
            assert (-1 if pick is None else pick) == best[g], (ov, g)
        hits += int((best >= 0).sum())
        _same(capi.candidates_best_overlap(heads, boxes, gts, ov), (best, o), ov)
    assert hits > 12


def test_boundary_of_the_strict_comparison():
    heads, boxes = _rec([(1.0, SQUARE)])
    for gt, ov in (((0, 0, 3, 3), 0.25), ((1, 1, 2, 4), 0.5)):    # inter 4 / area 16 and 4 / 8: exact
        best, o = capi.candidates_best_overlap(heads, boxes, [gt], ov)
        assert best[0] == -1 and o[0] == 0.0, "o == overlap is no match"
        below = float(np.nextafter(ov, 0.0))                        # o is one ulp above this overlap
        best, o = capi.candidates_best_overlap(heads, boxes, [gt], below)
        assert best[0] == 0 and o[0] == ov
        _same((best, o), ref.best_overlap_def(heads, boxes, [gt], below))


def test_ties_and_signed_zeros_go_to_the_first():
    gt = [(0, 0, 3, 3)]
    for scores in ((1.0, 1.0, 1.0), (-0.0, 0.0), (0.0, -0.0), (-1.0, 0.0, -0.0, 0.0)):
        heads, boxes = _rec([(s, SQUARE) for s in scores])
        exp = int(np.argmax(np.array(scores, np.float32)))
        got = capi.candidates_best_overlap(heads, boxes, gt, 0.1)
        assert got[0][0] == exp, scores
        _same(got, ref.best_overlap_def(heads, boxes, gt, 0.1))


def test_winner_is_not_the_globally_best_and_no_match():
    heads, boxes = _rec([(5.0, [(100, 100), (101, 101)]), (1.0, SQUARE), (0.5, SQUARE)])
    got = capi.candidates_best_overlap(heads, boxes, [(0, 0, 3, 3), (50, 50, 60, 60)], 0.2)
    assert list(got[0]) == [1, -1] and got[1][0] == 0.25 and got[1][1] == 0.0
    _same(got, ref.best_overlap_def(heads, boxes, [(0, 0, 3, 3), (50, 50, 60, 60)], 0.2))


def test_degenerate_gt_boxes():
    heads, boxes = _rec([(1.0, SQUARE), (2.0, [(7, 7)])])
    zero = [(5, 5, 4, 9)]                                           # x2 - x1 + 1 = 0: 0 / 0 = NaN matches nothing, whatever the overlap
    for ov in (0.3, -1.0):
        got = capi.candidates_best_overlap(heads, boxes, zero, ov)
        assert got[0][0] == -1 and got[1][0] == 0.0
        _same(got, ref.best_overlap_def(heads, boxes, zero, ov))
    neg = [(10, 10, 5, 5)]                                          # both sides -4: area 16, inter 0, o = 0
    got = capi.candidates_best_overlap(heads, boxes, neg, 0.3)
    assert got[0][0] == -1
    got = capi.candidates_best_overlap(heads, boxes, neg, -0.5)     # 0 > -0.5: every record with parts matches
    assert got[0][0] == 1 and got[1][0] == 0.0
    _same(got, ref.best_overlap_def(heads, boxes, neg, -0.5))
    one = [(10, 0, 5, 3)]                                           # one side negative: area -16, o <= 0
    got = capi.candidates_best_overlap(heads, boxes, one, -0.5)
    _same(got, ref.best_overlap_def(heads, boxes, one, -0.5))
    assert got[0][0] == 1


def test_records_without_parts_and_with_different_part_counts():
    heads, boxes = _rec([(9.0, None), (1.0, SQUARE), (3.0, [(1, 1), (2, 2), (2, 1)]), (2.0, [(2, 2)])])
    assert list(heads["nparts"]) == [0, 2, 3, 1]
    gt = [(0, 0, 3, 3)]
    got = capi.candidates_best_overlap(heads, boxes, gt, 0.2)       # the one-part record's inter is 1: o = 1 / 16
    assert got[0][0] == 2 and got[1][0] == 0.25
    _same(got, ref.best_overlap_def(heads, boxes, gt, 0.2))
    got = capi.candidates_best_overlap(heads, boxes, gt, -1.0)      # even then the record without parts matches nothing
    assert got[0][0] == 2
    clean = boxes.copy()
    clean[boxes == 123456789] = 0
    _same(capi.candidates_best_overlap(heads, clean, gt, 0.2), capi.candidates_best_overlap(heads, boxes, gt, 0.2), "junk beyond nparts")
    only = _rec([(9.0, None)])
    assert capi.candidates_best_overlap(*only, gt, -1.0)[0][0] == -1


def test_two_boxes_one_record_and_the_box_counts():
    heads, boxes = _rec([(1.0, SQUARE), (4.0, [(1, 2), (2, 1)])])
    got = capi.candidates_best_overlap(heads, boxes, [(0, 0, 3, 3), (1, 1, 2, 4)], 0.2)
    assert list(got[0]) == [1, 1] and list(got[1]) == [0.25, 0.5]
    best, o = capi.candidates_best_overlap(heads, boxes, np.zeros((0, 4)), 0.2)
    assert len(best) == 0 and len(o) == 0
    heads, boxes = ref.records(5, 400, 3, nparts=np.random.default_rng(5).integers(0, 4, 400), distinct=False)
    gts = ref.gt_boxes(6, capi.PBD_GT_MAX)
    got = capi.candidates_best_overlap(heads, boxes, gts, 0.1)
    _same(got, ref.best_overlap_def(heads, boxes, gts, 0.1))
    assert (got[0] >= 0).sum() > 10
    none = capi.candidates_best_overlap(heads[:0], boxes[:0], gts, 0.1)   # count == 0: PBD_OK, nothing found
    assert (none[0] == -1).all() and not none[1].any()


def _rc(heads, boxes, gt, ngt, overlap, count=None, mp=None, best=True, o=True):
    L = capi.lib()
    out_b = np.zeros(capi.PBD_GT_MAX + 1, np.int32)
    out_o = np.zeros(capi.PBD_GT_MAX + 1, np.float64)
    gt = None if gt is None else np.ascontiguousarray(gt, np.float64)
    return L.pbd_candidates_best_overlap(None if heads is None else heads.ctypes.data_as(C.c_void_p), capi._p(boxes, C.c_int32),
                                         len(heads) if count is None else count, boxes.shape[1] if mp is None else mp,
                                         capi._p(gt, C.c_double), ngt, C.c_double(overlap),
                                         capi._p(out_b, C.c_int32) if best else None, capi._p(out_o, C.c_double) if o else None)


def test_argument_refusals():
    heads, boxes = _rec([(1.0, SQUARE), (2.0, SQUARE)])
    gt = np.array([[0.0, 0, 3, 3]])
    assert _rc(heads, boxes, gt, 1, 0.3) == capi.PBD_OK
    for k in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            g = gt.copy(); g[0, k] = bad
            assert _rc(heads, boxes, g, 1, 0.3) == capi.PBD_ERR_ARG
    for ov in (np.nan, np.inf, -np.inf):
        assert _rc(heads, boxes, gt, 1, ov) == capi.PBD_ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        h = heads.copy(); h["score"][1] = bad
        assert _rc(h, boxes, gt, 1, 0.3) == capi.PBD_ERR_ARG
    for bad in (-1, boxes.shape[1] + 1):
        h = heads.copy(); h["nparts"][0] = bad
        assert _rc(h, boxes, gt, 1, 0.3) == capi.PBD_ERR_ARG
    many = np.tile(gt, (capi.PBD_GT_MAX + 1, 1))
    assert _rc(heads, boxes, many, capi.PBD_GT_MAX, 0.3) == capi.PBD_OK
    assert _rc(heads, boxes, many, capi.PBD_GT_MAX + 1, 0.3) == capi.PBD_ERR_ARG
    assert _rc(heads, boxes, gt, -1, 0.3) == capi.PBD_ERR_ARG
    assert _rc(heads, boxes, gt, 1, 0.3, count=-1) == capi.PBD_ERR_ARG
    assert _rc(heads, boxes, gt, 1, 0.3, mp=0) == capi.PBD_ERR_ARG
    assert _rc(None, boxes, gt, 1, 0.3, count=2) == capi.PBD_ERR_ARG        # NULL where a size is positive
    assert _rc(heads, None, gt, 1, 0.3, mp=3) == capi.PBD_ERR_ARG
    assert _rc(heads, boxes, None, 1, 0.3) == capi.PBD_ERR_ARG
    assert _rc(heads, boxes, gt, 1, 0.3, best=False) == capi.PBD_ERR_ARG
    assert _rc(heads, boxes, gt, 1, 0.3, o=False) == capi.PBD_ERR_ARG
    assert _rc(None, None, gt, 1, 0.3, count=0, mp=3) == capi.PBD_OK        # ... and only there
    assert _rc(heads, boxes, None, 0, 0.3, best=False, o=False) == capi.PBD_OK


def test_exported_names_and_the_null_handle():
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert capi.PBD_GT_MAX == 64
    heads, boxes = _rec([(1.0, SQUARE)])
    gt = np.array([[0.0, 0, 3, 3]])
    best = np.zeros(1, np.int32); o = np.zeros(1, np.float64)
    rc = L.pbd_candidates_select_gt(None, capi._p(gt, C.c_double), 1, C.c_double(0.3), heads.ctypes.data_as(C.c_void_p),
                                    capi._p(boxes, C.c_int32), 1, capi._p(best, C.c_int32), capi._p(o, C.c_double))
    assert rc == capi.PBD_ERR_ARG
