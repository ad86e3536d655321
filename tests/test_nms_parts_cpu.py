"""The part-wise overlap NMS of matlab/detection/nms.m (pbd_candidates_nms_parts, pbd_set_candidate_nms, pbd_candidates_filter_parts):
the definition against a restatement of nms.m, the host function against the definition, and the C ABI surface — no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from partsbaseddetector_amd import capi

from tests import nms_parts_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbd_candidates_nms_parts", "pbd_set_candidate_nms", "pbd_group_set_candidate_nms", "pbd_candidates_filter_parts")
OVERLAPS = (-0.5, 0.0, 0.3, 1.0, 3.0)


def make(parts, scores=None):
    """records from a list of part-box lists [(x, y, w, h), ...], in the given (already sorted) order; level = the index"""
    n, mp = len(parts), max(1, max(len(p) for p in parts))
    heads = np.zeros(n, capi.HEAD_DTYPE)
    heads["score"] = np.arange(n, 0, -1, dtype=np.float32) if scores is None else np.asarray(scores, np.float32)
    heads["level"] = np.arange(n)
    heads["nparts"] = [len(p) for p in parts]
    boxes = np.full((n, mp, 4), 12345, np.int32)   # (junk beyond nparts)
    for i, p in enumerate(parts):
        for q, b in enumerate(p):
            boxes[i, q] = b
    return heads, boxes, np.zeros((n, mp, 3), np.int32)


def host(recs, overlap, top):
    return [int(v) for v in capi.candidates_nms_parts(*recs, overlap, top)[0]["level"]]


def both(recs, overlap, top=0):
    """kept indices by the definition; the host function must agree"""
    d = ref.nms_parts_def(recs[0], recs[1], overlap, top)
    assert host(recs, overlap, top) == d, (overlap, top)
    return d


# ---- the definition against nms.m, where nms.m is defined ------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("n", [300, 1100])
def test_definition_matches_nms_m(P, n):
    rng = np.random.default_rng(100 * P + n)
    heads = np.zeros(n, capi.HEAD_DTYPE)
    heads["score"] = rng.permutation(n).astype(np.float32) * 0.25 - 7   # distinct
    heads["level"] = np.arange(n)
    heads["nparts"] = P
    boxes = np.zeros((n, P, 4), np.int32)
    root = rng.integers(0, 400, (n, 1, 2))
    boxes[..., :2] = root + rng.integers(-30, 30, (n, P, 2))
    boxes[..., 2:] = rng.integers(8, 60, (n, P, 2))                     # non-empty
    locs = np.zeros((n, P, 3), np.int32)
    mat = np.zeros((n, 4 * P + 2))
    for p in range(P):
        mat[:, 4 * p + 0] = boxes[:, p, 0]
        mat[:, 4 * p + 1] = boxes[:, p, 1]
        mat[:, 4 * p + 2] = boxes[:, p, 0] + boxes[:, p, 2] - 1         # x2 = x + w - 1
        mat[:, 4 * p + 3] = boxes[:, p, 1] + boxes[:, p, 3] - 1
    mat[:, -1] = heads["score"]
    srt = capi.candidates_sort(heads, boxes, locs)
    assert len(set(heads["score"])) == n
    for ov in (0.0, 0.3, 0.7):
        pick = ref.nms_m(mat, float(np.float32(ov)))   # (the library takes the overlap as a float)
        d = ref.nms_parts_def(srt[0], srt[1], ov, 1000)
        assert [int(srt[0]["level"][i]) for i in d] == pick, ov
        assert host(srt, ov, 1000) == pick, ov
        assert 1 < len(pick) < min(n, 1000)
    if n > 1000:   # the cap fired: the record ranked 1001st and beyond is gone, whatever it overlaps
        assert max(ref.nms_parts_def(srt[0], srt[1], 0.7, 1000)) < 1000 <= max(ref.nms_parts_def(srt[0], srt[1], 0.7, 0))


# ---- hand-made pairs --------------------------------------------------------------------------------------------------------
def test_divisor_is_the_kept_records_area():
    small, large = [(10, 10, 4, 4)], [(0, 0, 100, 100)]
    assert both(make([small, large]), 0.3) == [0]          # 16 / 16
    assert both(make([large, small]), 0.3) == [0, 1]       # 16 / 10000


def test_union_boxes_and_parts():
    a = [(0, 0, 10, 10), (90, 90, 10, 10)]
    b = [(90, 0, 10, 10), (0, 90, 10, 10)]
    assert both(make([a, b]), 0.3) == [0]                  # disjoint parts, equal covering boxes: the covering box rejects
    c = [(200, 0, 10, 10), (290, 90, 10, 10)]
    assert both(make([a, c]), 0.3) == [0, 1]               # disjoint covering boxes: nothing can meet
    assert both(make([a, c]), -0.5) == [0]                 # ... and 0 / area > -0.5


def test_a_single_coinciding_part_rejects():
    a = [(0, 0, 10, 10), (50, 50, 10, 10), (0, 100, 10, 10)]
    b = [(200, 0, 10, 10), (50, 50, 10, 10), (200, 100, 10, 10)]
    c = [(200, 0, 10, 10), (56, 50, 10, 10), (200, 100, 10, 10)]
    assert both(make([a, b]), 0.3) == [0]                  # covering boxes: 1100 / 6600; part 1: 100 / 100
    assert both(make([a, c]), 0.45) == [0, 1]              # part 1: 40 / 100


def test_strictly_greater():
    recs = make([[(0, 0, 4, 4)], [(0, 0, 2, 2)]])          # 4 / 16 = 0.25 exactly
    assert both(recs, 0.25) == [0, 1]
    assert both(recs, float(np.nextafter(np.float32(0.25), np.float32(0)))) == [0]


def test_empty_boxes_and_no_parts():
    e = [(5, 5, 0, 10)]
    full = [(0, 0, 20, 20)]
    for ov in OVERLAPS:
        assert both(make([e, full, e]), ov) == ([0, 1] if ov < 0 else [0, 1, 2])   # a kept empty record rejects nothing (0 / 0); 0 / 400 > ov
        assert both(make([[], full, []]), ov) == ([0, 1] if ov < 0 else [0, 1, 2])
        assert both(make([[], []]), ov) == [0, 1]
    assert both(make([full, e]), 0.0) == [0, 1]            # 0 / 400 > 0 is false
    assert both(make([[(0, 0, 10, 10), (3, 3, -1, 5)], [(0, 0, 10, 10), (3, 3, 5, 5)]]), 0.3) == [0]


def test_mixed_part_counts_compare_common_leading_parts():
    a = [(0, 0, 10, 10), (100, 0, 10, 10), (200, 0, 10, 10)]
    assert both(make([a, [(0, 0, 10, 10)]]), 0.3) == [0]                       # part 0 coincides
    assert both(make([a, [(200, 0, 10, 10)]]), 0.3) == [0, 1]                  # part 2's place, but compared as part 0; covers: 100 / 2100
    assert both(make([[(200, 0, 10, 10)], a]), 0.3) == [0]                     # ... the other way: the covers, 100 / 100


def test_signed_zero_ties_keep_the_sort_order():
    parts = [[(0, 0, 10, 10)], [(300, 0, 10, 10)], [(0, 0, 10, 10)], [(300, 0, 10, 10)]]
    h, b, l = make(parts, scores=[0.0, -0.0, -0.0, 0.0])
    srt = capi.candidates_sort(h, b, l)
    assert list(srt[0]["level"]) == [0, 1, 2, 3]
    assert both(srt, 0.3) == [0, 1]


@pytest.mark.parametrize("ov", OVERLAPS)
def test_random_sets_caps_and_overlaps(ov):
    for seed, n, mp in ((1, 20, 5), (2, 64, 3), (3, 130, 1)):
        recs = capi.candidates_sort(*ref.records(seed, n, mp))
        recs[0]["level"] = np.arange(n)
        for top in (0, 1, 7, n - 1, n, n + 1):
            d = both(recs, ov, top)
            assert len(d) >= 1 and max(d) < (n if top == 0 else min(n, top))
            if ov >= 1:
                assert d == list(range(n if top == 0 else min(n, top)))


def test_junk_coordinates_do_not_overflow():
    m, M = -2**31, 2**31 - 1
    recs = make([[(m, m, M, M), (M, M, M, M)], [(M - 5, M - 5, M, M), (m, m, 7, 7)], [(m, m, 1, 1)]])
    for ov in OVERLAPS:
        both(recs, ov)
    assert both(recs, 0.3) == [0, 2]                       # (m, m, 7, 7) lies inside the first record's part 0
    assert both(make([[(M, M, M, M)], [(M, M, M, 3)]]), 0.3) == [0, 1] and both(make([[(M, M, M, 3)], [(M, M, M, M)]]), 0.3) == [0]


# ---- each clause matters: five slips in the reference each change a result ------------------------------------------------------
def test_slips_change_results():
    cases = {
        "later_area": (make([[(10, 10, 4, 4)], [(0, 0, 100, 100)]]), 0.3, 0),
        "ge": (make([[(0, 0, 4, 4)], [(0, 0, 2, 2)]]), 0.25, 0),
        "no_cover": (make([[(0, 0, 10, 10), (90, 90, 10, 10)], [(90, 0, 10, 10), (0, 90, 10, 10)]]), 0.3, 0),
        "area_minus_one": (make([[(0, 0, 4, 4)], [(0, 0, 2, 2)]]), 0.3, 0),
        "cap_after": (make([[(0, 0, 10, 10)], [(1, 1, 10, 10)], [(300, 300, 10, 10)]]), 0.3, 2),
    }
    assert set(cases) == set(ref.SLIPS)
    for slip, (recs, ov, top) in cases.items():
        good = both(recs, ov, top)
        assert ref.nms_parts_def(recs[0], recs[1], ov, top, slip=slip) != good, slip


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"\b(pbd_[a-z0-9_]+)\s*\(", hdr))
    tune = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libpbd_hip_tune.so"))
    for name in NAMES:
        assert name in declared
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name) and hasattr(tune, name)
    assert "PBD_NMS_PAINTED = 0, PBD_NMS_PARTS = 1" in hdr
    assert (capi.PBD_NMS_PAINTED, capi.PBD_NMS_PARTS) == (0, 1)
    for cls in (capi.Handle, capi.Group):
        assert hasattr(cls, "set_candidate_nms")
    assert hasattr(capi.Handle, "candidates_filter_parts") and hasattr(capi, "candidates_nms_parts")


def test_abi_version_still_5():
    assert capi.lib().pbd_abi_version() == 5 == capi.PBD_ABI_VERSION


def test_null_handle_and_argument_errors():
    L = capi.lib()
    for kind in (0, 1, 2, -1):
        assert L.pbd_set_candidate_nms(None, kind, 1000) == capi.PBD_ERR_ARG
        assert L.pbd_group_set_candidate_nms(None, kind, 1000) == capi.PBD_ERR_ARG
    heads = (capi.pbd_candidate_head * 2)()
    boxes = (C.c_int32 * 8)()
    kept = C.c_int(-1)
    assert L.pbd_candidates_filter_parts(None, C.c_float(0.3), 1000, heads, boxes, None, 2, C.byref(kept)) == capi.PBD_ERR_ARG
    f = L.pbd_candidates_nms_parts
    assert f(heads, boxes, None, 2, 1, C.c_float(0.3), 1000, C.byref(kept)) == capi.PBD_OK and kept.value == 2
    kept.value = -1
    for args in ((None, boxes, None, 2, 1, C.c_float(0.3), 0, C.byref(kept)), (heads, None, None, 2, 1, C.c_float(0.3), 0, C.byref(kept)),
                 (heads, boxes, None, 2, 1, C.c_float(0.3), 0, None), (heads, boxes, None, -1, 1, C.c_float(0.3), 0, C.byref(kept)),
                 (heads, boxes, None, 2, 0, C.c_float(0.3), 0, C.byref(kept)), (heads, boxes, None, 2, 1, C.c_float(0.3), -1, C.byref(kept)),
                 (heads, boxes, None, 2, 1, C.c_float(float("nan")), 0, C.byref(kept)),
                 (heads, boxes, None, 2, 1, C.c_float(float("inf")), 0, C.byref(kept))):
        assert f(*args) == capi.PBD_ERR_ARG
    heads[1].nparts = 2
    assert f(heads, boxes, None, 2, 1, C.c_float(0.3), 0, C.byref(kept)) == capi.PBD_ERR_ARG
    assert kept.value == -1


def test_detector_exposes_the_setting():
    from partsbaseddetector_amd import Candidate, PartsBasedDetector
    det = PartsBasedDetector(cand_nms=(capi.PBD_NMS_PARTS, 1000))
    assert det._cand_nms == (capi.PBD_NMS_PARTS, 1000)
    det.setCandidateNms(capi.PBD_NMS_PARTS, 7)   # before distributeModel: remembered for the handle
    assert det._cand_nms == (capi.PBD_NMS_PARTS, 7)
    for bad in ((2, 0), (1, -1)):
        with pytest.raises(capi.PbdError) as e:
            det.setCandidateNms(*bad)
        assert e.value.code == capi.PBD_ERR_ARG
    assert hasattr(Candidate, "nonMaximaSuppressionParts")
    host = open(os.path.join(ROOT, "partsbaseddetector_amd", "host", "pbd_host.hpp")).read()
    assert "void setCandidateNms(int kind, int top" in host
    assert "static void nonMaximaSuppressionParts(std::vector<Candidate>& c, float overlap" in host
