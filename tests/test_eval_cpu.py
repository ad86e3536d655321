"""The evaluation ledger's definitions without a GPU (include/pbd_c.h "evaluation ledger"): the numpy form of the definitions against the
three MATLAB files restated line by line (tests/eval_ref.py), the C host functions (pbd_eval_host.cpp) against the definitions bit for
bit, hand-made cases for every rule, and the plumbing: refusals, declared = exported = bound symbols, the ABI version."""
import os
import re

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from tests import eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP = 6
COUNTS = [40, 0, 65, 17, 30, 1]
NGTS = [3, 2, 7, 0, 64, 1]


def _same(a, b):
    """bit for bit, NaN compared by isnan"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return a[ok].tobytes() == b[ok].tobytes()


def _head(score, P):
    h = np.zeros(len(score), ref.HEAD_DTYPE)
    h["score"] = score
    h["nparts"] = P
    return h


def _ledger(frames, P, thresh):
    """the definition's ledger of a list of frames: score [M], tp [M, P], npos"""
    tps = [ref.match_frame(f["heads"], f["boxes"], f["points"], f["scale"], P, thresh) for f in frames]
    score = np.concatenate([f["heads"]["score"] for f in frames]) if frames else np.zeros(0, np.float32)
    return score, (np.concatenate(tps) if tps else np.zeros((0, P), np.uint8)), sum(len(f["scale"]) for f in frames)


@pytest.fixture(scope="module", params=[(1, 11), (5, 12), (26, 13)], ids=["P1", "P5", "P26"])
def case(request):
    P, seed = request.param
    frames = ref.random_frames(seed, P, max(P, MP), COUNTS, NGTS)
    return P, frames, _ledger(frames, P, .5)


# ---- the definition against the MATLAB restatement ------------------------------------------------------------------------------------
def test_random_cases_are_not_vacuous(case):
    """asserted on the reference's output alone: true positives, misses by distance, double detections, empty frames, scores tied
    across frames"""
    P, frames, _ = case
    tp = fp_far = fp_dup = 0
    for p in range(P):
        for f in frames:
            ngt, count = len(f["scale"]), len(f["heads"])
            if not ngt or not count:
                continue
            ca = [dict(score=float(f["heads"]["score"][i]), fr=1, point=ref.keypoints(f["boxes"][i, p])) for i in range(count)]
            gt = [dict(numgt=ngt, point=f["points"][:, p], scale=f["scale"])]
            flags = ref.eval_apk_m(ca, gt)[3]
            tp += int(flags.sum())
            q = np.stack([ref.dist(c["point"][None], gt[0]["point"]) / f["scale"] for c in ca])   # [count, ngt]
            near = q.min(axis=1) <= .5
            fp_far += int((~near).sum())
            fp_dup += int((near & (flags == 0)).sum())
    assert tp > 10 and fp_far > 10 and fp_dup > 5, (tp, fp_far, fp_dup)
    assert any(len(f["scale"]) == 0 and len(f["heads"]) > 0 for f in frames)
    s0, s2 = frames[0]["heads"]["score"], frames[2]["heads"]["score"]
    assert len(np.intersect1d(s0, s2)) > 2
    assert any((np.signbit(f["heads"]["score"]) & (f["heads"]["score"] == 0)).any() for f in frames)


def test_definition_is_the_matlab_files(case):
    """per keypoint: eval_apk.m over all frames at once — flags, cumulative counts, rec and prec in bits, ap within (M + 1) 2^-53 (every
    partial sum lies in [0, 1], each of the M + 1 additions in either order errs by at most 2^-54)"""
    P, frames, (score, tp, npos) = case
    apk, prec, rec, tpc, order = ref.ap(score, tp, npos)
    M = len(score)
    for p in range(P):
        ca, gt = [], []
        for fi, f in enumerate(frames):
            gt.append(dict(numgt=len(f["scale"]), point=f["points"][:, p], scale=f["scale"]))
            ca += [dict(score=float(f["heads"]["score"][i]), fr=fi + 1, point=ref.keypoints(f["boxes"][i, p])) for i in range(len(f["heads"]))]
        m_ap, m_prec, m_rec, m_flags, m_tpc, m_fpc, m_si = ref.eval_apk_m(ca, gt)
        assert np.array_equal(m_flags, tp[:, p]), p
        assert np.array_equal(m_si, order)
        assert np.array_equal(m_tpc, tpc[p]) and np.array_equal(m_fpc, np.arange(1, M + 1) - tpc[p])
        assert _same(m_rec, rec[p]) and _same(m_prec, prec[p])
        assert abs(m_ap - apk[p]) <= (M + 1) * 2.0 ** -53, (p, m_ap, apk[p])
    assert 0 < apk.min() and apk.max() < 1


def test_pck_definition_is_eval_pck(case):
    P, frames, _ = case
    rng = np.random.default_rng(P)
    ca, gt = [], []
    for f in frames:
        for g in range(len(f["scale"])):
            pts = f["points"][g]
            pose = pts + rng.normal(0, .4 * f["scale"][g], pts.shape).round(1)
            ca.append(dict(point=pose)); gt.append(dict(point=pts, scale=float(f["scale"][g])))
    d = np.stack([ref.dist(c["point"], g["point"]) for c, g in zip(ca, gt)])
    scale = np.array([g["scale"] for g in gt])
    assert len(np.unique(scale)) > 3
    got = ref.pck(d, scale, .5, ref.SCALE_LAST)
    assert _same(ref.eval_pck_m(ca, gt), got) and 0 < got.min() and got.max() < 1
    assert _same(ref.eval_pck_m(ca, gt, .2), got)                                  # nargin < 4: the file's thresh is always 0.5
    assert _same(ref.eval_pck_m(ca, gt, .2, literal_nargin=False), ref.pck(d, scale, .2, ref.SCALE_LAST))
    assert not _same(ref.pck(d, scale, .5, ref.SCALE_OWN), got)


# ---- the C host functions against the definition ----------------------------------------------------------------------------------------
def test_host_functions_are_the_definition(case):
    P, frames, (score, tp, npos) = case
    for f in frames:
        for thresh in (.5, .2):
            exp = ref.match_frame(f["heads"], f["boxes"], f["points"], f["scale"], P, thresh)
            got = capi.eval_apk_match_host(f["heads"], f["boxes"], f["points"], f["scale"], P, thresh)
            assert np.array_equal(got, exp), thresh
        for i in range(min(3, len(f["heads"]))):
            pts = f["points"][0] if len(f["scale"]) else np.zeros((P, 2))
            assert _same(capi.eval_keypoint_dist(f["boxes"][i, :P], pts), ref.dist(ref.keypoints(f["boxes"][i, :P]), pts))
    apk, prec, rec, _, _ = ref.ap(score, tp, npos)
    g_apk, g_prec, g_rec = capi.eval_ap_host(score, tp, npos, curves=True)
    assert _same(g_apk, apk) and _same(g_prec, prec) and _same(g_rec, rec)
    assert _same(capi.eval_ap_host(score, tp, npos), apk)
    rng = np.random.default_rng(7)
    d = rng.uniform(0, 20, (50, P)); d[::7] = np.inf
    scale = rng.integers(5, 40, 50).astype(np.float64)
    for rule in (ref.SCALE_LAST, ref.SCALE_OWN):
        for thresh in (.5, .1):
            assert _same(capi.eval_pck_host(d, scale, thresh, rule), ref.pck(d, scale, thresh, rule))


# ---- hand-made cases --------------------------------------------------------------------------------------------------------------------
def test_three_four_five():
    """scale 10, thresh .5: a distance of exactly 5 is a PCK miss (5 < 5), a hit one ulp above; .5 <= .5 is an APK true positive"""
    box = np.array([[0, 0, 4, 4]], np.int32)                                        # centre (1.5, 1.5)
    pt = np.array([[4.5, 5.5]])
    d = capi.eval_keypoint_dist(box, pt)
    assert d[0] == 5.0 and ref.dist(ref.keypoints(box), pt)[0] == 5.0
    up = np.nextafter(.5, 1.0)
    for fn in (capi.eval_pck_host, ref.pck):
        assert fn(d[None], [10.0], .5, ref.SCALE_OWN)[0] == 0.0
        assert fn(d[None], [10.0], up, ref.SCALE_OWN)[0] == 1.0
    boxes = np.zeros((1, MP, 4), np.int32); boxes[0, 0] = box[0]
    for fn in (capi.eval_apk_match_host, ref.match_frame):
        assert fn(_head([1.0], 1), boxes, pt[None], [10.0], 1, .5)[0, 0] == 1
        assert fn(_head([1.0], 1), boxes, pt[None], [10.0], 1, np.nextafter(.5, 0.0))[0, 0] == 0


def test_square_roots_and_half_integer_centres():
    """dx = dy = 1 and other non-squares: sqrt correctly rounded; even widths give half-integer centres, exactly"""
    boxes = np.array([[0, 0, 1, 1], [3, 7, 2, 4], [-5, 2, 6, 1], [10, 10, 12, 11]], np.int32)
    assert np.array_equal(ref.keypoints(boxes), [[0, 0], [3.5, 8.5], [-2.5, 2], [15.5, 15]])
    pts = np.array([[1.0, 1.0], [1.25, 2.0], [0.1, 0.7], [-3.0, 40.0]])
    d = capi.eval_keypoint_dist(boxes, pts)
    assert d[0] == np.sqrt(2.0) and _same(d, ref.dist(ref.keypoints(boxes), pts))
    import math
    assert [float(v) for v in d] == [math.sqrt((c[0] - p[0]) * (c[0] - p[0]) + (c[1] - p[1]) * (c[1] - p[1]))
                                     for c, p in zip(ref.keypoints(boxes), pts)]


def test_matching_rules():
    P = 1
    one = lambda c: [ref.box_around(c, 1, 1)] + [[0, 0, 0, 0]] * (MP - 1)
    # jmin tie: two persons at the same distance -> the first; the second detection on the taken gt is a false positive although
    # person 1 is as near
    pts = np.array([[[10.0, 10.0]], [[14.0, 10.0]]])
    boxes = np.array([one((12, 10)), one((12, 10)), one((14, 10))], np.int32)
    for fn in (capi.eval_apk_match_host, ref.match_frame):
        tp = fn(_head([3, 2, 1], P), boxes, pts, [10.0, 10.0], P, .5)
        assert tp[:, 0].tolist() == [1, 0, 1]
        # order by score, ties by position, -0.0 == +0.0: records 0 (+0.0) and 1 (-0.0) tie, 0 goes first; record 2 (0.5) before both
        tp = fn(_head([0.0, -0.0, .5], P), np.array([one((10, 10)), one((10, 10)), one((10, 10))], np.int32), pts[:1], [10.0], P, .5)
        assert tp[:, 0].tolist() == [0, 0, 1]
        tp = fn(_head([-0.0, 0.0, -1.0], P), np.array([one((10, 10)), one((10, 10)), one((10, 10))], np.int32), pts[:1], [10.0], P, .5)
        assert tp[:, 0].tolist() == [1, 0, 0]
        # no person: every detection is a false positive
        assert not fn(_head([1, 2], P), boxes[:2], np.zeros((0, 1, 2)), np.zeros(0), P, .5).any()


def test_scale_rules_and_unmatched_instances():
    d = np.array([[4.0, 9.0], [4.0, 9.0]])
    scale = np.array([10.0, 20.0])
    for fn in (capi.eval_pck_host, ref.pck):
        assert fn(d, scale, .5, ref.SCALE_LAST).tolist() == [1.0, 1.0]              # both against 20: 4 < 10, 9 < 10
        assert fn(d, scale, .5, ref.SCALE_OWN).tolist() == [1.0, .5]                # instance 0 against 10: 9 < 5 fails
        with_miss = np.concatenate([d, np.full((1, 2), np.inf)])
        assert fn(with_miss, [10.0, 20.0, 20.0], .5, ref.SCALE_LAST).tolist() == [2 / 3, 2 / 3]
        assert np.isnan(fn(np.zeros((0, 2)), np.zeros(0), .5, ref.SCALE_LAST)).all()   # N == 0


def test_average_precision_cases():
    # a precision curve that rises late: fp, tp, tp -> prec 0, 1/2, 2/3; the suffix maximum lifts the first two to 2/3
    score = np.array([3, 2, 1], np.float32)
    tp = np.array([[0], [1], [1]], np.uint8)
    apk, prec, rec = capi.eval_ap_host(score, tp, 2, curves=True)
    assert prec[0].tolist() == [0.0, .5, 2 / 3] and rec[0].tolist() == [0.0, .5, 1.0]
    assert apk[0] == (.5 - 0.0) * (2 / 3) + (1.0 - .5) * (2 / 3) and apk[0] > .5 * .5 + .5 * (2 / 3)
    assert _same(apk, ref.ap(score, tp, 2)[0]) and abs(ref.vocap_m(rec[0], prec[0]) - apk[0]) <= 4 * 2.0 ** -53
    # M == 0: ap = 0, whatever npos
    for npos in (0, 5):
        assert capi.eval_ap_host(np.zeros(0, np.float32), np.zeros((0, 2), np.uint8), npos).tolist() == [0.0, 0.0]
        assert ref.ap(np.zeros(0, np.float32), np.zeros((0, 2), np.uint8), npos)[0].tolist() == [0.0, 0.0]
    # npos == 0: rec = 0 / 0 = NaN, and so is ap, as in MATLAB
    apk, prec, rec = capi.eval_ap_host(score, np.zeros((3, 1), np.uint8), 0, curves=True)
    assert np.isnan(apk).all() and np.isnan(rec).all() and not prec.any()
    assert np.isnan(ref.ap(score, np.zeros((3, 1), np.uint8), 0)[0]).all() and np.isnan(ref.vocap_m(rec[0], prec[0]))
    # tied and signed-zero scores: the sequence decides
    score = np.array([0.0, -0.0, 0.0, 1.0], np.float32)
    tp = np.array([[1], [0], [1], [0]], np.uint8)
    apk, prec, rec = capi.eval_ap_host(score, tp, 2, curves=True)
    assert prec[0].tolist() == [0.0, .5, 1 / 3, .5] and rec[0].tolist() == [0.0, .5, .5, 1.0]
    assert _same(apk, ref.ap(score, tp, 2)[0]) and _same(prec, ref.ap(score, tp, 2)[1])
    assert ref.ap(score, tp, 2)[4].tolist() == [3, 0, 1, 2]


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(capi.PbdError) as e:
        fn()
    return e.value.code


def test_host_refusals():
    h, b = _head([1.0], 1), np.zeros((1, MP, 4), np.int32)
    pts, sc = np.zeros((1, 1, 2)), np.array([10.0])
    A = capi.PBD_ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        assert _code(lambda: capi.eval_apk_match_host(h, b, np.full((1, 1, 2), bad), sc, 1)) == A
        assert _code(lambda: capi.eval_apk_match_host(h, b, pts, [bad], 1)) == A
        assert _code(lambda: capi.eval_apk_match_host(_head([bad], 1), b, pts, sc, 1)) == A
        assert _code(lambda: capi.eval_apk_match_host(h, b, pts, sc, 1, bad)) == A
        assert _code(lambda: capi.eval_keypoint_dist(b[0, :1], [[bad, 0.0]])) == A
        assert _code(lambda: capi.eval_pck_host(np.ones((1, 1)), [10.0], bad)) == A
        assert _code(lambda: capi.eval_pck_host(np.ones((1, 1)), [bad], .5)) == A
        assert _code(lambda: capi.eval_ap_host([bad], np.zeros((1, 1), np.uint8), 1)) == A
    for bad in (0.0, -1.0):
        assert _code(lambda: capi.eval_apk_match_host(h, b, pts, [bad], 1)) == A
        assert _code(lambda: capi.eval_pck_host(np.ones((1, 1)), [bad], .5)) == A
    assert _code(lambda: capi.eval_pck_host(np.full((1, 1), np.nan), [10.0], .5)) == A
    assert _code(lambda: capi.eval_pck_host(np.ones((1, 1)), [10.0], .5, 2)) == A
    assert _code(lambda: capi.eval_apk_match_host(_head([1.0], 2), b, pts, sc, 1)) == A            # nparts != P
    assert _code(lambda: capi.eval_apk_match_host(h, b, np.zeros((65, 1, 2)), np.ones(65), 1)) == A  # ngt > PBD_GT_MAX
    assert _code(lambda: capi.eval_ap_host([1.0], np.zeros((1, 1), np.uint8), -1)) == A
    assert capi.eval_apk_match_host(h, b, np.zeros((64, 1, 2)), np.ones(64), 1).shape == (1, 1)


def test_symbols_declared_exported_bound():
    text = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"^(?:int|void) (pbd_eval_\w+)\(", text, re.M))
    assert len(declared) == 17, sorted(declared)
    assert declared == {n for n in capi.EXPORTS if n.startswith("pbd_eval_")}
    L = capi.lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None, name
    assert L.pbd_abi_version() == 5 == capi.PBD_ABI_VERSION and "#define PBD_ABI_VERSION 5" in text
    for name in ("add_pck_records", "add_apk_records", "pck_frame", "pck_batch", "apk_frame", "apk_batch", "pck", "apk", "reset", "get", "dims"):
        assert callable(getattr(capi.Eval, name))
    from partsbaseddetector_amd import PartsBasedDetector
    from partsbaseddetector_amd.detector import Evaluation
    assert callable(PartsBasedDetector.evaluation)
    for name in ("addPck", "addPckBatch", "addApk", "addApkBatch", "pck", "apk", "reset"):
        assert callable(getattr(Evaluation, name))
    host = open(os.path.join(ROOT, "partsbaseddetector_amd", "host", "pbd_host.hpp")).read()
    assert "class Evaluation" in host and all(f"pbd_eval_{n}(" in host for n in ("create", "destroy", "pck", "apk", "reset"))
