"""The evaluation ledger on the device (k_eval.hip; include/pbd_c.h "evaluation ledger") against the host functions, which
tests/test_eval_cpu.py holds to the definitions and to the MATLAB files: the stand-alone adds, accumulation and the results (past the
global sort's LDS tile too), the whole-path adds against plain detect + stand-alone add, isolation, capacity, refusals, the bindings.
Everything is compared by bytes; NaN by isnan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import PERSON_TREE, make_image, make_tree_model
from tests import eval_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER_TILE = 256    # PBD_EVAL_ORDER_TILE: keys of a frame's ordering staged in LDS at a time
SORT_TILE = 1024    # PBD_EVAL_SORT_TILE: keys the global sort orders inside one workgroup
W, H = 160, 120
OVERLAP = 0.3
TREES = {1: ([-1], 2), 5: ([-1, 0, 1, 1, 0], 3), 26: (PERSON_TREE, 1)}


def _code(fn):
    with pytest.raises(capi.PbdError) as e:
        fn()
    return e.value


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return a[ok].tobytes() == b[ok].tobytes()


def _ledgers_equal(a, b):
    ga, gb = a.get(), b.get()
    return a.dims() == b.dims() and all(ga[k].tobytes() == gb[k].tobytes() for k in ("dist", "scale", "score", "tp"))


def _assert_results(ev):
    """pbd_eval_pck (both rules, two thresholds) and pbd_eval_apk (with the curves) = the host functions on the ledger's own arrays"""
    P, N, M, npos, _ = ev.dims()
    g = ev.get()
    for rule in (capi.PBD_EVAL_SCALE_LAST, capi.PBD_EVAL_SCALE_OWN):
        for thresh in (.5, .15):
            assert _same(ev.pck(thresh, rule), capi.eval_pck_host(g["dist"], g["scale"], thresh, rule)), (rule, thresh)
    apk, prec, rec = ev.apk(curves=True)
    e_apk, e_prec, e_rec = capi.eval_ap_host(g["score"], g["tp"], npos, curves=True)
    assert _same(apk, e_apk) and _same(prec, e_prec) and _same(rec, e_rec), (apk, e_apk)
    assert _same(ev.apk(), e_apk)
    return apk


@pytest.fixture(scope="module")
def handles():
    hs = {P: capi.Handle(make_tree_model(par, K, seed=5, kh=3, kw=3), conv_mode=capi.PBD_CONV_EXACT) for P, (par, K) in TREES.items()}
    yield hs
    for h in hs.values():
        h.close()


def _pck_records(rng, f, P, mp):
    """per person of frame f a pose slot: found or not, the pose a noisy copy of the person"""
    ngt = len(f["scale"])
    heads = np.zeros(ngt, ref.HEAD_DTYPE); heads["nparts"] = P
    boxes = np.zeros((ngt, mp, 4), np.int32)
    found = (rng.random(ngt) < .7).astype(np.int32)
    for g in range(ngt):
        for p in range(P):
            boxes[g, p] = ref.box_around(f["points"][g, p] + rng.normal(0, .4 * f["scale"][g], 2), rng.integers(1, 13), rng.integers(1, 13))
    return heads, boxes, found


# ---- the stand-alone adds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 5, 26])
def test_standalone_adds_are_the_host_functions(gpu_required, handles, P):
    """record counts 0, 1, 63, 64, 65 and one below, at and one above the ordering's tile; ngt 0, 1, 2, 63, 64; scores tied inside and
    across frames with both zeros (random_frames); frame after frame into one ledger"""
    h = handles[P]
    assert h.max_parts == P
    counts = [0, 1, 63, 64, 65, ORDER_TILE - 1, ORDER_TILE, ORDER_TILE + 1, 40]
    ngts = [2, 0, 1, 64, 63, 2, 5, 0, 64]
    frames = ref.random_frames(100 + P, P, P, counts, ngts)
    assert any((np.signbit(f["heads"]["score"]) & (f["heads"]["score"] == 0)).any() for f in frames)
    ev = capi.Eval(h, P, sum(ngts), sum(counts))
    rng = np.random.default_rng(P)
    e_tp, e_dist = [], []
    for f in frames:
        ev.add_apk_records(f["heads"], f["boxes"], f["points"], f["scale"])
        e_tp.append(capi.eval_apk_match_host(f["heads"], f["boxes"], f["points"], f["scale"], P, .5))
        heads, boxes, found = _pck_records(rng, f, P, P)
        ev.add_pck_records(heads, boxes, found, f["points"], f["scale"])
        for g in range(len(found)):
            e_dist.append(capi.eval_keypoint_dist(boxes[g, :P], f["points"][g]) if found[g] else np.full(P, np.inf))
    got = ev.get()
    e_tp = np.concatenate(e_tp)
    assert ev.dims() == (P, sum(ngts), sum(counts), sum(ngts), 2 * len(frames))
    assert got["tp"].tobytes() == e_tp.tobytes() and 0 < e_tp.mean() < 1
    assert got["score"].tobytes() == np.concatenate([f["heads"]["score"] for f in frames]).tobytes()
    assert got["dist"].tobytes() == np.stack(e_dist).tobytes() and np.isinf(got["dist"]).any() and np.isfinite(got["dist"]).any()
    assert got["scale"].tobytes() == np.concatenate([f["scale"] for f in frames]).tobytes()
    apk = _assert_results(ev)
    assert 0 < apk.min() and apk.max() < 1
    ev.reset()
    assert ev.dims() == (P, 0, 0, 0, 0) and np.isnan(ev.pck()).all() and not ev.apk().any()
    ev.close()


def test_square_roots_on_the_device(gpu_required, handles):
    """v_rsq_f64 + FMA corrections must give the correctly rounded root: non-squares (dx = dy = 1, thirds, large and tiny magnitudes)
    against the host's sqrt, bit for bit"""
    h = handles[1]
    rng = np.random.default_rng(3)
    n = 64
    pts = np.concatenate([[[1.0, 1.0]], rng.uniform(-1e3, 1e3, (20, 2)), rng.uniform(-1e-3, 1e-3, (20, 2)) / 3.0,
                          rng.uniform(-1e150, 1e150, (13, 2)), rng.uniform(-1e-150, 1e-150, (10, 2))])[:n, None, :]
    heads = np.zeros(n, ref.HEAD_DTYPE); heads["nparts"] = 1
    boxes = np.zeros((n, 1, 4), np.int32); boxes[:, 0, 2:] = 1                      # every keypoint at (0, 0)
    ev = capi.Eval(h, 1, n, 1)
    ev.add_pck_records(heads, boxes, np.ones(n, np.int32), pts, np.ones(n))
    d = ev.get()["dist"][:, 0]
    exp = np.array([capi.eval_keypoint_dist(boxes[i], pts[i])[0] for i in range(n)])
    assert d[0] == np.sqrt(2.0) and d.tobytes() == exp.tobytes()
    assert exp.tobytes() == np.sqrt(pts[:, 0, 0] * pts[:, 0, 0] + pts[:, 0, 1] * pts[:, 0, 1]).tobytes()
    ev.close()


# ---- accumulation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [[30, 0, 41], [600, SORT_TILE + 1 - 600], [900, 900, 700]], ids=["small", "tile+1", "two-global-steps"])
def test_accumulation_and_results(gpu_required, handles, counts):
    """synthetic frames through pbd_eval_add_apk_records, no detector: the results equal the host functions on the concatenation, also
    with M one past the sort's LDS tile and with two distances in device memory"""
    P = 5
    frames = ref.random_frames(sum(counts), P, P, counts, [3, 0, 9][:len(counts)])
    ev = capi.Eval(handles[P], P, 16, sum(counts))
    score, tp = [], []
    for f in frames:
        ev.add_apk_records(f["heads"], f["boxes"], f["points"], f["scale"])
        score.append(f["heads"]["score"])
        tp.append(capi.eval_apk_match_host(f["heads"], f["boxes"], f["points"], f["scale"], P, .5))
    got = ev.get()
    assert got["tp"].tobytes() == np.concatenate(tp).tobytes() and got["score"].tobytes() == np.concatenate(score).tobytes()
    apk = _assert_results(ev)
    assert _same(apk, capi.eval_ap_host(np.concatenate(score), np.concatenate(tp), 12 if len(counts) == 3 else 3))
    ev.close()


# ---- whole path -------------------------------------------------------------------------------------------------------------------------
def _model(orc, seed, im, pct):
    model = make_tree_model([-1, 0, 1, 1, 0], 3, seed=seed)
    model.thresh = -1e30
    fr = orc.detect(model, im, capacity=1, keep=True)[4]
    model.thresh = float(np.float32(np.percentile(np.concatenate([fr.root(l)[0].ravel() for l in range(fr.nlevels)]), pct)))
    fr.free()
    return model


def _persons_from(raw, ranks=(0, 9, 99)):
    """persons off a frame's records: the part centres of the records of these ranks by score, perturbed; one person where nothing is"""
    order = np.argsort(-raw[0]["score"].astype(np.float64), kind="stable")
    pts = [ref.keypoints(raw[1][order[r]][:5]) + np.array([.25, -.5]) * (1 + k) for k, r in enumerate(ranks)]
    pts.append(np.array([[5000.0 + 13 * p, 5000.0 + 7 * p] for p in range(5)]))
    return np.stack(pts), np.array([9.0, 14.0, 6.0, 11.0])[:len(pts)]


def _gt_boxes(points):
    p = np.asarray(points)
    return np.stack([p[..., 0].min(1), p[..., 1].min(1), p[..., 0].max(1), p[..., 1].max(1)], 1) if len(p) else np.zeros((0, 4))


@pytest.fixture(scope="module")
def scene(orc):
    frames = [make_image(61, W, H), make_image(62, W, H), make_image(63, W, H)]
    return _model(orc, 91, frames[0], 70.0), frames


def _filtered(hd, on):
    if on:
        hd.set_candidate_nms(capi.PBD_NMS_PARTS, 1000)
        hd.set_candidate_filter(capi.PBD_CAND_SORT_NMS, 0.3)
    else:
        hd.set_candidate_filter(capi.PBD_CAND_RAW)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_whole_path_is_detect_plus_standalone_add(gpu_required, scene, dtype):
    model, frames = scene
    hd = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, max_candidates=16384)
    raws = [hd.detect(f, 16384) for f in frames]
    assert all(len(r[0]) > 100 for r in raws)
    persons = [_persons_from(raws[0]), _persons_from(raws[1], (4,)), (np.zeros((0, 5, 2)), np.zeros(0))]
    # not vacuous, on the plain detect's output: matches and misses, for both protocols
    tp0 = capi.eval_apk_match_host(raws[0][0], raws[0][1], *persons[0], 5)
    best0 = capi.candidates_best_overlap(raws[0][0], raws[0][1], _gt_boxes(persons[0][0]), OVERLAP)[0]
    assert tp0.any() and not tp0.all() and (best0 >= 0).sum() >= 2 and best0[3] == -1
    total = sum(len(p[1]) for p in persons)
    # PCK: the ledger after the frame entry = pbd_detect_gtbox_u8 + pbd_eval_add_pck_records
    a, b = capi.Eval(hd, 5, 64, 40000), capi.Eval(hd, 5, 64, 40000)
    efounds = []
    for f, (pts, sc) in zip(frames, persons):
        found = a.pck_frame(f, pts, sc, OVERLAP)
        heads, boxes, locs, efound, _ = hd.detect_gtbox(f, _gt_boxes(pts), OVERLAP)
        assert np.array_equal(found, efound) and a.records == hd.gt_records
        b.add_pck_records(heads, boxes, efound, pts, sc)
        efounds.append(list(efound))
    assert _ledgers_equal(a, b) and a.dims()[1] == total
    assert efounds[0] == list((best0 >= 0).astype(int)) and efounds[2] == []
    d = a.get()["dist"]
    assert np.isinf(d[3]).all() and all(np.isfinite(d[i]).all() == bool(fl) for i, fl in enumerate(efounds[0] + efounds[1]))
    c = capi.Eval(hd, 5, 64, 40000)
    founds = c.pck_batch(frames, persons, OVERLAP)
    assert c.get()["dist"].tobytes() == d.tobytes() and c.get()["scale"].tobytes() == a.get()["scale"].tobytes()
    assert [list(x) for x in founds] == efounds and c.dims()[4] == 3
    _assert_results(a)
    # APK: RAW, then testmodel.m's nms.m
    for filt in (False, True):
        _filtered(hd, filt)
        recs = [hd.detect(f, 16384) for f in frames]
        a.reset(); b.reset(); c.reset()
        for f, r, (pts, sc) in zip(frames, recs, persons):
            assert a.apk_frame(f, pts, sc) == len(r[0])
            b.add_apk_records(r[0], r[1], pts, sc)
        assert _ledgers_equal(a, b), filt
        assert a.dims() == (5, 0, sum(len(r[0]) for r in recs), total, 3)
        tp = a.get()["tp"]
        assert tp.any() and tp.sum(0).max() <= total
        assert list(c.apk_batch(frames, persons)) == [len(r[0]) for r in recs]
        assert c.get()["tp"].tobytes() == tp.tobytes() and c.get()["score"].tobytes() == a.get()["score"].tobytes(), filt
        apk = _assert_results(a)
        assert (apk > 0).any()
        if filt:
            assert len(recs[0][0]) < len(raws[0][0])
    for e in (a, b, c):
        e.close()
    hd.close()


# ---- isolation, capacity, refusals --------------------------------------------------------------------------------------------------------
def test_plain_frames_on_a_graph_handle_are_untouched(gpu_required, scene):
    model, frames = scene
    hd = capi.Handle(model, graph=1, max_candidates=8192)
    plain = [hd.detect(frames[0], 8192) for _ in range(3)]                       # eager, captured, replayed
    pts, sc = _persons_from(plain[0])
    ev = capi.Eval(hd, 5, 64, 8192)
    assert ev.apk_frame(frames[0], pts, sc) == len(plain[0][0])
    ev.pck_frame(frames[0], pts, sc, OVERLAP)
    after = [hd.detect(frames[0], 8192) for _ in range(2)]
    for other in plain[1:] + after:
        for k in range(3):
            assert np.asarray(other[k]).tobytes() == np.asarray(plain[0][k]).tobytes()
    b = capi.Eval(hd, 5, 64, 8192)
    b.add_apk_records(plain[0][0], plain[0][1], pts, sc)
    assert b.get()["tp"].tobytes() == ev.get()["tp"].tobytes()
    hd.close()


def test_capacity_and_refusals(gpu_required, scene):
    model, frames = scene
    im = frames[0]
    hd = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, max_candidates=8192)
    raw = hd.detect(im, 8192)
    n = len(raw[0])
    pts, sc = _persons_from(raw)
    # capacity: nothing is added, the needed count is reported
    ev = capi.Eval(hd, 5, 5, n + 9)
    ev.add_apk_records(raw[0][:10], raw[1][:10], pts, sc)
    before = ev.get()
    for call in (lambda: ev.apk_frame(im, pts, sc), lambda: ev.add_apk_records(raw[0], raw[1], pts, sc)):
        e = _code(call)
        assert e.code == capi.PBD_ERR_CAPACITY and e.needed == n + 10 and "nothing was added" in str(e)
        assert ev.dims() == (5, 0, 10, 4, 1) and ev.get()["tp"].tobytes() == before["tp"].tobytes()
    found = ev.pck_frame(im, pts, sc, OVERLAP)
    heads, boxes, _, efound, _ = hd.detect_gtbox(im, _gt_boxes(pts), OVERLAP)
    for call in (lambda: ev.pck_frame(im, pts, sc, OVERLAP), lambda: ev.add_pck_records(heads, boxes, efound, pts, sc)):
        e = _code(call)
        assert e.code == capi.PBD_ERR_CAPACITY and e.needed == 8
        assert ev.dims()[1] == 4
    assert np.array_equal(found, efound)
    ev.add_apk_records(raw[0][:n - 1], raw[1][:n - 1], pts[:0], sc[:0])            # exactly full is fine
    assert ev.dims()[2] == n + 9
    short = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, max_candidates=n - 1)
    es = capi.Eval(short, 5, 8, 2 * n)
    e = _code(lambda: es.apk_frame(im, pts, sc))
    assert e.code == capi.PBD_ERR_CAPACITY and es.records == [n] and es.dims()[2] == 0
    short.close()
    # arguments
    A = capi.PBD_ERR_ARG
    e = _code(lambda: capi.Eval(hd, 4, 8, 8))
    assert e.code == A and "parts" in str(e)
    for bad in ((0, 8, 8, .5), (5, 0, 8, .5), (5, 8, 0, .5), (5, 8, 8, float("nan"))):
        assert _code(lambda: capi.Eval(hd, *bad)).code == A
    m0 = ev.dims()
    wrong = raw[0][:3].copy(); wrong["nparts"][2] = 4
    e = _code(lambda: ev.add_apk_records(wrong, raw[1][:3], pts, sc))
    assert e.code == A and "nothing was added" in str(e)
    wrongp = heads.copy(); wrongp["nparts"][0] = 3
    assert _code(lambda: ev.add_pck_records(wrongp, boxes, np.ones(4, np.int32), pts, sc)).code == A
    nan = raw[0][:3].copy(); nan["score"][1] = np.nan
    assert _code(lambda: ev.add_apk_records(nan, raw[1][:3], pts, sc)).code == A
    for bad_sc in (0.0, -1.0, np.inf, np.nan):
        s2 = sc.copy(); s2[1] = bad_sc
        assert _code(lambda: ev.add_apk_records(raw[0][:3], raw[1][:3], pts, s2)).code == A
        assert _code(lambda: ev.apk_frame(im, pts, s2)).code == A
        assert _code(lambda: ev.pck_frame(im, pts, s2)).code == A
    p2 = pts.copy(); p2[0, 0, 0] = np.inf
    assert _code(lambda: ev.apk_frame(im, p2, sc)).code == A
    assert _code(lambda: ev.apk_frame(im, np.zeros((65, 5, 2)), np.ones(65))).code == A
    assert _code(lambda: ev.pck(float("inf"))).code == A and _code(lambda: ev.pck(.5, 2)).code == A
    assert ev.dims() == m0
    # settings and state
    big = capi.Eval(hd, 5, 64, 40000)
    assert _code(lambda: big.pck_frame(im, pts, sc, float("nan"))).code == A and big.dims() == (5, 0, 0, 0, 0)
    for on, off in ((lambda: hd.set_depth_filter(True), lambda: hd.set_depth_filter(False)),
                    (lambda: hd.set_box3d(True, (500.0, 500.0, 80.0, 60.0)), lambda: hd.set_box3d(False)),
                    (lambda: hd.set_part_scores(True), lambda: hd.set_part_scores(False))):
        on()
        e = _code(lambda: big.apk_frame(im, pts, sc))
        assert e.code == capi.PBD_ERR_UNSUPPORTED and "evaluation" in str(e)
        e = _code(lambda: big.pck_frame(im, pts, sc))
        assert e.code == capi.PBD_ERR_UNSUPPORTED and "gt boxes" in str(e)
        off()
    hd.set_candidate_filter(capi.PBD_CAND_SORT)
    assert _code(lambda: big.pck_frame(im, pts, sc)).code == capi.PBD_ERR_UNSUPPORTED   # the gt-box selection searches RAW records
    hd.set_candidate_filter(capi.PBD_CAND_RAW)
    hd._geo = hd.geometry(W, H)
    hd.enqueue(np.ascontiguousarray(im))
    for call in (lambda: big.apk_frame(im, pts, sc), lambda: big.pck_frame(im, pts, sc), lambda: big.add_apk_records(raw[0], raw[1], pts, sc),
                 lambda: big.pck(), lambda: big.apk(), lambda: big.get()):
        assert _code(call).code == capi.PBD_ERR_STATE
    assert len(hd.collect(8192)[0]) == n and big.dims() == (5, 0, 0, 0, 0)
    assert big.apk_frame(im, pts, sc) == n                                        # the handle is fine afterwards
    compact = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dp_mode=2, max_candidates=8192)
    ec = capi.Eval(compact, 5, 8, 8192)
    e = _code(lambda: ec.apk_frame(im, pts, sc))
    assert e.code == capi.PBD_ERR_UNSUPPORTED and "evaluation" in str(e)
    compact.close()
    hd.close()
    grp = capi.Group(model, [0], gather=capi.PBD_GATHER_HOST, conv_mode=capi.PBD_CONV_EXACT)
    member = C.c_void_p(grp.L.pbd_group_member(grp.g, 0))
    q = C.c_void_p()
    assert grp.L.pbd_eval_create(member, 5, 8, 8, C.c_double(.5), C.byref(q)) == capi.PBD_OK
    img = np.ascontiguousarray(im)
    rec = C.c_int(0)
    rc = grp.L.pbd_eval_apk_frame_u8(q, img.ctypes.data_as(C.c_void_p), W, H, 3, W * 3, None, None, 0, C.byref(rec), None)
    assert rc == capi.PBD_ERR_UNSUPPORTED
    grp.L.pbd_eval_destroy(q)
    grp.close()


# ---- the layers above -----------------------------------------------------------------------------------------------------------------------
def test_python_and_cpp_evaluation(gpu_required, scene, tmp_path):
    """PartsBasedDetector.evaluation (train -> applyWeights -> evaluate closes on one handle) and pbd::PartsBasedDetector<float>::Evaluation
    (tests/tools/eval_host_check.cpp) reproduce the single-frame whole-path case"""
    from partsbaseddetector_amd import PartsBasedDetector
    model, frames = scene
    im = frames[0]
    det = PartsBasedDetector(device=0, conv_mode=capi.PBD_CONV_EXACT, max_candidates=8192)
    det.distributeModel(model)
    raw = det.handle.detect(im, 8192)
    pts, sc = _persons_from(raw)
    ev = det.evaluation(64, 8192)
    found = ev.addPck(im, pts, sc, OVERLAP)
    records = ev.addApk(im, pts, sc)
    best = capi.candidates_best_overlap(raw[0], raw[1], _gt_boxes(pts), OVERLAP)[0]
    assert list(found) == list((best >= 0).astype(int)) and 2 <= found.sum() < 4
    assert records == len(raw[0]) and ev.dims() == (5, 4, records, 4, 2)
    tp = capi.eval_apk_match_host(raw[0], raw[1], pts, sc, 5)
    e_apk = capi.eval_ap_host(raw[0]["score"], tp, 4)
    apk, prec, rec = ev.apk(curves=True)
    assert _same(apk, e_apk) and (apk > 0).any()
    pcks = [ev.pck(.5, r) for r in (ev.SCALE_LAST, ev.SCALE_OWN)]
    g = ev.ledger.get()
    assert all(_same(p, capi.eval_pck_host(g["dist"], g["scale"], .5, r)) for p, r in zip(pcks, (0, 1))) and (pcks[0] > 0).all()
    ev2 = det.evaluation(64, 3 * 8192)
    ev2.addPckBatch(frames[:2], [(pts, sc), (pts[:0], sc[:0])], OVERLAP)
    assert list(ev2.addApkBatch(frames[:1], [(pts, sc)])) == [records] and _same(ev2.apk(), apk) and _same(ev2.pck(), pcks[0])
    ev2.reset()
    assert ev2.dims() == (5, 0, 0, 0, 0)
    exe = tmp_path / "eval_host_check"
    lib_dir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-o", str(exe), os.path.join(ROOT, "tests", "tools", "eval_host_check.cpp"),
                           "-L" + lib_dir, "-lpbd_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    model.save(str(tmp_path / "model.bin"))
    np.ascontiguousarray(im).tofile(str(tmp_path / "im.raw"))
    with open(tmp_path / "persons.bin", "wb") as f:
        f.write(np.array([len(sc), 5], np.int32).tobytes() + np.ascontiguousarray(pts, np.float64).tobytes() + np.ascontiguousarray(sc, np.float64).tobytes())
    out = subprocess.run([str(exe), str(tmp_path / "model.bin"), str(tmp_path / "im.raw"), str(W), str(H), "3", str(tmp_path / "persons.bin")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = dict(l.split(" ", 1) for l in out.stdout.splitlines())
    assert lines["found"] == " ".join(str(int(v)) for v in found) and int(lines["records"]) == records and lines["dims"] == f"5 4 {records} 4 2"
    assert _same([float.fromhex(v) for v in lines["apk"].split()], apk)
    assert _same([float.fromhex(v) for v in lines["pck0"].split()], pcks[0]) and _same([float.fromhex(v) for v in lines["pck1"].split()], pcks[1])
    p0, rl = lines["prec0"].split(" rec_last ")
    assert float.fromhex(p0) == prec[0, 0] and float.fromhex(rl) == rec[-1, -1]
