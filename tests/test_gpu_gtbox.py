"""The best pose per ground-truth box on the device (k_gtbox.hip behind k_backtrack; matlab/detection/testmodel_gtbox.m and
bestoverlap.m) against the host function pbd_candidates_best_overlap, which tests/test_bestoverlap_cpu.py holds to the definition:
the stand-alone primitive on the caller's records, and every whole-path entry against the host function applied to the same handle's
plain detect — record bytes, found and the overlap by bytes.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_tree_model
from tests import bestoverlap_ref as ref

pytestmark = pytest.mark.gpu

# the launch code of k_gtbox.hip (pbd_internal.hpp): threads of a block, and the records one pass of k_gtbox_centres' grid covers
PBD_GT_BLOCK = 256
PBD_GT_SPAN = 64 * PBD_GT_BLOCK
W, H = 160, 120
OVERLAP = 0.3


def _code(fn):
    with pytest.raises(capi.PbdError) as e:
        fn()
    return e.value.code


# ---- the stand-alone primitive ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    h = capi.Handle(make_tree_model([-1, 0, 1, 1, 0], 3, seed=5), conv_mode=capi.PBD_CONV_EXACT)
    yield h
    h.close()


def _grown(boxes_of_record, grow):
    """the centre box of one record's parts, grown by `grow` pixels a side"""
    b = np.asarray(boxes_of_record, np.float64)
    cx = b[:, 0] + .5 * (b[:, 2] - 1)
    cy = b[:, 1] + .5 * (b[:, 3] - 1)
    return np.array([cx.min() - grow, cy.min() - grow, cx.max() + grow, cy.max() + grow])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, PBD_GT_BLOCK - 1, PBD_GT_BLOCK, PBD_GT_BLOCK + 1, PBD_GT_SPAN - 1, PBD_GT_SPAN,
                               PBD_GT_SPAN + 1, PBD_GT_SPAN + 1000])
def test_primitive_is_the_host_function(gpu_required, small, n):
    """runs of 100 exactly tied scores (they cross every block boundary), ascending with the position, and on top the last two records
    as one tied pair on gt box 0: its winner is record n - 2 — in the last, partial block, or for n = k * 256 + 1 across its boundary"""
    assert small.max_parts == 5
    heads, boxes = ref.records(11 * n + 1, n, 5, tie_run=100, nparts=np.random.default_rng(n).integers(0, 6, n))
    if n >= 2:
        heads["nparts"][n - 2:] = 5
        heads["score"][n - 2:] = heads["score"].max() + np.float32(1)
        boxes[n - 2] = [(300 + 7 * p, 200 + 11 * p, 20 + p, 31) for p in range(5)]
        boxes[n - 1] = boxes[n - 2]
    for ngt in (1, 3, capi.PBD_GT_MAX):
        gts = ref.gt_boxes(n + ngt, ngt)
        if n >= 2:
            gts[0] = _grown(boxes[n - 2], 2)
        exp = capi.candidates_best_overlap(heads, boxes, gts, OVERLAP)
        got = small.candidates_select_gt(heads, boxes, gts, OVERLAP)
        assert np.array_equal(got[0], exp[0]), (n, ngt, got[0], exp[0])
        assert got[1].tobytes() == exp[1].tobytes(), (n, ngt)
        if n >= 2:
            assert got[0][0] == n - 2
        if n >= 1000 and ngt == capi.PBD_GT_MAX:
            assert (got[0] >= 0).sum() > 32 and len(np.unique(got[0])) > 16


def test_primitive_arguments(gpu_required, small):
    heads, boxes = ref.records(3, 8, 5)
    gt = ref.gt_boxes(3, 2)
    for k in range(3):
        bad = heads.copy()
        bad["score"][k + 2] = (np.nan, np.inf, -np.inf)[k]
        assert _code(lambda: small.candidates_select_gt(bad, boxes, gt)) == capi.PBD_ERR_ARG
    for v in (-1, 6):
        bad = heads.copy()
        bad["nparts"][1] = v
        assert _code(lambda: small.candidates_select_gt(bad, boxes, gt)) == capi.PBD_ERR_ARG
    bad = gt.copy(); bad[1, 2] = np.inf
    assert _code(lambda: small.candidates_select_gt(heads, boxes, bad)) == capi.PBD_ERR_ARG
    assert _code(lambda: small.candidates_select_gt(heads, boxes, gt, float("nan"))) == capi.PBD_ERR_ARG
    assert _code(lambda: small.candidates_select_gt(heads, boxes, ref.gt_boxes(1, capi.PBD_GT_MAX + 1))) == capi.PBD_ERR_ARG
    best, o = small.candidates_select_gt(heads, boxes, np.zeros((0, 4)))
    assert len(best) == 0
    best, o = small.candidates_select_gt(heads[:0], boxes[:0], gt)
    assert list(best) == [-1, -1] and not o.any()


# ---- whole path ---------------------------------------------------------------------------------------------------------------
def _model(orc, seed, im, pct):
    """a 5-part tree model whose threshold sits at a low percentile of the frame's root scores (the CPU oracle's)"""
    model = make_tree_model([-1, 0, 1, 1, 0], 3, seed=seed)
    model.thresh = -1e30
    fr = orc.detect(model, im, capacity=1, keep=True)[4]
    model.thresh = float(np.float32(np.percentile(np.concatenate([fr.root(l)[0].ravel() for l in range(fr.nlevels)]), pct)))
    fr.free()
    return model


def _gt_from(raw, ranks=(0, 9, 99), grow=3.0):
    """gt boxes off a frame's raw records: the centre boxes of the records of these ranks by score, grown; one box off the frame; one
    tiny box"""
    order = np.argsort(-raw[0]["score"].astype(np.float64), kind="stable")
    gts = [_grown(raw[1][order[r]][:int(raw[0]["nparts"][order[r]])], grow) for r in ranks]
    gts.append(np.array([5000.0, 5000.0, 5100.0, 5200.0]))
    gts.append(np.array([70.25, 50.5, 71.0, 51.75]))
    return np.stack(gts)


@pytest.fixture(scope="module")
def frame(orc):
    im = make_image(61, W, H)
    model = _model(orc, 91, im, 70.0)
    raw = orc.detect(model, im, capacity=65536)[:3]
    return model, im, raw, _gt_from(raw)


def _expect(raw, gts, overlap=OVERLAP):
    best, o = capi.candidates_best_overlap(raw[0], raw[1], gts, overlap)
    return best, o


def _assert_winners(got, raw, gts, overlap=OVERLAP, what=""):
    heads, boxes, locs, found, o = got
    best, eo = _expect(raw, gts, overlap)
    assert len(heads) == len(gts) == len(found) == len(o), what
    assert np.array_equal(found, (best >= 0).astype(np.int32)), (what, found, best)
    assert np.asarray(o).tobytes() == eo.tobytes(), (what, o, eo)
    for g, b in enumerate(best):
        if b < 0:
            continue
        assert heads[g:g + 1].tobytes() == raw[0][b:b + 1].tobytes(), (what, g, heads[g], raw[0][b])
        assert np.array_equal(boxes[g], raw[1][b]) and np.array_equal(locs[g], raw[2][b]), (what, g)
    return best


def test_frame_is_not_vacuous(gpu_required, orc, frame):
    """the CPU oracle's records of the tested frame: a few hundred to a few thousand; a box matched by a record that is not the frame's
    best; an unmatched box; two matched boxes with different winners"""
    model, im, raw, gts = frame
    assert 300 <= len(raw[0]) <= 4000, len(raw[0])
    best, o = _expect(raw, gts)
    top = int(np.argmax(raw[0]["score"]))
    matched = best[best >= 0]
    assert (matched != top).any() and (best < 0).any() and len(np.unique(matched)) >= 2, best
    assert best[3] == -1


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_detect_gtbox_is_best_overlap_of_detect(gpu_required, orc, frame, dtype):
    """pbd_detect_gtbox_u8, the device-image entry and the compact plan (dp_mode 2): the host function applied to the same handle's
    plain detect; the float EXACT handle's plain detect is the oracle's"""
    import torch
    model, im, oraw, gts = frame
    for dp_mode in (0, 2):
        hd = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, dp_mode=dp_mode, max_candidates=8192)
        raw = hd.detect(im, 8192)
        if np.dtype(dtype) == np.float32:
            assert raw[0].tobytes() == np.ascontiguousarray(oraw[0]).tobytes() and np.array_equal(raw[1], oraw[1])
        assert len(raw[0]) >= 300
        best = _assert_winners(hd.detect_gtbox(im, gts, OVERLAP), raw, gts, what=("host", dp_mode))
        assert hd.gt_records == len(raw[0])
        assert (best >= 0).sum() >= 2
        t = torch.from_numpy(np.ascontiguousarray(im)).cuda()
        torch.cuda.synchronize()
        _assert_winners(hd.detect_gtbox_dev(t.data_ptr(), W, H, 3, gts, OVERLAP), raw, gts, what=("dev", dp_mode))
        for ov in (0.0, 0.7):
            _assert_winners(hd.detect_gtbox(im, gts, ov), raw, gts, ov, what=(ov, dp_mode))
        none = hd.detect_gtbox(im, np.zeros((0, 4)))
        assert len(none[0]) == 0 and hd.gt_records == len(raw[0])
        again = hd.detect(im, 8192)
        assert again[0].tobytes() == raw[0].tobytes() and np.array_equal(again[2], raw[2])
        hd.close()


def test_batch_of_three_frames(gpu_required, orc, frame):
    model, im, _, gts0 = frame
    frames = [im, make_image(62, W, H), make_image(63, W, H)]
    hd = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, max_candidates=16384)
    raws = [hd.detect(f, 16384) for f in frames]
    assert all(len(r[0]) > 100 for r in raws)
    # a box that only frame 1's records can match: the tight centre box of one of its records that no record of frame 0 sits on
    only1 = None
    for r in np.argsort(-raws[1][0]["score"].astype(np.float64), kind="stable"):
        box = _grown(raws[1][1][r][:int(raws[1][0]["nparts"][r])], 0.5)
        if _expect(raws[0], box[None], 0.8)[0][0] < 0 and _expect(raws[1], box[None], 0.8)[0][0] >= 0:
            only1 = box
            break
    assert only1 is not None
    gts = [gts0, np.stack([only1, _gt_from(raws[1], (4,))[0], gts0[3]]), np.zeros((0, 4))]
    singles = [hd.detect_gtbox(f, g, 0.8) for f, g in zip(frames, gts)]
    got = hd.detect_batch_gtbox(frames, gts, 0.8)
    assert hd.gt_records == sum(len(r[0]) for r in raws)
    for f in range(3):
        _assert_winners(got[f], raws[f], gts[f], 0.8, what=f)
        for a, b in zip(got[f], singles[f]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), f
    assert got[1][3][0] == 1 and len(got[2][0]) == 0
    assert int(got[1][0]["level"][0]) < hd.geometry(W, H)["nlevels"]          # the frame's own level, not the virtual one
    swapped = hd.detect_batch_gtbox(frames, [only1[None], gts[1], gts0[:2]], 0.8)
    assert swapped[0][3][0] == 0 and swapped[0][4][0] == 0.0                     # frame 1's box finds nothing in frame 0
    _assert_winners(swapped[2], raws[2], gts0[:2], 0.8, what="swapped")
    hd.close()


def test_plain_frames_on_a_graph_handle_are_untouched(gpu_required, orc, frame):
    model, im, _, gts = frame
    hd = capi.Handle(model, graph=1, max_candidates=8192)
    plain = [hd.detect(im, 8192) for _ in range(3)]                              # eager, captured, replayed
    got = hd.detect_gtbox(im, gts, OVERLAP)
    after = [hd.detect(im, 8192) for _ in range(2)]
    assert len(plain[0][0]) > 100
    for other in plain[1:] + after:
        for k in range(3):
            assert np.asarray(other[k]).tobytes() == np.asarray(plain[0][k]).tobytes()
    _assert_winners(got, plain[0], gts, what="graph")
    hd.close()


@pytest.mark.parametrize("special", ["gtbox_raw", "rgbd_filtered"])
def test_replayed_plain_frame_after_an_eager_special_frame(gpu_required, orc, frame, special):
    """graph=1: plain frame (eager), plain frame (captured), one eager special frame — gt-box on a RAW handle, RGB-D with depth pruning
    on a filtered one —, then a plain frame replayed from the graph: what the collect is told about the pending frame is the replayed
    frame's own, not what the special frame left, so its records are the first plain frame's, in bits"""
    model, im, _, gts = frame
    hd = capi.Handle(model, graph=1, max_candidates=8192)
    if special == "rgbd_filtered":
        hd.set_candidate_filter(capi.PBD_CAND_SORT)      # (every record kept, in Candidate::sort's order: the frame stays a few hundred records)
        hd.set_depth_filter(True, 0.03)
    first = hd.detect(im, 8192)
    captured = hd.detect(im, 8192)
    assert len(first[0]) > 20
    if special == "gtbox_raw":
        got = hd.detect_gtbox(im, gts, OVERLAP)
        _assert_winners(got, first, gts, what=special)
    else:
        depth = (2.0 + 0.001 * np.arange(W, dtype=np.float32))[None, :].repeat(H, 0)
        depth[::7, ::5] = 0.0
        pruned = hd.detect_rgbd(im, depth, 8192)
        assert 0 < len(pruned[0]) <= len(first[0])
    last = hd.detect(im, 8192)
    for other in (captured, last):
        for k in range(3):
            assert np.asarray(other[k]).tobytes() == np.asarray(first[k]).tobytes(), (special, k)
    hd.close()


def test_refusals_and_capacity(gpu_required, orc, frame):
    model, im, _, gts = frame
    hd = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, max_candidates=8192)
    n = len(hd.detect(im, 8192)[0])
    run = lambda: hd.detect_gtbox(im, gts, OVERLAP)
    for on, off in ((lambda: hd.set_candidate_filter(capi.PBD_CAND_SORT), lambda: hd.set_candidate_filter(capi.PBD_CAND_RAW)),
                    (lambda: hd.set_candidate_filter(capi.PBD_CAND_SORT_NMS, 0.3), lambda: hd.set_candidate_filter(capi.PBD_CAND_RAW)),
                    (lambda: hd.set_depth_filter(True), lambda: hd.set_depth_filter(False)),
                    (lambda: hd.set_box3d(True, (500.0, 500.0, 80.0, 60.0)), lambda: hd.set_box3d(False)),
                    (lambda: hd.set_cluster3d(True), lambda: hd.set_cluster3d(False)),
                    (lambda: hd.set_part_scores(True), lambda: hd.set_part_scores(False))):
        on()
        assert _code(run) == capi.PBD_ERR_UNSUPPORTED
        assert "gt boxes" in hd.L.pbd_last_error(hd.h).decode()
        off()
    bad = gts.copy(); bad[1, 0] = np.nan
    assert _code(lambda: hd.detect_gtbox(im, bad)) == capi.PBD_ERR_ARG
    assert _code(lambda: hd.detect_gtbox(im, gts, float("inf"))) == capi.PBD_ERR_ARG
    assert _code(lambda: hd.detect_gtbox(im, ref.gt_boxes(1, capi.PBD_GT_MAX + 1))) == capi.PBD_ERR_ARG
    hd._geo = hd.geometry(W, H)
    hd.enqueue(np.ascontiguousarray(im))
    assert _code(run) == capi.PBD_ERR_STATE
    assert _code(lambda: hd.candidates_select_gt(*ref.records(1, 4, 5), gts)) == capi.PBD_ERR_STATE
    assert len(hd.collect(8192)[0]) == n
    assert hd.detect_gtbox(im, gts, OVERLAP)[3].sum() >= 2                       # the handle is fine afterwards
    hd.close()
    grp = capi.Group(model, [0], gather=capi.PBD_GATHER_HOST, conv_mode=capi.PBD_CONV_EXACT)
    member = C.c_void_p(grp.L.pbd_group_member(grp.g, 0))
    img = np.ascontiguousarray(im)
    g = np.ascontiguousarray(gts)
    heads = np.zeros(len(g), capi.HEAD_DTYPE); found = np.zeros(len(g), np.int32)
    rc = grp.L.pbd_detect_gtbox_u8(member, img.ctypes.data_as(C.c_void_p), W, H, 3, W * 3, g.ctypes.data_as(C.c_void_p), len(g),
                                   C.c_double(OVERLAP), heads.ctypes.data_as(C.c_void_p), None, None, found.ctypes.data_as(C.c_void_p),
                                   None, None)
    assert rc == capi.PBD_ERR_UNSUPPORTED
    grp.close()
    exact = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, max_candidates=n)
    assert exact.detect_gtbox(im, gts, OVERLAP)[3].sum() >= 2 and exact.gt_records == n
    exact.close()
    short = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, max_candidates=n - 1)
    assert _code(lambda: short.detect_gtbox(im, gts, OVERLAP)) == capi.PBD_ERR_CAPACITY
    assert short.gt_records == n                                                 # the needed count, as the plain entries report it
    short.close()


# ---- the layers above ---------------------------------------------------------------------------------------------------------
def test_python_classes_and_cpp_demo(gpu_required, orc, frame, tmp_path):
    """PartsBasedDetector.detectGtBox and Candidate.bestOverlap give the handle's winners; host/demo.cpp --gtbox prints them — fused
    (pbd::PartsBasedDetector<T>::detectGtBox) and stagewise (pbd::Candidate::bestOverlap on argmin()'s candidates)"""
    import os
    import subprocess
    from partsbaseddetector_amd import Candidate, PartsBasedDetector
    model, im, raw, gts = frame
    best, o = _expect(raw, gts)
    det = PartsBasedDetector(device=0, conv_mode=capi.PBD_CONV_EXACT)
    det.distributeModel(model)
    poses, go = det.detectGtBox(im, gts, OVERLAP)
    assert go.tobytes() == o.tobytes() and [p is not None for p in poses] == list(best >= 0)
    for g, b in enumerate(best):
        if b >= 0:
            assert np.float32(poses[g].score()) == raw[0]["score"][b] and np.array_equal(poses[g].parts, raw[1][b][:5])
    cb, co = Candidate.bestOverlap(det.detect(im), gts, OVERLAP)
    assert np.array_equal(cb, best) and co.tobytes() == o.tobytes()
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "host", "pbd_demo")
    assert os.path.exists(exe), "build() did not produce the C++ demo"
    model.save(str(tmp_path / "model.bin"))
    np.ascontiguousarray(im).tofile(str(tmp_path / "im.raw"))
    args = [exe, str(tmp_path / "model.bin"), str(tmp_path / "im.raw"), str(W), str(H), "3"]
    opts = []
    for g in gts:
        opts += ["--gtbox", ",".join(repr(float(v)) for v in g) + f",{OVERLAP}"]
    for mode in ([], ["stagewise"]):
        out = subprocess.run(args + mode + opts, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (out.stdout, out.stderr)
        lines = [l for l in out.stdout.splitlines() if l.startswith("GtBox ")]
        assert len(lines) == len(gts), out.stdout
        for g, b in enumerate(best):
            tail = lines[g].split(": ", 1)[1]
            if b < 0:
                assert tail == "none", lines[g]
                continue
            ov, pose = tail.split(": ", 1)
            t = pose.split()
            assert float(ov.split()[1]) == o[g], lines[g]
            assert float(t[0]) == float(f"{raw[0]['score'][b]:.9g}") and int(t[2]) == raw[0]["level"][b], lines[g]
            assert [tuple(int(v) for v in q.split(",")) for q in t[3:]] == [tuple(int(v) for v in r) for r in raw[1][b][:5]], lines[g]
    bad = subprocess.run(args + ["--gtbox", "1,2,3"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--gtbox" in bad.stdout
