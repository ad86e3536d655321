"""Per-part scores on the device (k_partscore.hip): every comparison is between the handle and its OWN response planes and part
locations, so no candidate is ever excused as a near tie.

Bit-exact against tests/part_scores_ref.py (the contract of include/pbd_c.h in numpy float64); the re-scored total against the
root score within B = 4 P eps_T S (part_scores_ref.bound: the DP's own roundings, derived there); every detect path against the
stand-alone primitive; the refusals."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import (make_face_like_model, make_image, make_mixed_person_model, make_person_model,
                                          make_tree_model_k, make_voc_like_model)
from tests.part_scores_ref import bound, part_scores_ref, totals

pytestmark = pytest.mark.gpu

W, H = 320, 240
CAP = 8192
KINDS = ["person", "tree_k", "multi", "voc", "mixed"]


def make_model(kind):
    if kind == "person":
        return make_person_model(seed=1234, K=3)
    if kind == "tree_k":
        return make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21)
    if kind == "multi":
        return make_face_like_model(seed=77, ncomp=3, nfilters=40, part_counts=(9, 12))
    if kind == "voc":
        return make_voc_like_model(seed=11)
    return make_mixed_person_model(seed=5, K=2)


def set_thresh(model, im, q=99.5, **kw):
    """threshold = the q-th percentile of the handle's own root values on `im`"""
    model.thresh = 0.0
    h = capi.Handle(model, **kw)
    h.pyramid(im)
    h.pdf()
    h.dp_min()
    vals = np.concatenate([h.root(l, c)[0].ravel() for l in range(h._geo["nlevels"]) for c in range(model.ncomponents)])
    h.close()
    model.thresh = float(np.float32(np.percentile(vals[np.isfinite(vals)], q)))
    return model


def planes_of(h, w=W, hgt=H):
    h._geo = h.geometry(w, hgt)
    nf = len(h.model.filtersw)
    return lambda l: np.stack([h.level_response(l, n) for n in range(nf)])


def checked_count(res):
    assert 5 < len(res[0]) < CAP, len(res[0])
    return len(res[0])


def assert_bits(got, exp, what=""):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert got.tobytes() == exp.tobytes(), (what, np.argwhere(got.view(np.uint64) != exp.view(np.uint64))[:5])


# ---- 4. bit-exact against the definition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dp_mode", [0, 1])
@pytest.mark.parametrize("conv", [capi.PBD_CONV_EXACT, capi.PBD_CONV_AUTO])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", KINDS)
def test_bit_exact_against_the_definition(gpu_required, kind, dtype, conv, dp_mode):
    im = make_image(5, W, H)
    m = set_thresh(make_model(kind), im, conv_mode=conv, dtype=dtype)
    h = capi.Handle(m, conv_mode=conv, dtype=dtype, dp_mode=dp_mode, max_candidates=CAP)
    h.set_part_scores(True)
    heads, boxes, locs = h.detect(im, CAP)
    checked_count((heads, boxes, locs))
    got = h.part_scores(0)
    exp = part_scores_ref(m, planes_of(h), heads, locs)
    assert_bits(got, exp, kind)
    for i in range(len(heads)):   # unused part slots of components with fewer than max_parts parts
        assert not got[i, heads["nparts"][i]:].any()
    assert_bits(h.candidates_part_scores(heads, locs), exp, "stand-alone")
    h.close()


# ---- 5. self-consistency without the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("correct_ptr", [1, 0])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", KINDS)
def test_total_against_the_root_score(gpu_required, kind, dtype, correct_ptr):
    im = make_image(5, W, H)
    m = set_thresh(make_model(kind), im, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, dt_correct_ptr=correct_ptr)
    h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, dt_correct_ptr=correct_ptr, max_candidates=CAP)
    h.set_part_scores(True)
    heads, boxes, locs = h.detect(im, CAP)
    n = checked_count((heads, boxes, locs))
    ps = h.part_scores(0)
    total, B = totals(ps), bound(ps, heads["nparts"], dtype)
    score = heads["score"].astype(np.float64)
    if np.dtype(dtype) == np.dtype(np.float64):   # head.score is float: the root table holds the double
        h._geo = h.geometry(W, H)
        roots = {}
        for i in range(n):
            key = (int(heads["level"][i]), int(heads["component"][i]))
            if key not in roots:
                roots[key] = h.root(*key)[0]
            score[i] = roots[key][locs[i, 0, 1], locs[i, 0, 0]]
        np.testing.assert_array_equal(score.astype(np.float32), heads["score"])
    if correct_ptr:
        r = np.abs(total - score) / B
        print(f"{kind} {np.dtype(dtype).name}: {n} detections, worst |total - score| / B = {r.max():.3f}")
        assert (np.abs(total - score) <= B).all(), np.argwhere(np.abs(total - score) > B)[:5]
    else:
        below = int((total < score - B).sum())
        print(f"{kind} {np.dtype(dtype).name}: {below} of {n} detections re-score below score - B")
        assert (total <= score + B).all(), np.argwhere(total > score + B)[:5]
    h.close()


# ---- 6. every path, same numbers ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def person():
    return set_thresh(make_person_model(seed=1234, K=3), make_image(5, W, H), q=98.5)


def standalone(h, res, frame=0, nlevels=0):
    heads = res[0].copy()
    heads["level"] += frame * nlevels   # a batch plan's levels: frame f's level l is f * nlevels + l
    return h.candidates_part_scores(heads, res[2])


def check_frame(h, res, frame=0, nlevels=0, what=""):
    checked_count(res)
    got = h.part_scores(frame)
    assert len(got) == len(res[0]), what
    assert_bits(got, standalone(h, res, frame, nlevels), what)
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_frame_paths(gpu_required, person, dtype):
    import torch
    im = make_image(5, W, H)
    h = capi.Handle(person, dtype=dtype, max_candidates=CAP)
    h.set_part_scores(True)
    res = h.detect(im, CAP)
    first = check_frame(h, res, what="host")
    assert_bits(first, part_scores_ref(person, planes_of(h), res[0], res[2]), "definition")
    h.enqueue(im)
    res2 = h.collect(CAP)
    assert_bits(check_frame(h, res2, what="enqueue + collect"), first)
    d = torch.from_numpy(im).cuda()
    res3 = h.detect_dev(d.data_ptr(), W, H, 3, capacity=CAP)
    assert_bits(check_frame(h, res3, what="device image"), first)
    # sort + NMS: the records follow the candidates' returned order
    for mode, ov in ((capi.PBD_CAND_SORT, 0.0), (capi.PBD_CAND_SORT_NMS, 0.9)):
        h.set_candidate_filter(mode, ov)
        f = h.detect(im, CAP)
        assert (np.diff(f[0]["score"]) <= 0).all() and len(f[0]) <= len(res[0])
        if mode == capi.PBD_CAND_SORT_NMS:
            assert len(f[0]) < len(res[0])
        got = check_frame(h, f, what=f"filter {mode}")
        assert_bits(got, part_scores_ref(person, planes_of(h), f[0], f[2]), "definition, filtered")
    h.close()


def test_batch_of_three_frames(gpu_required, person):
    frames = [make_image(s, W, H) for s in (5, 7, 1)]
    h = capi.Handle(person, max_candidates=CAP)
    h.set_part_scores(True)
    singles = []
    for f in frames:
        r = h.detect(f, CAP)
        singles.append((r, h.part_scores(0)))
    for mode in (capi.PBD_CAND_RAW, capi.PBD_CAND_SORT_NMS):
        h.set_candidate_filter(mode, 0.9)
        res = h.detect_batch(frames, CAP)
        nl = h.geometry(W, H)["nlevels"]
        for f in range(3):
            got = check_frame(h, res[f], f, nl, f"batch frame {f} mode {mode}")
            if mode == capi.PBD_CAND_RAW:   # per frame identical to the single-frame call
                assert res[f][0].tobytes() == singles[f][0][0].tobytes() and np.array_equal(res[f][2], singles[f][0][2])
                assert_bits(got, singles[f][1], f"batch frame {f} against the single frame")
        with pytest.raises(capi.PbdError) as e:
            h.part_scores(3)
        assert e.value.code == capi.PBD_ERR_STATE
    h.close()


def test_graph_replay_on_different_frames(gpu_required, person):
    frames = [make_image(s, W, H) for s in (5, 7, 1, 2)]
    eager = capi.Handle(person, max_candidates=CAP)
    eager.set_part_scores(True)
    h = capi.Handle(person, graph=1, max_candidates=CAP)
    h.set_part_scores(True)
    for f in frames:   # eager, captured, replayed, replayed
        res = h.detect(f, CAP)
        got = check_frame(h, res, what="graph")
        ref = eager.detect(f, CAP)
        assert res[0].tobytes() == ref[0].tobytes() and np.array_equal(res[2], ref[2])
        assert_bits(got, eager.part_scores(0), "graph against eager")
    # toggled on a replaying handle: the graph is captured again without / with the step
    h.set_part_scores(False)
    for f in frames[:2]:
        h.detect(f, CAP)
        with pytest.raises(capi.PbdError) as e:
            h.part_scores(0)
        assert e.value.code == capi.PBD_ERR_STATE
    h.set_part_scores(True)
    for f in frames[:3]:
        check_frame(h, h.detect(f, CAP), what="graph, toggled on again")
    h.close()
    eager.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_depth_filter_scores_only_survivors(gpu_required, person, dtype):
    im = make_image(5, W, H)
    depth = scene(1, W, H, dtype)
    h = capi.Handle(person, dtype=dtype, max_candidates=CAP)
    h.set_part_scores(True)
    raw = h.detect(im, CAP)
    h.set_depth_filter(True, 0.03)
    kept = h.detect_rgbd(im, depth, CAP)
    assert 0 < len(kept[0]) < len(raw[0])
    got = h.part_scores(0)
    assert len(got) == len(kept[0])
    assert_bits(got, h.candidates_part_scores(kept[0], kept[2]), "depth-pruned")
    h.set_candidate_filter(capi.PBD_CAND_SORT_NMS, 0.9)
    kept2 = h.detect_rgbd(im, depth, CAP)
    assert 0 < len(kept2[0]) <= len(kept[0])
    assert_bits(h.part_scores(0), h.candidates_part_scores(kept2[0], kept2[2]), "depth-pruned + NMS")
    h.close()


def scene(seed, w, hgt, dtype):
    """a few planes with noise and holes (0): parts that straddle two planes fail the depth test, the others pass"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:hgt, 0:w].astype(np.float64)
    d = 3.0 + 0.002 * yy
    d = np.where(xx < w * 0.4, 1.2 + 0.0005 * xx, d)
    d = np.where((yy > hgt * 0.6) & (xx > w * 0.5), 2.0 + 0.001 * (xx - w * 0.5), d)
    d = d + rng.normal(0, 0.01, d.shape)
    d[rng.random(d.shape) < 0.05] = 0.0
    return d.astype(dtype)


# ---- 7. off means off -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
def test_off_means_off(gpu_required, person, graph):
    frames = [make_image(s, W, H) for s in (5, 7, 1)]
    fresh = capi.Handle(person, graph=graph, max_candidates=CAP)
    h = capi.Handle(person, graph=graph, max_candidates=CAP)

    def same():
        for f in frames:
            a, b = h.detect(f, CAP), fresh.detect(f, CAP)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            with pytest.raises(capi.PbdError) as e:
                h.part_scores(0)
            assert e.value.code == capi.PBD_ERR_STATE
    same()
    fb0 = h.footprint()
    h.set_part_scores(True)
    for f in frames:
        a, b = h.detect(f, CAP), fresh.detect(f, CAP)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))   # on: the records themselves do not change either
        assert len(h.part_scores(0)) == len(a[0])
    assert h.footprint()[1] >= fb0[1] + CAP * h.max_parts * 24   # the step's buffers count in the footprint
    h.set_part_scores(False)
    same()
    h.close()
    fresh.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_out_of_range_records_are_refused(gpu_required, person):
    im = make_image(5, W, H)
    h = capi.Handle(person, max_candidates=CAP)
    heads, boxes, locs = h.detect(im, CAP)
    checked_count((heads, boxes, locs))
    g = h.geometry(W, H)
    ok = h.candidates_part_scores(heads, locs)
    l0 = int(heads["level"][0])

    def refused(hd, lc):
        with pytest.raises(capi.PbdError) as e:
            h.candidates_part_scores(hd, lc)
        assert e.value.code == capi.PBD_ERR_ARG

    for field, bad in (("level", -1), ("level", g["nlevels"]), ("level", 2 ** 30), ("component", -1), ("component", 1),
                       ("nparts", 0), ("nparts", 25), ("nparts", 27), ("nparts", -3)):
        hd = heads.copy()
        hd[field][len(hd) // 2] = bad
        refused(hd, locs)
    for p in (0, 7, 25):
        for k, bad in ((0, -1), (0, int(g["cell_w"][l0])), (1, -1), (1, int(g["cell_h"][l0])), (2, -1), (2, 3), (0, 2 ** 31 - 1),
                       (1, -2 ** 31)):
            lc = locs.copy()
            lc[0, p, k] = bad
            refused(heads, lc)
    assert_bits(h.candidates_part_scores(heads, locs), ok, "after the refusals")
    L = capi.lib()
    assert L.pbd_candidates_part_scores(h.h, None, None, 1, None) == capi.PBD_ERR_ARG
    assert L.pbd_candidates_part_scores(h.h, None, None, -1, None) == capi.PBD_ERR_ARG
    assert L.pbd_candidates_part_scores(h.h, None, None, 0, None) == capi.PBD_OK
    cnt = C.c_int(0)
    h.set_part_scores(True)
    h.detect(im, CAP)
    assert L.pbd_get_part_scores(h.h, 0, None, 0, C.byref(cnt)) == capi.PBD_ERR_CAPACITY and cnt.value == len(heads)
    h.close()
    # a handle restricted to a level set refuses the levels it does not process
    h = capi.Handle(person, max_candidates=CAP)
    h.set_levels([l0])
    h.detect(im, CAP)
    hd = heads[heads["level"] != l0][:1]
    if len(hd):
        with pytest.raises(capi.PbdError) as e:
            h.candidates_part_scores(hd, locs[heads["level"] != l0][:1])
        assert e.value.code == capi.PBD_ERR_ARG
    h.close()


def test_stand_alone_needs_resident_responses(gpu_required, person):
    h = capi.Handle(person, max_candidates=CAP)
    heads = np.zeros(1, capi.HEAD_DTYPE)
    heads[0] = (0.0, 0, 0, 26)
    with pytest.raises(capi.PbdError) as e:
        h.candidates_part_scores(heads, np.zeros((1, 26, 3), np.int32))
    assert e.value.code == capi.PBD_ERR_STATE
    h.begin_frame(W, H, 3)
    with pytest.raises(capi.PbdError) as e:
        h.candidates_part_scores(heads, np.zeros((1, 26, 3), np.int32))
    assert e.value.code == capi.PBD_ERR_STATE
    h.close()


def test_group_member_refused(gpu_required, person):
    g = capi.Group(person, [0, 0])
    L = capi.lib()
    mem = C.c_void_p(L.pbd_group_member(g.g, 0))
    out = (C.c_double * (3 * 26))()
    cnt = C.c_int(0)
    heads = (capi.pbd_candidate_head * 1)()
    locs = (C.c_int32 * (3 * 26))()
    assert L.pbd_set_part_scores(mem, 1) == capi.PBD_ERR_UNSUPPORTED
    assert b"pbd_group members are not supported" in L.pbd_last_error(mem)
    assert L.pbd_get_part_scores(mem, 0, out, 1, C.byref(cnt)) == capi.PBD_ERR_UNSUPPORTED
    assert L.pbd_candidates_part_scores(mem, heads, locs, 1, out) == capi.PBD_ERR_UNSUPPORTED
    g.close()


@pytest.mark.parametrize("graph", [0, 1])
def test_compact_plan_is_refused_and_detect_still_succeeds(gpu_required, person, graph):
    im = make_image(5, W, H)
    ref = capi.Handle(person, max_candidates=CAP)
    exp = ref.detect(im, CAP)
    ref.close()
    h = capi.Handle(person, dp_mode=2, graph=graph, max_candidates=CAP)
    h.set_part_scores(True)
    for _ in range(3):
        got = h.detect(im, CAP)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, exp))
        with pytest.raises(capi.PbdError) as e:
            h.part_scores(0)
        assert e.value.code == capi.PBD_ERR_UNSUPPORTED and "compact memory plan" in str(e.value)
        with pytest.raises(capi.PbdError) as e:   # the planes are gone: not scored from stale memory
            h.candidates_part_scores(got[0], got[2])
        assert e.value.code == capi.PBD_ERR_STATE and "compact memory plan" in str(e.value)
    h.set_part_scores(False)
    h.detect(im, CAP)
    with pytest.raises(capi.PbdError) as e:
        h.part_scores(0)
    assert e.value.code == capi.PBD_ERR_STATE
    h.close()


# ---- 9. stage use: planes of the test's own, every sum exact ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_stage_use_exact_total(gpu_required, dtype):
    m = make_tree_model_k([-1, 0, 1, 1, 0], [2, 3, 2, 4, 3], seed=9, quantised=True)   # dyadic deformations, biases k / 4
    planes = {}

    def staged():
        h = capi.Handle(m, dtype=dtype, dt_correct_ptr=1, max_candidates=CAP)
        h.begin_frame(W, H, 3)
        g = h._geo
        rng = np.random.default_rng(17)
        for l in range(g["nlevels"]):
            for n in range(len(m.filtersw)):
                planes[l, n] = rng.integers(-8, 9, (g["cell_h"][l], g["cell_w"][l])).astype(dtype)   # small integers
                h.set_level_response(l, n, planes[l, n])
        h.dp_min()
        return h
    h = staged()   # the threshold: a percentile of these planes' own root values
    vals = np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])])
    h.close()
    m.thresh = float(np.float32(np.percentile(vals, 99.5)))
    h = staged()
    heads, boxes, locs = h.dp_argmin(CAP)
    checked_count((heads, boxes, locs))
    with pytest.raises(capi.PbdError) as e:   # the stage entry point scores nothing itself
        h.part_scores(0)
    assert e.value.code == capi.PBD_ERR_STATE
    ps = h.candidates_part_scores(heads, locs)
    assert_bits(ps, part_scores_ref(m, lambda l: np.stack([planes[l, n] for n in range(len(m.filtersw))]), heads, locs))
    np.testing.assert_array_equal(totals(ps), heads["score"].astype(np.float64))
    h.close()


# ---- the host layer ----------------------------------------------------------------------------------------------------------------
def test_detector_fills_confidences(gpu_required, person):
    from partsbaseddetector_amd import PartsBasedDetector
    im = make_image(5, W, H)
    det = PartsBasedDetector(device=0, max_candidates=CAP)
    det.distributeModel(person)
    off = det.detect(im)
    assert len(off) > 5 and all(not c.confidence[1:].any() and c.partScores() is None for c in off)
    det.setPartScores(True)
    on = det.detect(im)
    assert len(on) == len(off)
    for a, b in zip(on, off):
        assert a.score() == b.score() and np.array_equal(a.parts, b.parts)
        ps = a.partScores()
        assert ps.shape == (26, 3)
        np.testing.assert_array_equal(a.confidence[1:], ((ps[1:, 0] + ps[1:, 1]) + ps[1:, 2]).astype(np.float32))
        assert a.confidence[1:].any()
    det.setPartScores(False)
    assert all(not c.confidence[1:].any() for c in det.detect(im))


def test_cpp_demo_prints_part_scores(gpu_required, tmp_path):
    """host/demo.cpp --part-scores (pbd::PartsBasedDetector<T>::setPartScores): one line per detection whose figures are the
    handle's own; without the flag the output is the plain demo's"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "host", "pbd_demo")
    assert os.path.exists(exe), "build() did not produce the C++ demo"
    im = make_image(5, W, H)
    m = set_thresh(make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21), im, conv_mode=capi.PBD_CONV_EXACT)
    m.save(str(tmp_path / "model.bin"))
    im.tofile(str(tmp_path / "im.raw"))
    base = [exe, str(tmp_path / "model.bin"), str(tmp_path / "im.raw"), str(W), str(H), "3"]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    out = subprocess.run(base + ["--part-scores"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, (plain.stdout, out.stdout, out.stderr)
    lines = out.stdout.splitlines()
    assert [l for l in lines if not l.startswith("  part scores:")] == plain.stdout.splitlines()
    h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, max_candidates=CAP)
    h.set_part_scores(True)
    h.set_candidate_filter(capi.PBD_CAND_SORT)
    heads, _, _ = h.detect(im, CAP)
    ps = h.part_scores(0)
    h.close()
    got = [l.split() for l in lines if l.startswith("  part scores:")]
    assert len(got) == len(heads) > 5
    sc = (ps[:, :, 0] + ps[:, :, 1]) + ps[:, :, 2]
    for i, t in enumerate(got):   # "part scores: total T root R weakest part P (S = app A + def D + bias B)"
        assert float(t[3]) == float(f"{totals(ps)[i]:.9g}") and float(t[5]) == float(f"{heads['score'][i]:.9g}")
        assert int(t[8]) == int(np.argmin(sc[i, :5]))
