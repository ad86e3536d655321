"""Feature vectors of detections on the device (k_featvec.hip, pbd_candidates_features*): every comparison is between the handle
and its OWN feature planes and part locations.

Bit-exact against tests/feature_vector_ref.py (the contract of include/pbd_c.h in numpy) on every plan the entry points serve; the
hand-made records at the planes' edges; the ancestor's assertion w . x = score on the device path, within bounds derived in the two
ref files; every refusal, with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import (dense_feature_vectors, make_face_like_model, make_image, make_mixed_person_model,
                                          make_person_model, make_tree_model_k, make_voc_like_model)
from tests.feature_vector_ref import dot64, feature_vector_ref, window_bound, window_bounds, wx
from tests.part_scores_ref import bound

pytestmark = pytest.mark.gpu

W, H = 320, 240
SW, SH = 100, 80
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


def planes_of(h, w, hgt, frame=0):
    """feat_of_level for feature_vector_ref: the handle's own planes of one frame of its plan (padded when the padding is on)"""
    g = h.geometry(w, hgt)

    def feat(l):
        out = np.zeros((g["cell_h"][l % g["nlevels"]], g["cell_w"][l % g["nlevels"]], 32), h.dtype)
        h._chk(h._fn("pbd_get_frame_level_features")(h.h, frame, l % g["nlevels"], capi._p(out, h._ct)))
        return out
    return feat


def assert_same(got, exp, what=""):
    for g, e, name in zip(got, exp, ("blocks", "windows")):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape)
        assert g.tobytes() == e.tobytes(), (what, name, np.argwhere(g != e)[:5] if name == "windows" else np.argwhere(g != e)[:5])


def check_slots(model, heads, blocks, windows):
    """tails and unused part slots: zeros, ids -1"""
    sizes = model.filter_sizes()
    for i in range(len(heads)):
        n = int(heads["nparts"][i])
        rest = blocks[i, n:]
        assert (rest["bias_id"] == -1).all() and (rest["def_id"] == -1).all() and (rest["filter_id"] == -1).all()
        assert not rest["kh"].any() and not rest["kw"].any() and not rest["def"].any() and not windows[i, n:].any()
        assert not blocks[i]["reserved"].any() and blocks[i, 0]["def_id"] == -1 and not blocks[i, 0]["def"].any()
        for p in range(n):
            f = int(blocks[i, p]["filter_id"])
            assert not windows[i, p, int(sizes[f, 0] * sizes[f, 1]) * 32:].any()


def dev_features(h, heads, locs):
    """pbd_candidates_features_dev into torch buffers, read back"""
    import torch
    n, mp, wmax = len(heads), h.max_parts, h.feature_window_max()
    d_b = torch.full((max(n * mp * 56, 8),), 0xA5, dtype=torch.uint8, device="cuda")
    d_w = torch.full((max(n * mp * wmax, 4),), -7.0, dtype=torch.float64 if h._f64 else torch.float32, device="cuda")
    h.candidates_features_dev(heads, locs, d_b.data_ptr(), d_w.data_ptr())
    torch.cuda.synchronize()
    blocks = d_b.cpu().numpy()[:n * mp * 56].view(capi.FEATURE_BLOCK_DTYPE).reshape(n, mp)
    return blocks, d_w.cpu().numpy()[:n * mp * wmax].reshape(n, mp, wmax)


# ---- 1. bit-exact against the definition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dp_mode", [0, 1])
@pytest.mark.parametrize("conv", [capi.PBD_CONV_EXACT, capi.PBD_CONV_AUTO])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", KINDS)
def test_bit_exact_against_the_definition(gpu_required, kind, dtype, conv, dp_mode):
    im = make_image(5, W, H)
    m = set_thresh(make_model(kind), im, conv_mode=conv, dtype=dtype)
    h = capi.Handle(m, conv_mode=conv, dtype=dtype, dp_mode=dp_mode, max_candidates=CAP)
    heads, _, locs = h.detect(im, CAP)
    assert 5 < len(heads) < CAP
    got = h.candidates_features(heads, locs)
    assert got[1].dtype == np.dtype(dtype) and got[1].shape == (len(heads), m.max_parts, h.feature_window_max())
    assert_same(got, feature_vector_ref(m, planes_of(h, W, H), heads, locs, dtype), kind)
    check_slots(m, heads, *got)
    assert_same(dev_features(h, heads, locs), got, "device buffers")
    h.close()


# ---- 2. hand-made records through the stand-alone entry ------------------------------------------------------------------------
ODD_SIZES = [(9, 9), (6, 4), (3, 7), (5, 5), (3, 3)]   # the filter size of part p (every mixture of it)


def odd_model():
    m = make_tree_model_k([-1, 0, 1, 1, 0], [1, 2, 2, 2, 2], seed=4)
    rng = np.random.default_rng(8)
    for c in range(m.ncomponents):
        for p in range(m.nparts(c)):
            for f in m.filterid[c][p]:
                kh, kw = ODD_SIZES[p]
                m.filtersw[f] = rng.normal(0.0, 0.05, (kh, kw * 32)).astype(np.float32)
    return m


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("frame", [(SW, SH), (80, 80)], ids=["100x80", "80x80"])   # 80 x 80: its coarsest level has 3 x 3 cells
def test_hand_made_records_at_the_edges(gpu_required, frame, dtype):
    w, hgt = frame
    m = odd_model()
    h = capi.Handle(m, dtype=dtype, max_candidates=CAP)
    h.pyramid(make_image(3, w, hgt))
    g = h.geometry(w, hgt)
    levels = [0, g["nlevels"] - 1]
    if frame == (80, 80):
        assert (g["cell_h"][-1], g["cell_w"][-1]) == (3, 3)
    recs = []
    for l in levels:
        ch, cw = int(g["cell_h"][l]), int(g["cell_w"][l])
        for k, (x, y) in enumerate([(0, 0), (cw - 1, 0), (0, ch - 1), (cw - 1, ch - 1), (cw // 2, 0), (cw // 2, ch - 1), (0, ch // 2),
                                    (cw - 1, ch // 2)]):
            recs.append((l, [(x, y, (p + k) % len(m.filterid[0][p])) for p in range(5)]))
    heads = np.zeros(len(recs), capi.HEAD_DTYPE)
    locs = np.zeros((len(recs), 5, 3), np.int32)
    for i, (l, lc) in enumerate(recs):
        heads[i] = (0.0, 0, l, 5)
        locs[i] = lc
    blocks, windows = h.candidates_features(heads, locs)
    assert_same((blocks, windows), feature_vector_ref(m, planes_of(h, w, hgt), heads, locs, dtype), "hand-made")
    assert_same(dev_features(h, heads, locs), (blocks, windows), "device buffers")
    outside = 0
    for i, (l, lc) in enumerate(recs):   # the border, cell by cell, without the ref's window code
        ch, cw = int(g["cell_h"][l]), int(g["cell_w"][l])
        for p, (x, y, _) in enumerate(lc):
            kh, kw = ODD_SIZES[p]
            assert (blocks[i, p]["kh"], blocks[i, p]["kw"]) == (kh, kw)
            win = windows[i, p, :kh * kw * 32].reshape(kh, kw, 32)
            for a in range(kh):
                for b in range(kw):
                    yy, xx = y - kh // 2 + a, x - kw // 2 + b
                    if not (0 <= yy < ch and 0 <= xx < cw):
                        outside += 1
                        assert not win[a, b, :31].any() and win[a, b, 31] == 1
    assert outside > 500
    h.close()


# ---- 3. other plans and call patterns -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def person():
    return set_thresh(make_person_model(seed=1234, K=3), make_image(5, W, H), q=99.5)


def test_batch_plan_of_three_frames(gpu_required, person):
    frames = [make_image(s, W, H) for s in (5, 7, 1)]
    h = capi.Handle(person, max_candidates=CAP)
    res = h.detect_batch(frames, CAP)
    nl = h.geometry(W, H)["nlevels"]
    for f in range(3):
        heads, locs = res[f][0].copy(), res[f][2]
        assert len(heads) > 5
        heads["level"] += f * nl   # a batch plan's levels: frame f's level l is f * nlevels + l
        assert_same(h.candidates_features(heads, locs), feature_vector_ref(person, planes_of(h, W, H, f), heads, locs, np.float32),
                    f"batch frame {f}")
    h.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_boundary_pad(gpu_required, dtype):
    im = make_image(5, SW, SH)
    m = make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21)
    m.thresh = 0.0
    h = capi.Handle(m, dtype=dtype, max_candidates=CAP)
    h.set_boundary_pad(3)
    h.pyramid(im); h.pdf(); h.dp_min()
    vals = np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])])
    h.close()
    m.thresh = float(np.float32(np.percentile(vals[np.isfinite(vals)], 97.0)))
    h = capi.Handle(m, dtype=dtype, max_candidates=CAP)
    h.set_boundary_pad(3)
    heads, _, locs = h.detect(im, CAP)
    assert len(heads) > 5
    got = h.candidates_features(heads, locs)
    assert_same(got, feature_vector_ref(m, planes_of(h, SW, SH), heads, locs, dtype), "padded")
    # a part in the padded plane's corner: the ring's cells come from the plane, the rule applies beyond it
    g = h.geometry(SW, SH)
    hd = heads[:1].copy()
    hd["level"] = 0
    lc = np.zeros((1, 5, 3), np.int32)
    lc[0, :, 0], lc[0, :, 1] = g["cell_w"][0] - 1, g["cell_h"][0] - 1
    assert_same(h.candidates_features(hd, lc), feature_vector_ref(m, planes_of(h, SW, SH), hd, lc, dtype), "padded corner")
    h.close()


def test_after_detect_latent(gpu_required, person):
    im = make_image(5, W, H)
    h = capi.Handle(person, max_candidates=CAP)
    heads, boxes, _ = h.detect(im, CAP)
    one = h.detect_latent(im, boxes[int(np.argmax(heads["score"]))], 0.7)
    assert len(one[0]) == 1
    assert_same(h.candidates_features(one[0], one[2]), feature_vector_ref(person, planes_of(h, W, H), one[0], one[2], np.float32),
                "latent")
    h.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_after_set_level_features(gpu_required, dtype):
    m = make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21)
    h = capi.Handle(m, dtype=dtype, max_candidates=CAP)
    h.begin_frame(SW, SH, 3)
    g = h._geo
    rng = np.random.default_rng(2)
    planes = [rng.uniform(0.0, 0.4, (g["cell_h"][l], g["cell_w"][l], 32)).astype(dtype) for l in range(g["nlevels"])]
    for l, f in enumerate(planes):
        h.set_level_features(l, f)
    n = 40
    heads = np.zeros(n, capi.HEAD_DTYPE)
    locs = np.zeros((n, 5, 3), np.int32)
    for i in range(n):
        l = int(rng.integers(0, g["nlevels"]))
        heads[i] = (0.0, 0, l, 5)
        locs[i, :, 0] = rng.integers(0, g["cell_w"][l], 5)
        locs[i, :, 1] = rng.integers(0, g["cell_h"][l], 5)
        locs[i, :, 2] = [rng.integers(0, len(m.filterid[0][p])) for p in range(5)]
    assert_same(h.candidates_features(heads, locs), feature_vector_ref(m, planes.__getitem__, heads, locs, dtype), "caller planes")
    h.close()


def test_more_records_than_a_staging_chunk(gpu_required, person):
    im = make_image(5, W, H)
    h = capi.Handle(person, max_candidates=CAP)
    heads, _, locs = h.detect(im, CAP)
    n = len(heads)
    assert n > 5
    fb0 = h.footprint()
    first = h.candidates_features(heads, locs)
    assert h.footprint()[1] >= fb0[1] + capi.PBD_FEATVEC_STAGING_BYTES   # the staging buffer counts in the footprint
    rec_bytes = h.max_parts * (56 + h.feature_window_max() * 4)
    total = 2 * (capi.PBD_FEATVEC_STAGING_BYTES // rec_bytes) + 3
    idx = np.arange(total) % n
    blocks, windows = h.candidates_features(heads[idx], locs[idx])
    assert len(blocks) == total
    assert blocks.tobytes() == first[0][idx].tobytes()
    for k in range(0, total, n):   # every copy equals the first
        assert np.array_equal(windows[k:k + n], first[1][:min(n, total - k)]), k
    assert h.footprint()[1] - fb0[1] < 2 * capi.PBD_FEATVEC_STAGING_BYTES   # ... and is bounded
    # count == 0
    L = capi.lib()
    assert L.pbd_candidates_features(h.h, None, None, 0, None, None) == capi.PBD_OK
    assert L.pbd_candidates_features_dev(h.h, None, None, 0, None, None) == capi.PBD_OK
    e = h.candidates_features(heads[:0], locs[:0])
    assert e[0].shape == (0, h.max_parts) and e[1].shape == (0, h.max_parts, h.feature_window_max())
    h.close()


# ---- 4. the ancestor's assertion on the device path --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["person", "tree_k"])
def test_wx_reproduces_the_score(gpu_required, kind, dtype):
    im = make_image(5, W, H)
    kw = dict(conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, dt_correct_ptr=1)
    m = set_thresh(make_model(kind), im, **kw)
    h = capi.Handle(m, max_candidates=CAP, **kw)
    heads, _, locs = h.detect(im, CAP)
    n = len(heads)
    assert 5 < n < CAP
    blocks, windows = h.candidates_features(heads, locs)
    ps = h.candidates_part_scores(heads, locs)
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
    got, _ = wx(m.weight_vector(), dense_feature_vectors(m, blocks, windows))
    B = bound(ps, heads["nparts"], dtype) + window_bounds(m, blocks, windows, dtype)
    r = np.abs(got - score) / B
    print(f"{kind} {np.dtype(dtype).name}: {n} detections, worst |w.x - score| / bound = {r.max():.3f}")
    assert (r <= 1.0).all(), np.argwhere(r > 1.0)[:5]
    worst = 0.0
    for i in range(n):   # filter . window against the handle's own response, within the window bound alone
        for p in range(int(heads["nparts"][i])):
            filt = m.filtersw[int(blocks[i, p]["filter_id"])]
            win = windows[i, p, :filt.size]
            e, b = abs(dot64(filt, win) - ps[i, p, 0]), window_bound(filt, win, dtype)
            worst = max(worst, e / b)
            assert e <= b, (i, p, e, b)
    print(f"{kind} {np.dtype(dtype).name}: worst |filter . window - app| / bound = {worst:.3f}")
    h.close()


# ---- 5. every refusal ---------------------------------------------------------------------------------------------------------
def raw(h, heads, lc, count=None, fn="pbd_candidates_features", blocks=None, windows=None):
    """the C entry on sentinel-filled outputs -> (rc, outputs untouched)"""
    mp, wmax = h.max_parts, h.feature_window_max()
    n = len(heads) if count is None else count
    b = np.full((max(n, 1), mp), 0x5A, np.uint8).repeat(56, axis=1) if blocks is None else blocks
    w = np.full((max(n, 1), mp, wmax), -3.0, np.float64 if fn.endswith("_f64") else np.float32) if windows is None else windows
    rc = getattr(capi.lib(), fn)(h.h, heads.ctypes.data_as(C.c_void_p), capi._p(lc, C.c_int32), n, b.ctypes.data_as(C.c_void_p),
                                 w.ctypes.data_as(C.c_void_p))
    return rc, bool((b == 0x5A).all() and (w == -3.0).all())


def test_refusals(gpu_required, person):
    im = make_image(5, W, H)
    h = capi.Handle(person, max_candidates=CAP)
    zero_h, zero_l = np.zeros(1, capi.HEAD_DTYPE), np.zeros((1, 26, 3), np.int32)
    zero_h[0] = (0.0, 0, 0, 26)
    assert raw(h, zero_h, zero_l) == (capi.PBD_ERR_STATE, True)            # no frame planned
    h.begin_frame(W, H, 3)
    assert raw(h, zero_h, zero_l) == (capi.PBD_ERR_STATE, True)            # no resident features
    heads, _, locs = h.detect(im, CAP)
    assert len(heads) > 5
    lc = np.ascontiguousarray(locs, np.int32)
    g = h.geometry(W, H)
    l0 = int(heads["level"][0])
    assert raw(h, heads, lc)[0] == capi.PBD_OK
    for field, bad in (("level", -1), ("level", g["nlevels"]), ("level", 2 ** 30), ("component", -1), ("component", 1), ("nparts", 0),
                       ("nparts", 25), ("nparts", 27), ("nparts", -3)):
        hd = heads.copy()
        hd[field][len(hd) // 2] = bad
        assert raw(h, hd, lc) == (capi.PBD_ERR_ARG, True), (field, bad)
    for p in (0, 7, 25):
        for k, bad in ((0, -1), (0, int(g["cell_w"][l0])), (1, -1), (1, int(g["cell_h"][l0])), (2, -1), (2, 3), (0, 2 ** 31 - 1),
                       (1, -2 ** 31)):
            bl = lc.copy()
            bl[0, p, k] = bad
            assert raw(h, heads, bl) == (capi.PBD_ERR_ARG, True), (p, k, bad)
    L = capi.lib()
    assert L.pbd_candidates_features(h.h, None, None, 1, None, None) == capi.PBD_ERR_ARG
    assert L.pbd_candidates_features(h.h, None, None, -1, None, None) == capi.PBD_ERR_ARG
    assert raw(h, heads, lc, fn="pbd_candidates_features_f64") == (capi.PBD_ERR_STATE, True)   # the scalar type must match the handle's
    import torch
    d = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    assert L.pbd_candidates_features_dev(h.h, heads.ctypes.data_as(C.c_void_p), capi._p(lc, C.c_int32), 1, C.c_void_p(d.data_ptr()),
                                         C.c_void_p(d.data_ptr() + 4)) == capi.PBD_ERR_ARG     # d_windows: 16-byte aligned
    h.enqueue(im)                                                          # a frame is pending
    assert raw(h, heads, lc) == (capi.PBD_ERR_STATE, True)
    h.collect(CAP)
    assert raw(h, heads, lc)[0] == capi.PBD_OK
    h.close()
    # a handle restricted to a level set refuses the levels it does not process
    h = capi.Handle(person, max_candidates=CAP)
    h.set_levels([l0])
    h.detect(im, CAP)
    other = heads["level"] != l0
    if other.any():
        assert raw(h, heads[other][:1], np.ascontiguousarray(lc[other][:1])) == (capi.PBD_ERR_ARG, True)
    h.close()
    # the compact memory plan: min() reuses the feature planes' memory
    h = capi.Handle(person, dp_mode=2, max_candidates=CAP)
    got = h.detect(im, CAP)
    assert raw(h, got[0], np.ascontiguousarray(got[2])) == (capi.PBD_ERR_STATE, True)
    assert b"compact memory plan" in L.pbd_last_error(h.h)
    h.close()
    # pbd_group members
    grp = capi.Group(person, [0, 0])
    mem = C.c_void_p(L.pbd_group_member(grp.g, 0))
    b, w = (C.c_char * (56 * 26))(), (C.c_float * (26 * 800))()
    for fn in ("pbd_candidates_features", "pbd_candidates_features_f64", "pbd_candidates_features_dev"):
        assert getattr(L, fn)(mem, zero_h.ctypes.data_as(C.c_void_p), capi._p(zero_l, C.c_int32), 1, b, w) == capi.PBD_ERR_UNSUPPORTED
    assert b"pbd_group members are not supported" in L.pbd_last_error(mem)
    grp.close()


# ---- the host layer ---------------------------------------------------------------------------------------------------------------
def test_detector_features(gpu_required, person):
    from partsbaseddetector_amd import PartsBasedDetector
    im = make_image(5, W, H)
    det = PartsBasedDetector(device=0, max_candidates=CAP)
    det.distributeModel(person)
    cands = det.detect(im)
    assert len(cands) > 5
    pick = cands[::3]
    blocks, windows = det.features(pick)
    heads, _, locs = det.handle.detect(im, CAP)
    assert_same((blocks, windows), tuple(a[::3] for a in det.handle.candidates_features(heads, locs)), "detector")
    x = dense_feature_vectors(person, blocks, windows)
    assert x.shape == (len(pick), len(person.weight_vector()))


def test_cpp_demo_dumps_dense_feature_vectors(gpu_required, tmp_path):
    """host/demo.cpp --features FILE (pbd::PartsBasedDetector<T>::features): the sorted records' dense vectors are the handle's own,
    w . x is each record's score, and without the flag the output is the plain demo's"""
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
    out = subprocess.run(base + ["--features", str(tmp_path / "x.bin")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, (plain.stdout, out.stdout, out.stderr)
    assert [l for l in out.stdout.splitlines() if not l.startswith("Features:")] == plain.stdout.splitlines()
    h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, max_candidates=CAP)
    h.set_candidate_filter(capi.PBD_CAND_SORT)
    heads, _, locs = h.detect(im, CAP)
    exp = dense_feature_vectors(m, *h.candidates_features(heads, locs))
    h.close()
    raw_ = np.fromfile(str(tmp_path / "x.bin"), np.uint8)
    rows, cols = (int(v) for v in raw_[:16].view(np.int64))
    assert (rows, cols) == exp.shape and rows > 5
    assert raw_[16:].view(np.float64).reshape(rows, cols).tobytes() == exp.tobytes()
