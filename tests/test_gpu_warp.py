"""The warped positives on the device (k_warp.hip, k_hog.hip, k_qp_poswrite; include/pbd_c.h "warped positives"), on float and double
handles: the windows equal tests/warp_ref.py in bits; the features equal, in bits, the library's own HOG of that window handed in as a
double frame (and, on the clean cases, the definition and the compiled features.cc); the columns equal tests/qp_ref.py's
standardisation of those features in bits; the skip rule, a full cache, position and split-call invariance, the closed loop
warped positives + negatives -> opt -> weights -> with_weight_vector, every refusal with the cache untouched, and the C++ demo."""
import ctypes as C
import os

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.detector import PartsBasedDetector
from partsbaseddetector_amd.model import make_mixed_person_model
from tests import pyramid_checks
from tests import warp_cases as wc
from tests import warp_ref as wr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ref_warp_v1.npz")
DTYPES = [np.float32, np.float64]
T_IDS = ["T_float", "T_double"]
CPOS, CNEG = 0.002, 0.004
KEYS = [(fi, cn) for fi in range(len(wc.FILTERS)) for cn in (3, 1)]


@pytest.fixture(scope="module")
def ref_windows():
    """the numpy window of every case, computed once: {(fi, cn): [n, oh, ow, 3]} in boxes_of(fi)'s order"""
    return {(fi, cn): np.stack([wr.window(wc.frame(cn), b, *wc.FILTERS[fi]) for b in wc.boxes_of(fi)[1]]) for fi, cn in KEYS}


@pytest.fixture(scope="module", params=DTYPES, ids=T_IDS)
def dev(request, gpu_required):
    """the device's windows and features of every case, computed once per scalar type: (dtype, {(fi, cn): (windows, features)})"""
    out = {}
    for fi in range(len(wc.FILTERS)):
        h = capi.Handle(wc.model_for(fi), conv_mode=capi.PBD_CONV_EXACT, dtype=request.param)
        for cn in (3, 1):
            out[fi, cn] = h.warp_windows(wc.frame(cn), wc.boxes_of(fi)[1], 0)
        h.close()
    return np.dtype(request.param), out


def same(got, exp, what=""):
    for g, e, name in zip(got, exp, ("x", "ids", "b", "d")):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        assert g.tobytes() == e.tobytes(), (what, name, np.argwhere(g != e)[:5])


def columns_ref(model, feats, ids, filter, bias, k):
    _, wreg, w0, _ = model.qp_vectors()
    cols = [wr.column_ref(model, f, filter, bias, i, CPOS, wreg, w0, k) for f, i in zip(feats, ids)]
    return (np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols]), np.array([c[2] for c in cols], np.float32),
            np.array([c[3] for c in cols], np.float64))


# ---- (a) windows ----------------------------------------------------------------------------------------------------------------------
def test_windows_equal_the_restatement_in_bits(dev, ref_windows):
    dtype, got = dev
    for key in KEYS:
        win, feat = got[key]
        kh, kw, sbin = wc.FILTERS[key[0]]
        assert win.dtype == np.float64 and win.shape == ref_windows[key].shape and feat.shape == (len(win), kh, kw, 32) and feat.dtype == dtype
        for i, name in enumerate(wc.boxes_of(key[0])[0]):
            assert win[i].tobytes() == ref_windows[key][i].tobytes(), (key, name, float(np.abs(win[i] - ref_windows[key][i]).max()))


# ---- (b) features == the library's own HOG of the window, every case ------------------------------------------------------------------
def test_features_equal_the_librarys_hog_of_the_window_in_bits(dev):
    dtype, got = dev
    for fi in range(len(wc.FILTERS)):
        h1 = capi.Handle(wc.model_for(fi, interval=1), conv_mode=capi.PBD_CONV_EXACT, dtype=dtype)
        for cn in (3, 1):
            win, feat = got[fi, cn]
            for i, name in enumerate(wc.boxes_of(fi)[0]):
                h1.pyramid_image(win[i])                          # level 0 of an interval-1 model is the frame itself
                assert np.array_equal(h1.level_image_raw(0), win[i])
                assert h1.level_features(0).tobytes() == feat[i].tobytes(), (fi, cn, name)
        h1.close()


# ---- (c) clean cases against the definition and the compiled features.cc ---------------------------------------------------------------
def test_features_of_clean_cases_match_the_definition(dev):
    dtype, got = dev
    gold = np.load(GOLDEN)
    for c in wc.cases():
        if not c["clean"]:
            continue
        i = wc.boxes_of(c["fi"])[0].index(c["box_name"])
        win, feat = got[c["fi"], c["cn"]]
        pyramid_checks.check_hog(feat[i], win[i], c["sbin"], c["name"])
        if dtype == np.float64:
            worst = float(np.abs(feat[i] - gold[c["name"]]).max())
            print(f"[warp f64 vs features.cc] {c['name']}: {worst:.3e}")
            assert worst <= pyramid_checks.F64_TOL, (c["name"], worst)


# ---- (d) columns ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=T_IDS)
def test_columns_equal_the_standardisation_of_the_features_in_bits(gpu_required, dtype):
    for fi in range(len(wc.FILTERS)):
        model = wc.model_for(fi)
        h = capi.Handle(model, dtype=dtype)
        names, boxes = wc.boxes_of(fi)
        filter, bias = 3, 2                                       # any filter and bias of the model, not only the root's
        for cn in (3, 1):
            im = wc.frame(cn)
            q = capi.QpCache(h, len(boxes) + 2, CPOS, CNEG)
            length, k, cap, _ = q.dims()
            ids = np.arange(100, 100 + len(boxes), dtype=np.int32)
            written, status = q.write_warped(im, boxes, filter, bias, 0.0, ids)
            assert written == len(boxes) == q.dims()[3] and (status == capi.PBD_WARP_WRITTEN).all()
            _, feat = h.warp_windows(im, boxes, filter)
            same(q.get(), columns_ref(model, feat, ids, filter, bias, k), (fi, cn))
            x = q.get()[0]
            assert (x[:, 0] == 2).all() and (x[:, 1] == bias + 1).all() and (x[:, 4] == model.feature_layout()["filters"][filter] + 1).all()
            a, sv, _, _ = q.state()                               # the solver's state of the new examples: a = 0, sv = 1
            assert not a.any() and sv[:written].all() and not sv[written:].any()
            q.close()
        h.close()


def test_columns_on_a_mixed_bank_and_the_root_bias(gpu_required):
    """a bank with several filter sizes: the caller's filter order, that filter's own size; the bias block at the root bias (wreg .01)"""
    model = make_mixed_person_model(seed=5, K=2)
    h = capi.Handle(model)
    im = wc.frame(3)
    boxes = wc.boxes_of(0)[1][[0, 1, 5, 9]]
    sizes = model.filter_sizes()
    for filter in (model.filterid[0][0][0], model.filterid[0][1][1], model.filterid[0][2][0]):
        kh, kw = (int(v) for v in sizes[filter])
        assert h.filter_size(filter) == (kh, kw)
        q = capi.QpCache(h, 8, CPOS, CNEG)
        k = q.dims()[1]
        written, _ = q.write_warped(im, boxes, filter, 0)
        win, feat = h.warp_windows(im, boxes, filter)
        assert written == 4 and feat.shape == (4, kh, kw, 32)
        for i, b in enumerate(boxes):
            assert win[i].tobytes() == wr.window(im, b, kh, kw, model.sbin).tobytes(), (filter, i)
        exp = columns_ref(model, feat, np.arange(4), filter, 0, k)
        same(q.get(), exp, filter)
        assert model.qp_vectors()[1][0] == .01 and exp[0][0, 3] == np.float32(CPOS / .01)
        q.close()
    h.close()


# ---- (e), (f) the skip rule, a full cache ---------------------------------------------------------------------------------------------
def test_skip_rule_status_and_a_full_cache(gpu_required):
    model = wc.model_for(0)
    det = PartsBasedDetector(device=0)
    det.distributeModel(model)
    h = det.handle
    im = wc.frame(3)
    names, boxes = wc.boxes_of(0)
    area = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    small = area < 400.0                                          # prod(max filter size * sbin) = (5 * 4) * (5 * 4)
    assert small.sum() == 2 and small[names.index("upsampled")] and small[names.index("one_pixel")] and area[names.index("exact")] == 400.0
    q = capi.QpCache(h, 32, CPOS, CNEG)
    written, status = det.writeWarped(im, boxes, q)               # component 0's root filter and bias, min_area as train.m:135
    assert written == int((~small).sum()) == q.dims()[3]
    assert np.array_equal(status, np.where(small, capi.PBD_WARP_SKIPPED, capi.PBD_WARP_WRITTEN))
    kept = np.nonzero(~small)[0]
    _, feat = h.warp_windows(im, boxes[kept], 0)
    same(q.get(), columns_ref(model, feat, kept, 0, 0, q.dims()[1]), "skip")    # ids default to the box's index in the call
    q.close()
    # (f) 3 free slots, 5 boxes that pass: the first 3 are written and that is no error
    q = capi.QpCache(h, 5, CPOS, CNEG)
    assert q.write_warped(im, boxes[kept[:2]], 0, 0)[0] == 2
    sel = np.concatenate([[names.index("one_pixel")], kept[2:7]])
    written, status = q.write_warped(im, boxes[sel], 0, 0, 400.0)
    assert written == 3 and q.dims()[3] == 5
    W, S, F = capi.PBD_WARP_WRITTEN, capi.PBD_WARP_SKIPPED, capi.PBD_WARP_FULL
    assert status.tolist() == [S, W, W, W, F, F]
    _, feat = h.warp_windows(im, boxes[kept[:5]], 0)
    same(q.get(), columns_ref(model, feat, [0, 1, 1, 2, 3], 0, 0, q.dims()[1]), "full")
    before = q.get()
    written, status = q.write_warped(im, boxes[kept[:2]], 0, 0)   # a full cache: nothing written, no error
    assert written == 0 and status.tolist() == [F, F]
    same(q.get(), before, "full cache untouched")
    q.close()
    det.handle.close()


# ---- (g) position and split-call invariance ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=T_IDS)
def test_position_and_split_call_invariance(gpu_required, dtype):
    model = wc.model_for(2)
    h = capi.Handle(model, dtype=dtype)
    im = wc.frame(3)
    _, boxes = wc.boxes_of(2)
    n = len(boxes)
    win, feat = h.warp_windows(im, boxes, 1)
    perm = np.random.default_rng(5).permutation(n)
    win2, feat2 = h.warp_windows(im, boxes[perm], 1)
    assert win2.tobytes() == win[perm].tobytes() and feat2.tobytes() == feat[perm].tobytes()
    win3, feat3 = h.warp_windows(im, boxes[4:5], 1)               # alone
    assert win3.tobytes() == win[4:5].tobytes() and feat3.tobytes() == feat[4:5].tobytes()
    q1, q2 = capi.QpCache(h, n, CPOS, CNEG), capi.QpCache(h, n + 7, CPOS, CNEG)
    ids = np.arange(n, dtype=np.int32)
    assert q1.write_warped(im, boxes, 1, 1, 0.0, ids)[0] == n
    for lo, hi in ((0, 1), (1, 6), (6, n)):                       # three calls, another capacity
        assert q2.write_warped(im, boxes[lo:hi], 1, 1, 0.0, ids[lo:hi])[0] == hi - lo
    same(q2.get(), q1.get(), "split")
    q2.keep(np.arange(0, n, 2))                                   # columns freed by keep are written again, in another order
    assert q2.write_warped(im, boxes[perm], 1, 1, 0.0, ids[perm])[0] == n + 7 - len(range(0, n, 2))
    full = q1.get()
    m = q2.dims()[3] - len(range(0, n, 2))
    same(q2.get(len(range(0, n, 2))), tuple(v[perm[:m]] for v in full), "after keep")
    q1.close(); q2.close(); h.close()


# ---- (h) the closed loop ---------------------------------------------------------------------------------------------------------------
def test_warped_positives_and_negatives_solve_into_a_model(gpu_required):
    model = wc.model_for(0, interval=5)
    model.thresh = -1e30
    det = PartsBasedDetector(device=0, conv_mode=capi.PBD_CONV_EXACT)
    det.distributeModel(model)
    h = det.handle
    im = wc.frame(3)
    names, boxes = wc.boxes_of(0)
    q = capi.QpCache(h, 64, 0.002, 0.002)
    npos, _ = det.writeWarped(im, boxes, q)
    heads, _, locs = h.detect(im, 4096)
    assert npos == 11 and len(heads) >= 40
    pick = np.linspace(0, len(heads) - 1, 40).astype(int)
    assert q.write(heads[pick], locs[pick], -1, 0) == 40
    _, _, _, noneg = model.qp_vectors()
    q.noneg(noneg)
    q.fix(npos)
    lb, ub, passes = q.opt(.05, 200, seed=3)
    assert 0 < lb <= ub and passes >= 1 and (passes == 200 or 1 - lb / ub < .05), (lb, ub, passes)
    w = q.weights()
    assert np.isfinite(w).all()
    new = model.with_weight_vector(w)
    assert new.weight_vector().tobytes() == w.astype(np.float32).astype(np.float64).tobytes()
    a, sv, ws, _ = q.state()
    _, wreg, w0, _ = model.qp_vectors()
    assert a[:npos].any() and w.tobytes() == (ws / wreg + w0).tobytes()      # the positives carry weight in the solution (qp_w.m)
    assert np.abs(new.filtersw[0]).max() > 0 and not np.array_equal(new.filtersw[0], model.filtersw[0])
    new.thresh = -1e30
    h2 = capi.Handle(new, conv_mode=capi.PBD_CONV_EXACT)          # the new model's handle can be created and detects
    assert len(h2.detect(im, 4096)[0]) == len(heads)
    assert q.dims()[3] == npos + 40
    h2.close(); q.close(); h.close()


# ---- (i) refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_cache_untouched(gpu_required):
    model = wc.model_for(0)
    h = capi.Handle(model)
    im = wc.frame(3)
    _, boxes = wc.boxes_of(0)
    q = capi.QpCache(h, 8, CPOS, CNEG)
    assert q.write_warped(im, boxes[:2], 0, 0)[0] == 2
    before, state = q.get(0, 8), q.dims()

    def refused(code, text, boxes=boxes[:3], filter=0, bias=0, min_area=0.0, im=im):
        with pytest.raises(capi.PbdError) as e:
            q.write_warped(im, boxes, filter, bias, min_area)
        assert e.value.code == code and text in str(e.value), (code, text, str(e.value))
        assert q.dims() == state
        same(q.get(0, 8), before, text)

    bad = boxes[:3].copy(); bad[1, 2] = np.nan
    refused(capi.PBD_ERR_ARG, "box 1 is not finite", boxes=bad)
    bad = boxes[:3].copy(); bad[2, 3] = np.inf
    refused(capi.PBD_ERR_ARG, "box 2 is not finite", boxes=bad)
    bad = boxes[:3].copy(); bad[2, [0, 2]] = bad[2, [2, 0]]
    refused(capi.PBD_ERR_ARG, "inverted", boxes=bad)
    bad = boxes[:3].copy(); bad[0] = (1, 1, 12000, 40)
    refused(capi.PBD_ERR_UNSUPPORTED, "side beyond 16384", boxes=bad)
    refused(capi.PBD_ERR_ARG, "filter outside", filter=len(model.filtersw))
    refused(capi.PBD_ERR_ARG, "filter outside", filter=-1)
    refused(capi.PBD_ERR_ARG, "bias outside", bias=len(model.biasw))
    refused(capi.PBD_ERR_ARG, "bias outside", bias=-1)
    refused(capi.PBD_ERR_ARG, "min_area", min_area=np.nan)
    refused(capi.PBD_ERR_ARG, "im / w / hgt / cn", im=np.zeros((8, 8, 2), np.uint8))
    # a frame pending
    h.enqueue(im)
    refused(capi.PBD_ERR_STATE, "a frame is in flight")
    with pytest.raises(capi.PbdError) as e:
        h.warp_windows(im, boxes[:1], 0)
    assert e.value.code == capi.PBD_ERR_STATE
    h.collect(4096)
    assert q.write_warped(im, boxes[2:3], 0, 0)[0] == 1       # and after the collect it goes through
    # the stand-alone entry: the other scalar type, bad boxes, a large box that must work
    L = capi.lib()
    b1 = np.ascontiguousarray(boxes[:1])
    assert L.pbd_warp_windows_u8_f64(h.h, capi._vp(im), 96, 80, 3, 288, capi._vp(b1), 1, 0, None, None) == capi.PBD_ERR_STATE
    with pytest.raises(capi.PbdError) as e:
        h.warp_windows(im, [(5, 5, 4, 9)], 0)
    assert e.value.code == capi.PBD_ERR_ARG
    assert h.warp_windows(im, np.zeros((0, 4)), 0)[0].shape == (0, 28, 28, 3)
    q.close()
    # pbd_group members
    grp = capi.Group(model, [0, 0])
    mem = C.c_void_p(L.pbd_group_member(grp.g, 0))
    assert L.pbd_warp_windows_u8(mem, capi._vp(im), 96, 80, 3, 288, capi._vp(b1), 1, 0, None, None) == capi.PBD_ERR_UNSUPPORTED
    assert b"pbd_group members are not supported" in L.pbd_last_error(mem)
    grp.close()
    h.close()


def test_a_box_thousands_of_pixels_a_side(gpu_required):
    """the intermediate lives in HBM: a 1500 x 1200 frame, a crop that covers it and more (2379 x 2335), both orders of the axes and
    taps by the dozen, against numpy"""
    rng = np.random.default_rng(11)
    im = rng.integers(0, 256, (1200, 1500), dtype=np.uint8)      # grey: replicated
    h = capi.Handle(wc.model_for(1))
    boxes = np.array([(-200, -100, 1650, 1300), (100, 50, 1400, 250), (600, 20, 800, 1190)], np.float64)
    g = [wr.geometry(b, 3, 7, 8) for b in boxes]
    assert max(x["cw"] for x in g) > 2000 and max(x["ch"] for x in g) > 2000 and {x["rows_first"] for x in g} == {True, False}
    assert max(x["px"] for x in g) > 50 and max(x["py"] for x in g) > 100
    win, feat = h.warp_windows(im, boxes, 0)
    for i, b in enumerate(boxes):
        assert win[i].tobytes() == wr.window(im, b, 3, 7, 8).tobytes(), i
    assert np.isfinite(feat).all() and feat.any()
    h.close()


# ---- (j) the C++ host layer ----------------------------------------------------------------------------------------------------------------
def test_cpp_demo_dumps_warped_positives(gpu_required, tmp_path):
    """host/demo.cpp --warp x1,y1,x2,y2 (pbd::ExampleCache::writeWarped): the columns' b, d and checksum are the binding's"""
    import subprocess
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "host", "pbd_demo")
    assert os.path.exists(exe), "build() did not produce the C++ demo"
    model = wc.model_for(0, interval=5)
    im = wc.frame(3)
    model.save(str(tmp_path / "model.bin"))
    im.tofile(str(tmp_path / "im.raw"))
    names, boxes = wc.boxes_of(0)
    sel = [names.index(n) for n in ("interior", "one_pixel", "fractional", "right")]
    args = [exe, str(tmp_path / "model.bin"), str(tmp_path / "im.raw"), str(wc.FW), str(wc.FH), "3"]
    for i in sel:
        args += ["--warp", ",".join(repr(float(v)) for v in boxes[i])]
    out = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = out.stdout.splitlines()
    det = PartsBasedDetector(device=0, conv_mode=capi.PBD_CONV_EXACT)
    det.distributeModel(model)
    q = capi.QpCache(det.handle, 4, 1.0, 1.0)
    written, status = det.writeWarped(im, boxes[sel], q)
    x, ids, b, d = q.get()
    assert written == 3 and lines[0].startswith(f"Warped positives: 3 of 4 written, k {q.dims()[1]}, len {q.dims()[0]}, min area 400")
    e = 0
    for i, line in enumerate(lines[1:5]):
        assert line.startswith(f"Box {i} (")
        if status[i] != capi.PBD_WARP_WRITTEN:
            assert line.endswith("skipped")
            continue
        f = line.split(": written ")[1].split()
        got = dict(zip(f[0::2], f[1::2]))
        chk = float(np.add.accumulate(np.arange(1, x.shape[1] + 1, dtype=np.float64) * x[e].astype(np.float64))[-1])
        assert int(got["id"]) == ids[e, 1] == i and int(got["blocks"]) == 2
        assert np.float32(got["b"]) == b[e] and float(got["d"]) == d[e] and float(got["checksum"]) == chk, (line, b[e], d[e], chk)
        e += 1
    assert e == 3
    q.close()
    det.handle.close()
