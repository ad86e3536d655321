"""The warped positives without a GPU (include/pbd_c.h "warped positives"): the host planner (pbd_warp_geometry, pbd_warp_taps) equals
tests/warp_ref.py in bits; the bilinear taps are what the definition says (identity at scale 1, [1 3 3 1] / 8 at 2:1, constants stay
constant); every case's `clean` flag is what tests/hog_ref.excused_cells finds; hog_def of the numpy windows is the compiled
features.cc (tests/golden/ref_warp_v1.npz) within F64_TOL; Model.with_weight_vector is vec2model.m; and the entry points are declared,
exported, bound and refuse NULL and bad arguments.  tests/test_gpu_warp.py holds the device to the same restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_mixed_person_model, make_tree_model
from tests import warp_cases as wc
from tests import warp_ref as wr
from tests.hog_ref import excused_cells, hog_def
from tests.pyramid_checks import F64_TOL

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ref_warp_v1.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pbd_warp_geometry", "pbd_warp_taps", "pbd_warp_windows_u8", "pbd_warp_windows_u8_f64", "pbd_qp_write_warped_u8"]


@pytest.fixture(scope="module")
def windows():
    """the numpy window of every case, computed once"""
    frames = {cn: wc.frame(cn) for cn in (3, 1)}
    return {c["name"]: wr.window(frames[c["cn"]], c["box"], c["kh"], c["kw"], c["sbin"]) for c in wc.cases()}


# ---- 1. the planner -------------------------------------------------------------------------------------------------------------------
def test_planner_equals_the_restatement_in_bits():
    seen = set()
    for c in wc.cases():
        g = wr.geometry(c["box"], c["kh"], c["kw"], c["sbin"])
        got = capi.warp_geometry(c["box"], c["kh"], c["kw"], c["sbin"])
        assert (got["rect"], got["rows_first"], got["py"], got["px"]) == (g["rect"], g["rows_first"], g["py"], g["px"]), (c["name"], got, g)
        for n_in, n_out in ((g["ch"], g["oh"]), (g["cw"], g["ow"])):
            if (n_in, n_out) in seen:
                continue
            seen.add((n_in, n_out))
            idx, w = capi.warp_taps(n_in, n_out)
            ridx, rw = wr.taps(n_in, n_out)
            assert idx.shape == ridx.shape == (n_out, wr.ntaps(n_in, n_out)) and idx.tobytes() == ridx.tobytes(), (c["name"], n_in, n_out)
            assert w.tobytes() == rw.tobytes(), (c["name"], n_in, n_out)
            assert idx.min() >= 0 and idx.max() < n_in
    # both orders of the axes, ties, up- and downsampling all occur
    geo = [wr.geometry(c["box"], c["kh"], c["kw"], c["sbin"]) for c in wc.cases()]
    assert {g["rows_first"] for g in geo} == {True, False}
    assert any(g["cw"] < g["ow"] for g in geo) and any(g["cw"] > 2 * g["ow"] for g in geo) and any(g["cw"] == g["ow"] and g["ch"] == g["oh"] for g in geo)


def test_rounding_is_half_away_from_zero_and_one_based():
    # padx = 4 * 8 / 20 = 1.6: 0.9 - 1.6 = -0.7 -> -1;  x1 = 2.1: 0.5 -> 1 (away from zero), x1 = 1.1: -0.5 -> -1
    assert capi.warp_geometry((2.1, 1, 9.1, 8), 5, 5, 4)["rect"][0] == 1 == wr.geometry((2.1, 1, 9.1, 8), 5, 5, 4)["rect"][0]
    assert capi.warp_geometry((1.1, 1, 8.1, 8), 5, 5, 4)["rect"][0] == -1 == wr.geometry((1.1, 1, 8.1, 8), 5, 5, 4)["rect"][0]
    # a tie of the two scales goes to rows
    assert capi.warp_geometry((33, 22, 52, 41), 5, 5, 4)["rows_first"] is True


def test_bilinear_taps_are_the_definition():
    idx, w = capi.warp_taps(28, 28)                       # scale 1: the identity
    hit = idx == np.arange(28)[:, None]
    assert (np.where(hit, w, 0).sum(axis=1) == 1.0).all() and (w[~hit] == 0).all()
    idx, w = capi.warp_taps(56, 28)                       # 2:1: the antialiased triangle [1 3 3 1] / 8
    for x in (3, 14, 20):
        nz = w[x] > 0
        assert idx[x][nz].tolist() == [2 * x - 1, 2 * x, 2 * x + 1, 2 * x + 2] and w[x][nz].tolist() == [.125, .375, .375, .125]
    assert idx[0][w[0] > 0].tolist() == [0, 0, 1, 2]      # the mirror at the border: tap 0 of 1-based index 0 is pixel 1 again
    idx, w = capi.warp_taps(14, 28)                       # 1:2: taps 1/4 and 3/4
    assert sorted(w[5][w[5] > 0].tolist()) == [.25, .75]
    for n_in, n_out in ((7, 28), (200, 28), (33, 56), (1, 40)):
        _, w = capi.warp_taps(n_in, n_out)
        assert np.abs(w.sum(axis=1) - 1).max() <= 4 * 2.0 ** -52 * w.shape[1]


def test_a_constant_image_stays_constant():
    im = np.full((80, 96, 3), 173, np.uint8)
    for c in wc.cases():
        if c["cn"] == 3 and c["fi"] == 1:
            g = wr.geometry(c["box"], c["kh"], c["kw"], c["sbin"])
            win = wr.window(im, c["box"], c["kh"], c["kw"], c["sbin"])
            assert win.shape == (g["oh"], g["ow"], 3)
            assert np.abs(win - 173.0).max() <= 173.0 * 2.0 ** -52 * 2 * (g["py"] + g["px"]), c["name"]


def test_scale_one_window_is_the_crop(windows):
    for c in wc.cases():
        if c["box_name"] == "exact":
            g = wr.geometry(c["box"], c["kh"], c["kw"], c["sbin"])
            assert (g["cw"], g["ch"]) == (g["ow"], g["oh"])
            assert np.array_equal(windows[c["name"]], wr.crop(wc.frame(c["cn"]), g["rect"])), c["name"]


def test_grey_frames_are_replicated(windows):
    for c in wc.cases():
        if c["cn"] == 1:
            w = windows[c["name"]]
            assert np.array_equal(w[..., 0], w[..., 1]) and np.array_equal(w[..., 0], w[..., 2]), c["name"]


# ---- 2. the clean list is verified, not trusted ----------------------------------------------------------------------------------------
def test_clean_flags_are_what_excused_cells_finds(windows):
    clean_sides = set()
    for c in wc.cases():
        feat, margin, det = hog_def(windows[c["name"]], c["sbin"], details=True)
        assert feat.shape == (c["kh"], c["kw"], 32), c["name"]
        _, nbad = excused_cells(margin, det, feat.shape[:2])
        assert (nbad == 0) == c["clean"], (c["name"], nbad)
        if c["clean"]:
            X1, Y1, X2, Y2 = wr.geometry(c["box"], c["kh"], c["kw"], c["sbin"])["rect"]
            clean_sides |= {s for s, out in (("left", X1 < 1), ("top", Y1 < 1), ("right", X2 > wc.FW), ("bottom", Y2 > wc.FH)) if out}
    assert clean_sides == {"left", "top", "right", "bottom"}    # a clean crossing of every side


# ---- 3. the windows' HOG against the compiled features.cc ------------------------------------------------------------------------------
def test_hog_def_of_the_windows_matches_the_compiled_reference(windows):
    gold = np.load(GOLDEN)
    clean = [c for c in wc.cases() if c["clean"]]
    assert sorted(gold.files) == sorted(c["name"] for c in clean)
    for c in clean:
        worst = float(np.abs(hog_def(windows[c["name"]], c["sbin"])[0] - gold[c["name"]]).max())
        print(f"[def vs features.cc] {c['name']}: {worst:.3e}")
        assert gold[c["name"]].dtype == np.float64 and worst <= F64_TOL, (c["name"], worst)


# ---- 4. vec2model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda: make_tree_model([-1, 0, 1, 1, 0], 3, seed=5), lambda: make_mixed_person_model(seed=5, K=2)])
def test_with_weight_vector_round_trip(make):
    m = make()
    w = m.weight_vector()
    m2 = m.with_weight_vector(w)                          # float32-representable weights: exact
    assert m2.weight_vector().tobytes() == w.tobytes()
    assert all(np.array_equal(a, b) and a.dtype == b.dtype == np.float32 and a.shape == b.shape for a, b in zip(m2.filtersw, m.filtersw))
    assert np.array_equal(m2.biasw, m.biasw) and np.array_equal(m2.defw, m.defw) and m2.defw.shape == np.asarray(m.defw).shape
    rng = np.random.default_rng(3)
    v = rng.normal(0, 1, w.size)                          # any float64 vector: vec2model.m's assertion holds on the float32-rounded weights
    m3 = m.with_weight_vector(v)
    assert m3.weight_vector().tobytes() == v.astype(np.float32).astype(np.float64).tobytes()
    lay = m.feature_layout()
    assert m3.biasw[1] == np.float32(v[1]) and m3.defw.ravel()[5] == np.float32(v[lay["deform"] + 5])
    f = len(m.filtersw) - 1
    assert m3.filtersw[f].ravel()[7] == np.float32(v[int(lay["filters"][f]) + 7])
    assert m.weight_vector().tobytes() == w.tobytes() and m3.filterid == m.filterid      # the source model is untouched
    assert m3.to_desc_sized()[0].nfilters == len(m.filtersw)
    with pytest.raises(ValueError):
        m.with_weight_vector(v[:-1])
    v[3] = np.inf
    with pytest.raises(ValueError):
        m.with_weight_vector(v)


# ---- 5. declared, exported, bound; refusals -------------------------------------------------------------------------------------------
def test_warp_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"\b(pbd_[a-z0-9_]+)\s*\(", hdr))
    L = capi.lib()
    for name in NEW:
        assert name in declared and name in capi.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert callable(capi.Handle.warp_windows) and callable(capi.QpCache.write_warped)
    assert L.pbd_abi_version() == 5 and "#define PBD_ABI_VERSION 5" in hdr
    assert "DEVIATION: MATLAB's own summation order is unknown" in hdr
    host = open(os.path.join(ROOT, "partsbaseddetector_amd", "host", "pbd_host.hpp")).read()
    assert "pbd_qp_write_warped_u8(" in host and "writeWarped" in host
    from partsbaseddetector_amd.detector import PartsBasedDetector
    assert callable(PartsBasedDetector.writeWarped)


def test_null_and_bad_arguments_are_refused():
    L = capi.lib()
    n = C.c_int()
    box = np.array([1., 1., 8., 8.])
    im = np.zeros((8, 8, 3), np.uint8)
    assert L.pbd_warp_windows_u8(None, capi._vp(im), 8, 8, 3, 24, capi._vp(box), 1, 0, None, None) == capi.PBD_ERR_ARG
    assert L.pbd_warp_windows_u8_f64(None, capi._vp(im), 8, 8, 3, 24, capi._vp(box), 1, 0, None, None) == capi.PBD_ERR_ARG
    assert L.pbd_qp_write_warped_u8(None, capi._vp(im), 8, 8, 3, 24, capi._vp(box), None, 1, 0, 0, 0.0, None, C.byref(n)) == capi.PBD_ERR_ARG
    assert L.pbd_warp_geometry(None, 5, 5, 4, None, None, None, None) == capi.PBD_ERR_ARG
    assert L.pbd_warp_geometry(capi._vp(box), 5, 5, 4, None, None, None, None) == capi.PBD_OK          # outputs may be NULL
    for bad in ((np.nan, 1, 8, 8), (1, 1, np.inf, 8), (9, 1, 8, 8), (1, 9, 8, 8)):
        with pytest.raises(capi.PbdError) as e:
            capi.warp_geometry(bad, 5, 5, 4)
        assert e.value.code == capi.PBD_ERR_ARG, bad
    for kh, kw, sbin in ((0, 5, 4), (5, 0, 4), (5, 5, 0)):
        with pytest.raises(capi.PbdError):
            capi.warp_geometry(box, kh, kw, sbin)
    with pytest.raises(capi.PbdError) as e:
        capi.warp_geometry((1, 1, 12000, 8), 5, 5, 4)     # crop side 12000 * 1.4 > 16384
    assert e.value.code == capi.PBD_ERR_UNSUPPORTED
    assert capi.warp_geometry((1, 1, 11000, 8), 5, 5, 4)["px"] == wr.ntaps(15400, 28)      # thousands of pixels a side are planned
    with pytest.raises(capi.PbdError) as e:
        capi.warp_geometry((1e12, 1, 1e12 + 5, 8), 5, 5, 4)
    assert e.value.code == capi.PBD_ERR_UNSUPPORTED
    P = C.c_int32()
    assert L.pbd_warp_taps(0, 8, None, None, 0, C.byref(P)) == capi.PBD_ERR_ARG
    assert L.pbd_warp_taps(8, 0, None, None, 0, C.byref(P)) == capi.PBD_ERR_ARG
    assert L.pbd_warp_taps(8, 8, None, None, 0, None) == capi.PBD_ERR_ARG
    idx = np.zeros(8, np.int32)
    assert L.pbd_warp_taps(8, 8, capi._vp(idx), None, 8, C.byref(P)) == capi.PBD_ERR_CAPACITY and P.value == 4 and not idx.any()
