"""The MATLAB pyramid kind (pbd_set_pyramid_kind, PBD_PYRAMID_MATLAB) without a GPU: the numpy restatement of
matlab/detection/featpyramid.m:13-34 (tests/matlab_pyramid_ref.py) against the outputs of the compiled matlab/mex/resize.cc and
matlab/mex/reduce.cc (tests/golden/ref_matpyr_v1.npz), equal bits; the host planner's geometry, tap lists and pyramid jobs
(tests/tools/plan_check_matpyr.cpp) against the restatement; and the C ABI's, the binding's and the host layers' surface."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_person_model, make_tree_model
from tests import matlab_pyramid_ref as mp
from tests.hog_ref import excused_cells, hog_def
from tests.pyramid_cases import noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partsbaseddetector_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_matpyr_v1.npz")
NAMES = ("pbd_set_pyramid_kind", "pbd_get_pyramid_kind", "pbd_resize_area_f64", "pbd_reduce_f64")
GEOMETRIES = [(96, 80), (37, 29), (640, 480)]
INTERVALS = [2, 3, 10]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


# ---- the restatement against the compiled reference files ---------------------------------------------------------------------
def test_fixture_holds_every_case(golden):
    names = [n for n, _, _ in mp.resize_cases()] + [n for n, _ in mp.reduce_cases()]
    for interval in mp.PYRAMID_INTERVALS:
        g = mp.geometry_matlab(mp.PYRAMID_FRAME[1], mp.PYRAMID_FRAME[2], mp.PYRAMID_SBIN, interval)
        names += [f"pyr_i{interval}_l{l}" for l in range(g["nlevels"])]
    assert sorted(names) == sorted(golden.files)
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("case", mp.resize_cases(), ids=lambda c: c[0])
def test_resize_restatement_equals_the_compiled_reference(golden, case):
    name, im, scale = case
    assert same_bits(mp.resize_def(im, scale), golden[name].reshape(golden[name].shape[:2] + im.shape[2:])), name


def test_resize_at_scale_one_is_the_identity_and_larger_scales_are_refused():
    im = mp.doubles(5, 23, 31)
    assert same_bits(mp.resize_def(im, 1.0), im)
    with pytest.raises(ValueError):
        mp.resize_def(im, 1.0000001)


def test_the_tap_dropping_rule_is_exercised():
    """2001 -> 2000 and 1001 -> 1000: a partial tap that covers k / 2000 (k / 1000) of a source pixel is dropped where that is
    <= 1e-3 (resize.cc:44,59): those destination indices keep ONE tap, and their weights no longer sum to 1"""
    for s, d, dropped in ((2001, 2000, [0, 1, 1999]), (1001, 1000, [0])):
        taps = mp.resize_taps(s, d)
        short = [i for i, run in enumerate(taps) if abs(sum(a for _, a in run) - 1.0) > 1e-6]
        print(f"{s} -> {d}: destination indices with a dropped tap: {short}")
        assert short == dropped and all(len(taps[i]) == 1 for i in short)
        assert all(len(run) == 2 for i, run in enumerate(taps) if i not in short)


def test_reduce_restatement_equals_the_compiled_reference(golden):
    for name, im in mp.reduce_cases():
        assert same_bits(mp.reduce_def(im), golden[name]), name


@pytest.mark.parametrize("interval", mp.PYRAMID_INTERVALS)
def test_pyramid_restatement_equals_the_compiled_reference(golden, interval):
    g, lv = mp.pyramid_def(noise(*mp.PYRAMID_FRAME), mp.PYRAMID_SBIN, interval)
    assert g["nlevels"] >= interval + 2          # (more than one reduced octave member)
    for l, a in enumerate(lv):
        assert same_bits(a, golden[f"pyr_i{interval}_l{l}"]), (interval, l)
    assert same_bits(lv[0], noise(*mp.PYRAMID_FRAME).astype(np.float64))   # level 0 is the frame, converted


def test_no_near_tie_pixel_on_the_float_hog_frame():
    """The float-handle HOG check of tests/test_gpu_matlab_pyramid.py excuses cells around near-tie pixels (hog_ref.excused_cells) and
    caps them at 0.1 % per level; on levels this small one such pixel would excuse over 10 %.  On this frame at sbin 4, interval 2
    there is none on any level, so the GPU test excludes nothing."""
    g, lv = mp.pyramid_def(noise(*mp.PYRAMID_FRAME), 4, 2)
    for l, im in enumerate(lv):
        feat, margin, det = hog_def(im, 4, details=True)
        mask, nbad = excused_cells(margin, det, feat.shape[:2])
        assert nbad == 0 and not mask.any(), (l, nbad)


# ---- the host planner ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = tmp_path_factory.mktemp("planmat") / "plan_check_matpyr.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC,
                           os.path.join(ROOT, "tests", "tools", "plan_check_matpyr.cpp"), os.path.join(CSRC, "pbd_plan.cpp"), "-o", str(so)])
    return C.CDLL(str(so))


def planner_geometry(lib, w, h, sbin, interval):
    n = C.c_int(0)
    a = [np.zeros(128, np.int32) for _ in range(4)]
    sc = np.zeros(128, np.float32)
    if lib.matpyr_geometry(w, h, sbin, interval, C.byref(n), *[x.ctypes.data_as(C.c_void_p) for x in a], sc.ctypes.data_as(C.c_void_p)):
        return None
    k = n.value
    return dict(nlevels=k, img_w=a[0][:k], img_h=a[1][:k], cell_w=a[2][:k], cell_h=a[3][:k], scales=sc[:k])


@pytest.mark.parametrize("interval", INTERVALS)
@pytest.mark.parametrize("wh", GEOMETRIES)
@pytest.mark.parametrize("sbin", [4, 8])
def test_planner_geometry_and_taps_equal_the_restatement(planner, wh, interval, sbin):
    w, h = wh
    want, got = mp.geometry_matlab(w, h, sbin, interval), planner_geometry(planner, w, h, sbin, interval)
    assert (want is None) == (got is None), (want, got)
    if want is None:
        return
    assert got["nlevels"] == want["nlevels"]
    for k in ("img_w", "img_h", "cell_w", "cell_h", "scales"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    for i in range(interval):
        for slen, dlen in ((h, int(want["img_h"][i])), (w, int(want["img_w"][i]))):
            cap = 4 * slen + 16
            first, count, si = (np.zeros(cap, np.int32) for _ in range(3))
            alpha = np.zeros(cap, np.float64)
            nt = planner.matpyr_taps(slen, dlen, *[x.ctypes.data_as(C.c_void_p) for x in (first, count, si, alpha)], cap)
            runs = mp.resize_taps(slen, dlen)
            flat = [t for run in runs for t in run]
            assert nt == len(flat)
            assert [int(c) for c in count[:dlen]] == [len(r) for r in runs]
            assert [int(f) for f in first[:dlen]] == list(np.cumsum([0] + [len(r) for r in runs[:-1]]))
            assert [int(s) for s in si[:nt]] == [s for s, _ in flat]
            assert same_bits(alpha[:nt], np.array([a for _, a in flat]))


def test_geometry_is_featpyramid_not_the_opencv_one():
    """640 x 480, sbin 8, interval 10: featpyramid.m:15 gives 1 + floor(log(480 / 40) / log(2^0.1)) levels, the first octave's sizes
    are C-rounded products and level 10 is exactly round(0.5 * level 0)"""
    g = mp.geometry_matlab(640, 480, 8, 10)
    assert g["nlevels"] == 36 and (g["img_w"][0], g["img_h"][0]) == (640, 480) and (g["img_w"][10], g["img_h"][10]) == (320, 240)
    assert g["scales"][0] == 8.0 and g["scales"][10] == 16.0 and g["scales"][20] == 32.0
    assert mp.c_round(2.5) == 3 and mp.c_round(0.5) == 1 and mp.c_round(1.4999) == 1      # halves away from zero


def plan(lib, model, w, h, cn=3, batch=1, depth=capi.PBD_DEPTH_8U, kind=capi.PBD_PYRAMID_MATLAB, pad=0, f64=False):
    desc = model.to_desc()
    opt = capi.pbd_options(0, capi.PBD_CONV_AUTO, 4096, 0, 0, 0, capi.PBD_SCALAR_F64 if f64 else capi.PBD_SCALAR_F32, 0, (C.c_int32 * 2)(0, 0))
    out = (C.c_ulonglong * 6)()
    rep = C.create_string_buffer(4096)
    rc = lib.matpyr_plan(C.byref(desc), C.byref(opt), w, h, cn, batch, depth, kind, pad, out, rep, len(rep))
    return rc, list(out), rep.value.decode()


@pytest.mark.parametrize("case", [dict(w=96, h=80), dict(w=96, h=80, cn=1), dict(w=96, h=80, batch=2, pad=3), dict(w=640, h=480),
                                  dict(w=640, h=480, batch=4, f64=True), dict(w=1920, h=1080)], ids=str)
def test_planned_pyramid_jobs_stay_inside_their_buffers(planner, case):
    model = make_person_model() if case["w"] > 96 else make_tree_model([-1, 0, 0], 2, seed=3, interval=2)
    rc, out, rep = plan(planner, model, **case)
    assert rc == capi.PBD_OK, rep
    g = mp.geometry_matlab(case["w"], case["h"], model.sbin, model.interval)
    cn, batch = case.get("cn", 3), case.get("batch", 1)
    assert out[0] == 8 * cn * batch * sum(int(a) * int(b) for a, b in zip(g["img_w"], g["img_h"]))     # double level images
    assert out[1] == case["w"] * case["h"] * cn * batch and out[2:4] == [8, 1]                         # an 8-bit frame buffer
    assert out[4] == batch * g["nlevels"] and out[5] == -(-g["nlevels"] // model.interval)             # one launch per octave
    rc0, out0, rep0 = plan(planner, model, kind=capi.PBD_PYRAMID_OPENCV, **case)
    assert rc0 == capi.PBD_OK and out0[2:4] == [1, 1], rep0


def test_planner_refusals(planner):
    model = make_person_model()
    for depth in (capi.PBD_DEPTH_16U, capi.PBD_DEPTH_32F, capi.PBD_DEPTH_64F):
        rc, _, rep = plan(planner, model, 640, 480, depth=depth)
        assert rc == capi.PBD_ERR_UNSUPPORTED and "8-bit" in rep, rep
        assert plan(planner, model, 640, 480, depth=depth, kind=capi.PBD_PYRAMID_OPENCV)[0] == capi.PBD_OK
    rc, _, rep = plan(planner, model, 30, 30)                 # fewer levels than the interval
    assert rc == capi.PBD_ERR_ARG, rep
    # 12000 x 8000 x 3 doubles: level 0 alone is 2.3 GB, over the 2 GiB the plan gives the double level images
    rc, _, rep = plan(planner, model, 12000, 8000)
    assert rc == capi.PBD_ERR_UNSUPPORTED and "budget" in rep, rep
    assert "budget" not in plan(planner, model, 12000, 8000, kind=capi.PBD_PYRAMID_OPENCV)[2]
    rc, _, rep = plan(planner, model, 4000, 3000, batch=8)    # the budget holds for the whole batch
    assert rc == capi.PBD_ERR_UNSUPPORTED and "budget" in rep, rep


# ---- C ABI, binding, host layers ----------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"\b(pbd_[a-z0-9_]+)\s*\(", hdr))
    tune = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libpbd_hip_tune.so"))
    for name in NAMES:
        assert name in declared and name in capi.EXPORTS
        assert hasattr(capi.lib(), name) and hasattr(tune, name)
    assert re.search(r"#define\s+PBD_PYRAMID_OPENCV\s+0\b", hdr) and re.search(r"#define\s+PBD_PYRAMID_MATLAB\s+1\b", hdr)
    assert (capi.PBD_PYRAMID_OPENCV, capi.PBD_PYRAMID_MATLAB) == (0, 1)
    assert capi.lib().pbd_abi_version() == capi.PBD_ABI_VERSION == 5
    for cite in ("featpyramid.m:13-34", "resize.cc:94-95", "resize.cc:82-106", "reduce.cc:50-70", "reduce.cc:58-59", "resize.cc:90"):
        assert cite in hdr, cite
    for attr in ("set_pyramid_kind", "pyramid_kind", "resize_area", "reduce"):
        assert hasattr(capi.Handle, attr), attr
    assert not hasattr(capi.Group, "set_pyramid_kind")        # groups get no setter


def test_argument_errors_before_any_hip_call():
    L = capi.lib()
    im, out = np.zeros((8, 8, 3)), np.zeros((8, 8, 3))
    ow, oh = C.c_int(0), C.c_int(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.pbd_set_pyramid_kind(None, capi.PBD_PYRAMID_MATLAB) == capi.PBD_ERR_ARG
    assert L.pbd_get_pyramid_kind(None) == capi.PBD_PYRAMID_OPENCV
    assert L.pbd_resize_area_f64(None, p(im), 8, 8, 3, C.c_double(0.5), p(out), C.byref(ow), C.byref(oh)) == capi.PBD_ERR_ARG
    assert L.pbd_reduce_f64(None, p(im), 8, 8, 3, p(out), C.byref(ow), C.byref(oh)) == capi.PBD_ERR_ARG


def test_detector_mirror_keeps_the_setting():
    from partsbaseddetector_amd.detector import PartsBasedDetector
    det = PartsBasedDetector(device=0)
    assert det.pyramid_kind == "opencv"
    det.setPyramidKind("matlab")
    assert det.pyramid_kind == "matlab"
    with pytest.raises(ValueError):
        det.setPyramidKind("gaussian")
    assert det.pyramid_kind == "matlab"
    det.setPyramidKind("opencv")
    assert det.pyramid_kind == "opencv"


def test_host_layer_and_demo_surface():
    hpp = open(os.path.join(ROOT, "partsbaseddetector_amd", "host", "pbd_host.hpp")).read()
    assert hpp.count("void setPyramidKind(int kind)") == 3           # Device, HipHOGFeatures, PartsBasedDetector<T>
    assert "pbd_set_pyramid_kind(h, kind)" in hpp and "pyramid_kind_ != PBD_PYRAMID_OPENCV" in hpp
    demo = open(os.path.join(ROOT, "partsbaseddetector_amd", "host", "demo.cpp")).read()
    assert '"--matlab-pyramid"' in demo and "setPyramidKind(PBD_PYRAMID_MATLAB)" in demo
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_pyramid_mat.o" in mk
