"""Boundary padding (pbd_set_boundary_pad) without a GPU: the numpy restatement of the step (tests/boundary_pad_ref.py) against
first principles, the frame planner under padding (tests/tools/plan_check_pad.cpp: every invariant of test_plan_cpu.py plus the
padding's own tables), and the host layers' plumbing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import orc
from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import (make_face_like_model, make_image, make_mixed_person_model, make_person_model,
                                          make_tree_model, make_tree_model_k)
from tests import boundary_pad_ref as bp
from tests.util import assert_candidates_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partsbaseddetector_amd", "csrc")
NCU = 256
NAMES = ("pbd_set_boundary_pad", "pbd_get_boundary_pad", "pbd_group_set_boundary_pad")


# ---- the restatement against first principles -----------------------------------------------------------------------------
def thresholded(model, im, pct, dtype=np.float32):
    model.thresh = -1e30
    _, _, _, _, fr = orc.detect(model, im, capacity=1, keep=True, dtype=dtype)
    model.thresh = float(np.float32(np.percentile(np.concatenate([fr.root(l)[0].ravel() for l in range(fr.nlevels)]), pct)))
    fr.free()
    return model


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pad0_reproduces_the_oracle(dtype):
    """compose(pad = 0) is orc.detect: candidates (and so the recomputed boxes), features, responses and root tables, exactly"""
    model = thresholded(make_tree_model_k([-1, 0, 0, 1], [2, 3, 1, 2], seed=9), make_image(3, 200, 150), 99.0, dtype)
    im = make_image(3, 200, 150)
    ref = orc.detect(model, im, keep=True, dtype=dtype)
    got = bp.compose(model, im, 0, dtype)
    assert len(ref[0]) > 0
    assert_candidates_equal((got.heads, got.boxes, got.locs), ref[:3], score_tol=0.0)
    np.testing.assert_array_equal(got.oracle_boxes, ref[1])   # a box recomputed with pad = 0 equals the oracle's own box
    fr = ref[4]
    for l in range(fr.nlevels):
        np.testing.assert_array_equal(got.feat[l], fr.feat(l))
        if got.resp[l] is not None:
            np.testing.assert_array_equal(got.resp[l], fr.resp(l))
            np.testing.assert_array_equal(got.rootv[l], fr.root(l)[0])
    fr.free()


@pytest.mark.parametrize("H,W,pad", [(1, 1, 1), (4, 5, 3), (5, 4, 1), (3, 9, 8), (12, 7, 2), (2, 2, 7)])
def test_border_rule_matches_the_reference_lines(H, W, pad):
    """pad_features == copyMakeBorder(feature, padded, pad, pad, pad * flen, pad * flen, BORDER_CONSTANT, 0) followed by the index
    conditions of boundaryOcclusionFeature (src/HOGFeatures.cpp:68-76), transcribed literally"""
    rng = np.random.default_rng(H * 100 + W * 10 + pad)
    feat = rng.random((H, W, bp.FLEN), np.float32)
    feat[:, :, 31] = 0   # (the HOG truncation feature)
    lit = bp.copy_make_border_literal(feat.reshape(H, W * bp.FLEN), pad, pad, pad * bp.FLEN, pad * bp.FLEN)
    lit = bp.boundary_occlusion_literal(lit, bp.FLEN, pad).reshape(H + 2 * pad, W + 2 * pad, bp.FLEN)
    got = bp.pad_features(feat, pad)
    np.testing.assert_array_equal(got, lit)
    assert got[:, :, 31].sum() == (H + 2 * pad) * (W + 2 * pad) - H * W and (got[pad:pad + H, pad:pad + W] == feat).all()


def test_box_shift_is_the_padding_in_scaled_cells():
    model = make_tree_model([-1, 0], 2, seed=1)
    locs = np.array([[[7, 9, 1], [3, 4, 0]]], np.int32)
    for dtype in (np.float32, np.float64):
        b0 = bp.boxes_from_locs(model, 0, locs, 4.0, 0, dtype)
        b3 = bp.boxes_from_locs(model, 0, locs + np.array([3, 3, 0], np.int32), 4.0, 3, dtype)
        np.testing.assert_array_equal(b0, b3)           # the same image cell -> the same box
        neg = bp.boxes_from_locs(model, 0, np.array([[[0, 2, 0], [0, 0, 0]]], np.int32), 8.0, 3, dtype)
        assert neg[0, 0].tolist() == [-32, -16, 39, 39]  # a root in the ring: (0 - 4) * 8, (2 - 4) * 8, 5 * 8 - 1


def test_padded_oracle_finds_a_root_in_the_ring():
    """the composed oracle itself returns candidates whose root cell lies in the padding ring, with boxes that leave the frame"""
    im = make_image(11, 160, 120)
    model = bp.occlusion_trained(make_tree_model([-1, 0, 0], 2, seed=21))   # (a last channel trained as "outside the image")
    model.thresh = -1e30
    roots = bp.compose(model, im, 3, capacity=1).rootv
    model.thresh = float(np.float32(np.percentile(np.concatenate([r.ravel() for r in roots if r is not None]), 99.0)))
    got = bp.compose(model, im, 3)
    n = 0
    for i in range(len(got.heads)):
        l = got.heads["level"][i]
        H, W = got.rootv[l].shape[1:]
        x, y = got.locs[i, 0, :2]
        bx, by, bw, bh = got.boxes[i, 0]
        if (x < 3 or y < 3 or x >= W - 3 or y >= H - 3) and (bx < 0 or by < 0 or bx + bw >= 160 or by + bh >= 120):
            n += 1
    assert n > 0


# ---- the planner ---------------------------------------------------------------------------------------------------------
PERSON = make_person_model()
CASES = {   # name: (model, frame and handle options, the pad = 0 footprint pinned in tests/test_plan_cpu.py's CASES)
    "person_640_b1": (PERSON, dict(), 350815894),
    "person_640_b4": (PERSON, dict(batch=4), 1403253904),
    "person_1080_compact": (PERSON, dict(w=1920, h=1080), 1476770584),
    "person_640_dp2": (PERSON, dict(dp_mode=2), 214234600),
    "person_640_dp1": (PERSON, dict(dp_mode=1), 507133734),
    "person_640_f64": (PERSON, dict(f64=True), 529673650),
    "mixed_640": (make_mixed_person_model(), dict(), 350858582),
    "face_640": (make_face_like_model(), dict(), 632816892),
    "person_640_levelset": (PERSON, dict(levels=[0, 2, 5, 11, 40]), 223621134),
}
COMPACT = ("person_1080_compact", "person_640_dp2")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = tmp_path_factory.mktemp("planpad") / "plan_check_pad.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "tools"),
                           os.path.join(ROOT, "tests", "tools", "plan_check_pad.cpp"), os.path.join(CSRC, "pbd_plan.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.plan_check_pad.restype = C.c_int
    return lib


def plan(lib, model, pad, w=640, h=480, batch=1, f64=False, dp_mode=0, levels=()):
    desc, fsize = (model.to_desc(), None) if model.is_uniform() else model.to_desc_sized()
    opt = capi.pbd_options(0, capi.PBD_CONV_AUTO, 4096, 0, 0, 0, capi.PBD_SCALAR_F64 if f64 else capi.PBD_SCALAR_F32, 0,
                           (C.c_int32 * 2)(0, dp_mode))
    lv = np.ascontiguousarray(list(levels), np.int32)
    fb, cells, base = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
    rep = C.create_string_buffer(4096)
    rc = lib.plan_check_pad(C.byref(desc), None if fsize is None else fsize.ctypes.data_as(C.c_void_p), int(fsize is not None),
                            C.byref(opt), w, h, 3, batch, capi.PBD_DEPTH_8U, lv.ctypes.data_as(C.c_void_p), len(lv), NCU, pad,
                            C.byref(fb), C.byref(cells), C.byref(base), rep, len(rep))
    return rc, fb.value, cells.value, base.value, rep.value.decode()


@pytest.mark.parametrize("pad", [3, 8])
@pytest.mark.parametrize("name", list(CASES))
def test_padded_plan_invariants_and_cells(planner, name, pad):
    model, kw, _ = CASES[name]
    rc, fb, cells, base, rep = plan(planner, model, pad, **kw)
    assert rc == capi.PBD_OK, rep
    assert cells == base > 0, (cells, base, rep)          # sum over the levels of (cw0 + 2 pad)(ch0 + 2 pad)
    # independent of the planner: the oracle's geometry
    g = orc.geometry(kw.get("w", 640), kw.get("h", 480), model.sbin, model.interval)
    want = sum((int(a) + 2 * pad) * (int(b) + 2 * pad) for a, b in zip(g["cell_w"], g["cell_h"]) if a > 0 and b > 0)
    assert cells == want * kw.get("batch", 1)
    # compact: forced (dp_mode 2) or the responses over 400 MB — of the PADDED planes (person_640_b4 crosses it with 8 cells)
    big = cells * len(model.filtersw) * (8 if kw.get("f64") else 4) > (400 << 20)
    assert rep.startswith("compact") == (name in COMPACT or (big and name != "person_640_dp1")), rep
    legacy = name == "person_640_dp1"
    assert (re.search(r" 0 reduce jobs", rep) is None) == legacy and (re.search(r" 0 folds", rep) is not None) == legacy, rep
    assert re.search(r" 0 ring blocks", rep) is None, rep
    _, fb0, cells0, _, rep0 = plan(planner, model, 0, **kw)
    assert cells > cells0 and (fb > fb0 or rep0.startswith("compact") != rep.startswith("compact"))   # (more memory under the same kind of plan)


@pytest.mark.parametrize("name", list(CASES))
def test_pad0_plan_is_the_unpadded_plan(planner, name):
    model, kw, footprint = CASES[name]
    rc, fb, cells, base, rep = plan(planner, model, 0, **kw)
    assert rc == capi.PBD_OK, rep
    assert fb == footprint, (fb, footprint, rep)
    assert cells == base and " 0 ring blocks" in rep


def test_limits_are_checked_on_padded_sizes(planner):
    """the widest 48-row frame the unpadded planner accepts (bisection; the limit it meets first is the LDS-resident distance
    transform's line length or the 16-bit pointers) is refused with 8 cells of padding: the same limit, met by the padded line"""
    lo, hi = 640, 140000          # accepted, refused (tests/test_plan_cpu.py: test_plan_errors)
    assert plan(planner, PERSON, 0, w=lo, h=48)[0] == capi.PBD_OK and plan(planner, PERSON, 0, w=hi, h=48)[0] == capi.PBD_ERR_UNSUPPORTED
    while hi - lo > 4:
        mid = (lo + hi) // 8 * 4
        if plan(planner, PERSON, 0, w=mid, h=48)[0] == capi.PBD_OK:
            lo = mid
        else:
            hi = mid
    rc, _, _, _, rep = plan(planner, PERSON, 8, w=lo, h=48)
    assert rc == capi.PBD_ERR_UNSUPPORTED and "too large" in rep, (lo, rc, rep)


# ---- host layers and binding ----------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"\b(pbd_[a-z0-9_]+)\s*\(", hdr))
    tune = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libpbd_hip_tune.so"))
    for name in NAMES:
        assert name in declared and name in capi.EXPORTS
        assert hasattr(capi.lib(), name) and hasattr(tune, name)
    assert hasattr(capi.Handle, "set_boundary_pad") and hasattr(capi.Handle, "boundary_pad") and hasattr(capi.Group, "set_boundary_pad")
    assert capi.lib().pbd_abi_version() == capi.PBD_ABI_VERSION == 5
    for cite in ("src/HOGFeatures.cpp:147-148", "src/HOGFeatures.cpp:64-79", "featpyramid.m:37-44", "detect.m:266-267",
                 "src/DynamicProgram.cpp:239"):
        assert cite in hdr, cite


def test_argument_errors_before_any_hip_call():
    L = capi.lib()
    assert L.pbd_set_boundary_pad(None, 3) == capi.PBD_ERR_ARG
    assert L.pbd_group_set_boundary_pad(None, 3) == capi.PBD_ERR_ARG
    assert L.pbd_get_boundary_pad(None) == 0


def test_detector_mirror_keeps_the_setting():
    from partsbaseddetector_amd.detector import PartsBasedDetector
    det = PartsBasedDetector(device=0)
    assert det.boundary_pad == 0
    det.setBoundaryPad(3)
    assert det.boundary_pad == 3
    for bad in (-1, 9):
        with pytest.raises(ValueError):
            det.setBoundaryPad(bad)
    assert det.boundary_pad == 3


def test_host_header_and_demo_take_the_option(tmp_path):
    hpp = open(os.path.join(ROOT, "partsbaseddetector_amd", "host", "pbd_host.hpp")).read()
    assert hpp.count("void setBoundaryPad(int pad)") == 3 and "pbd_set_boundary_pad(h, pad)" in hpp   # Device, HipHOGFeatures, PartsBasedDetector<T>
    demo = os.path.join(ROOT, "partsbaseddetector_amd", "host", "pbd_demo")
    for args, want in ((["--pad", "9", "m.bin", "i.raw", "8", "8", "3"], "--pad N"), (["m.bin", "i.raw", "8", "8", "3", "--pad"], "--pad N"),
                       (["--pad", "x", "m.bin", "i.raw", "8", "8", "3"], "--pad N"),
                       (["--pad", "3", "m.txt", "i.raw", "8", "8", "3"], "Unsupported model format"),     # parsed and removed: the positional arguments are intact
                       (["m.txt", "i.raw", "8", "8", "--pad", "3", "3", "double"], "Unsupported model format"),
                       (["--pad", "3"], "Usage")):
        r = subprocess.run([demo] + args, capture_output=True, text=True, cwd=str(tmp_path))
        assert want in r.stdout, (args, r.stdout, r.stderr)
    assert "[--pad N]" in subprocess.run([demo], capture_output=True, text=True).stdout
