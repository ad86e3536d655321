"""Latent positives (include/pbd_c.h "latent positives") without a GPU: the new entry points are declared, exported and bound; NULL
arguments are refused before anything touches a device; pbd_croppos against tests/croppos_ref.py (croppos.m restated in MATLAB's
1-based terms); and the route of a latent-positive frame (tests/tools/latent_write_route_check.cpp over pbd_route.hpp).  The write
itself: tests/test_gpu_latent_write.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from tests import croppos_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partsbaseddetector_amd", "csrc")
SYMBOLS = ["pbd_qp_write_latent_u8", "pbd_qp_write_latent_dev_u8", "pbd_qp_write_latent_batch_u8", "pbd_croppos"]


def test_symbols_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "pbd_c.h")) as f:
        header = f.read()
    L = capi.lib()
    for name in SYMBOLS:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in capi.EXPORTS and getattr(L, name) is not None, name
    assert re.search(r"^typedef struct pbd_latent_example \{", header, re.M)
    assert re.search(r"#define PBD_ABI_VERSION 5\b", header) and L.pbd_abi_version() == 5
    # one fixed block per frame, the size the header states
    assert capi.LATENT_EXAMPLE_DTYPE.itemsize == 32 and "32 bytes" in header
    assert capi.LATENT_EXAMPLE_DTYPE.names == ("found", "written", "component", "level", "x", "y", "score")
    for name in ("write_latent", "write_latent_dev", "write_latent_batch"):
        assert hasattr(capi.QpCache, name), name
    assert callable(capi.croppos)
    from partsbaseddetector_amd import PartsBasedDetector
    assert hasattr(PartsBasedDetector, "latentPositives")


def test_null_arguments():
    L = capi.lib()
    im = np.zeros((8, 8, 3), np.uint8)
    p = im.ctypes.data_as(C.c_void_p)
    truth = np.zeros((4, 4), np.int32)
    t = truth.ctypes.data_as(C.c_void_p)
    out = np.full(1, 7, capi.LATENT_EXAMPLE_DTYPE)
    o = out.ctypes.data_as(C.c_void_p)
    ids = (C.c_int32 * 1)(0)
    ptrs = (C.c_void_p * 1)(im.ctypes.data)
    assert L.pbd_qp_write_latent_u8(None, p, 8, 8, 3, 24, t, None, -1, C.c_double(.5), 0, o) == capi.PBD_ERR_ARG
    assert L.pbd_qp_write_latent_dev_u8(None, p, 8, 8, 3, 24, t, None, -1, C.c_double(.5), 0, o) == capi.PBD_ERR_ARG
    assert L.pbd_qp_write_latent_batch_u8(None, ptrs, 1, 8, 8, 3, 24, t, None, -1, C.c_double(.5), ids, o) == capi.PBD_ERR_ARG
    assert L.pbd_qp_write_latent_u8(None, None, 8, 8, 3, 24, None, None, -1, C.c_double(.5), 0, None) == capi.PBD_ERR_ARG
    assert (out["found"] == 7).all() and (out["score"] == 7).all()
    roi = np.zeros(4, np.int32)
    r = roi.ctypes.data_as(C.c_void_p)
    assert L.pbd_croppos(None, 1, 8, 8, r, None) == capi.PBD_ERR_ARG
    assert L.pbd_croppos(t, 1, 8, 8, None, None) == capi.PBD_ERR_ARG
    assert L.pbd_croppos(t, 0, 8, 8, r, None) == capi.PBD_ERR_ARG
    assert L.pbd_croppos(t, 1, 8, 8, r, None) == capi.PBD_OK          # truth_out may be NULL
    neg = np.array([[1, 1, -1, 2]], np.int32)
    assert L.pbd_croppos(neg.ctypes.data_as(C.c_void_p), 1, 8, 8, r, None) == capi.PBD_ERR_ARG


# name -> (truth (x, y, width, height) rows, frame width, frame height)
CROPS = {
    "inside": ([[60, 50, 20, 30], [70, 60, 10, 10], [65, 85, 12, 9]], 400, 300),
    "inside_odd_pad": ([[60, 50, 21, 30], [70, 60, 10, 10]], 400, 300),             # the extent sum is odd: pad is a half
    "touch_left": ([[0, 40, 20, 30], [5, 50, 10, 10]], 200, 200),
    "touch_top": ([[40, 0, 20, 30], [45, 5, 10, 10]], 200, 200),
    "touch_right": ([[170, 40, 29, 30], [180, 50, 10, 10]], 200, 200),              # x + width = w - 1: the last pixel column
    "touch_bottom": ([[40, 170, 20, 29], [45, 175, 10, 10]], 200, 200),
    "clip_left_only": ([[10, 120, 30, 20]], 400, 300),                              # pad 26: reaches over the left border alone
    "clip_bottom_only": ([[150, 270, 20, 20]], 400, 300),
    "neg_half": ([[3, 100, 4, 3]], 300, 300),                                       # X1 = 4, pad = 4.5: X1 - pad = -0.5 -> round -1 (not 0)
    "neg_half_far": ([[0, 0, 6, 3]], 300, 300),                                     # X1 = 1, pad = 5.5: -4.5 -> -5; Y1 - pad = -4.5 too
    "neg_half_y": ([[100, 2, 3, 6]], 300, 300),                                     # Y1 = 3, pad = 5.5: -2.5 -> -3
    "single_part": ([[100, 90, 24, 24]], 320, 240),
    "frame_filled": ([[0, 0, 63, 47]], 64, 48),
    "partly_outside": ([[-10, -5, 30, 30], [180, 190, 40, 40]], 200, 200),          # boxes over the border: the crop is the frame's part
}


@pytest.mark.parametrize("name", sorted(CROPS))
def test_croppos_against_the_matlab_restatement(name):
    truth, w, h = CROPS[name]
    want = croppos_ref.croppos_abi(truth, w, h)
    assert want is not None
    roi, out = capi.croppos(truth, len(truth), w, h)
    assert roi == tuple(int(v) for v in want[0]), (roi, want[0])
    np.testing.assert_array_equal(out, want[1])
    t = np.asarray(truth, np.int32)
    # what the definition implies: the crop lies in the frame, sizes are unchanged, the shift is the crop's corner
    assert roi[0] >= 0 and roi[1] >= 0 and roi[2] >= 1 and roi[3] >= 1 and roi[0] + roi[2] <= w and roi[1] + roi[3] <= h
    np.testing.assert_array_equal(out[:, 2:], t[:, 2:])
    np.testing.assert_array_equal(out[:, :2], t[:, :2] - np.array(roi[:2], np.int32))


def test_croppos_negative_halves_round_away_from_zero():
    """round(X1 - pad) for a negative half: MATLAB gives -1 for -0.5 where round-half-even and floor(v + .5) give 0 — invisible behind
    max(1, .), so the reference's rounding is pinned on its own, and the cases above on the high side (X2 + pad a positive half)"""
    assert [croppos_ref.matlab_round(v) for v in (-0.5, -1.5, -4.5, 0.5, 1.5, 2.5, -2.0, 3.0)] == [-1, -2, -5, 1, 2, 3, -2, 3]
    # X1 = Y1 = 11, X2 = 19, Y2 = 16, pad = 7.5: round(26.5) = 27 where half-even gives 26; round(23.5) = 24; round(3.5) = 4
    (x1, y1, x2, y2), _ = croppos_ref.croppos(croppos_ref.to_matlab([[10, 10, 8, 5]]), 400, 400)
    assert (x1, y1, x2, y2) == (4, 4, 27, 24)
    assert capi.croppos([[10, 10, 8, 5]], 1, 400, 400)[0] == (3, 3, 24, 21)


@pytest.mark.parametrize("truth", [[[500, 10, 20, 20]], [[10, 700, 20, 20]], [[-200, 10, 20, 20], [-190, 15, 5, 5]], [[10, -300, 30, 30]]],
                         ids=["right", "below", "left", "above"])
def test_croppos_refuses_a_truth_wholly_outside(truth):
    assert croppos_ref.croppos_abi(truth, 200, 200) is None
    with pytest.raises(capi.PbdError) as e:
        capi.croppos(truth, len(truth), 200, 200)
    assert e.value.code == capi.PBD_ERR_ARG


def test_croppos_in_place_and_random_cases():
    L = capi.lib()
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(1, 6))
        w, h = int(rng.integers(20, 300)), int(rng.integers(20, 300))
        t = np.stack([rng.integers(-20, w + 10, n), rng.integers(-20, h + 10, n), rng.integers(0, 80, n), rng.integers(0, 80, n)], 1).astype(np.int32)
        want = croppos_ref.croppos_abi(t, w, h)
        roi = np.zeros(4, np.int32)
        buf = t.copy()
        rc = L.pbd_croppos(buf.ctypes.data_as(C.c_void_p), n, w, h, roi.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p))   # truth_out = truth
        if want is None:
            assert rc == capi.PBD_ERR_ARG
            continue
        assert rc == capi.PBD_OK and tuple(roi) == tuple(want[0])
        np.testing.assert_array_equal(buf, want[1])


def test_route_of_a_latent_positive_frame(tmp_path):
    exe = tmp_path / "latent_write_route_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "tools", "latent_write_route_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures"), r.stdout + r.stderr
