"""The warped positives' test cases, shared by tests/test_warp_cpu.py, tests/test_gpu_warp.py and tests/golden/make_ref_warp.py:
one 96 x 80 make_image frame with 3 channels and with 1, three filters (kh != kw catches a transposed axis), and boxes (x1, y1, x2, y2),
1-based inclusive, that cross every border, exceed the frame, are upsampled, are one pixel, tall, wide, of exactly the window's size
(scale 1 on both axes) and fractional.

`clean`: no pixel of the case's numpy window is a near-tie under tests/hog_ref.excused_cells, so a float HOG of it may be held to
hog_ref's bound with nothing excused.  Columns replicated beyond the right border come out of the x resample equal only up to rounding;
that noise-level dx puts vertical gradients on the exact vv[4] == vv[5] tie, so windows that cross the right border are mostly not
clean (any evaluation order may flip them).  tests/test_warp_cpu.py asserts every flag against excused_cells: the list is verified."""
import numpy as np

from partsbaseddetector_amd.model import make_image, make_tree_model

FW, FH = 96, 80
SEED = 7
FILTERS = [(5, 5, 4), (3, 7, 8), (6, 4, 4)]       # (kh, kw, sbin)
BOXES = {
    "interior": (30, 20, 69, 59),
    "left": (-3, 25, 36, 64),
    "top": (25, -3, 64, 36),
    "bottom": (25, 45, 64, 84),
    "right": (57, 25, 100, 64),
    "right_corner": (70, 60, 96, 80),
    "larger": (-20, -20, 120, 100),
    "upsampled": (40, 30, 45, 34),
    "one_pixel": (50, 40, 50, 40),
    "tall": (20, 10, 27, 70),
    "wide": (10, 30, 90, 37),
    "fractional": (5.5, 7.5, 60.5, 49.5),
}


def exact_box(kh, kw, sbin):
    """a box whose crop is exactly the window's size: scale 1 on both axes (the crop adds one cell on every side)"""
    return (33, 22, 33 + kw * sbin - 1, 22 + kh * sbin - 1)


# (filter index, cn, box name) of the cases that are NOT clean; everything else is
NOT_CLEAN = {(fi, cn, name) for cn in (3, 1) for fi, names in (
    (0, ("right", "right_corner", "larger")),
    (1, ("left", "right", "larger", "upsampled", "tall", "wide", "fractional")),
    (2, ("right", "right_corner", "larger"))) for name in names}


def frame(cn):
    return make_image(SEED, FW, FH, cn)


def model_for(fi, interval=1):
    kh, kw, sbin = FILTERS[fi]
    return make_tree_model([-1, 0, 0], 2, seed=31 + fi, kh=kh, kw=kw, sbin=sbin, interval=interval)


def cases():
    """[dict(name, fi, kh, kw, sbin, cn, box, clean)]"""
    out = []
    for fi, (kh, kw, sbin) in enumerate(FILTERS):
        boxes = dict(BOXES, exact=exact_box(kh, kw, sbin))
        for cn in (3, 1):
            for name, box in boxes.items():
                out.append(dict(name=f"{name}-{kh}x{kw}x{sbin}-cn{cn}", box_name=name, fi=fi, kh=kh, kw=kw, sbin=sbin, cn=cn,
                                box=tuple(float(v) for v in box), clean=(fi, cn, name) not in NOT_CLEAN))
    return out


def boxes_of(fi):
    """the boxes of filter fi, in cases() order -> (names, [n, 4] float64)"""
    kh, kw, sbin = FILTERS[fi]
    b = dict(BOXES, exact=exact_box(kh, kw, sbin))
    return list(b), np.asarray(list(b.values()), np.float64)
