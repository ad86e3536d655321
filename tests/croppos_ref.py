"""matlab/learning/croppos.m restated in its own 1-based terms (host reference for pbd_croppos; no GPU, no library).

The definition, in words (croppos.m:10-25): the part boxes are rows (x1, y1, x2, y2), 1-based and inclusive.  Their bounding box is the
smallest x1 and y1 and the largest x2 and y2 over all parts (:10-14).  The pad is half the sum of the bounding box's width and height,
each counted inclusively (:17), so it is a multiple of 0.5.  The crop's low corner is the bounding box's low corner minus the pad,
rounded, and not below 1; its high corner is the high corner plus the pad, rounded, and not beyond the image's width and height
(:18-21).  The image is cut to that rectangle (:23) and every box coordinate is moved by the crop's low corner so that the crop's
first pixel is pixel 1 again (:24-25).  MATLAB's round takes halves away from zero (Python's round and numpy's take them to even)."""
import math
from fractions import Fraction

import numpy as np


def matlab_round(v):
    """round() of MATLAB for a Fraction or a float that is a multiple of 0.5: halves away from zero"""
    v = Fraction(v)
    f = math.floor(abs(v) + Fraction(1, 2))
    return f if v >= 0 else -f


def to_matlab(truth):
    """this library's boxes (x, y, width, height), 0-based, covering x .. x + width -> box.xy rows (x1, y1, x2, y2), 1-based inclusive"""
    t = np.asarray(truth, np.int64).reshape(-1, 4)
    return [(int(x) + 1, int(y) + 1, int(x) + int(w) + 1, int(y) + int(h) + 1) for x, y, w, h in t]


def croppos(xy, im_w, im_h):
    """croppos.m on box.xy rows (1-based inclusive) and an im_h x im_w image -> ((x1, y1, x2, y2) of the crop, 1-based inclusive, the
    new box.xy rows); None when im(y1:y2, x1:x2, :) is empty"""
    x1, y1 = min(r[0] for r in xy), min(r[1] for r in xy)
    x2, y2 = max(r[2] for r in xy), max(r[3] for r in xy)
    pad = Fraction(1, 2) * ((x2 - x1 + 1) + (y2 - y1 + 1))
    x1 = max(1, matlab_round(x1 - pad))
    y1 = max(1, matlab_round(y1 - pad))
    x2 = min(im_w, matlab_round(x2 + pad))
    y2 = min(im_h, matlab_round(y2 + pad))
    if x2 < x1 or y2 < y1:
        return None
    return (x1, y1, x2, y2), [(a - x1 + 1, b - y1 + 1, c - x1 + 1, d - y1 + 1) for a, b, c, d in xy]


def croppos_abi(truth, im_w, im_h):
    """the same in this library's convention: (roi (x, y, width, height) of the crop, 0-based corner and pixel counts; truth relative to
    it), or None"""
    got = croppos(to_matlab(truth), im_w, im_h)
    if got is None:
        return None
    (x1, y1, x2, y2), xy = got
    out = np.array([(a - 1, b - 1, c - a, d - b) for a, b, c, d in xy], np.int32)
    return (x1 - 1, y1 - 1, x2 - x1 + 1, y2 - y1 + 1), out
