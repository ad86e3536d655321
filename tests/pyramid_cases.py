"""Frames shared by tests/golden/make_ref_hog.py, tests/test_pyramid_definition_cpu.py and tests/test_gpu_pyramid_definition.py.
Everything is regenerated from seeds; nothing here is read from a file."""
import os

import numpy as np

from partsbaseddetector_amd.model import make_image, make_wide_image
from tests.pyramid_ref import geometry_def

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_hog_v1.npz")
PYRDOWN_SIZES = [(7, 5), (8, 6), (7, 6), (8, 5), (1, 9), (9, 1), (2, 3), (5, 4), (640, 480)]
RESIZE_CASES = [(640, 480, 597, 448), (640, 480, 343, 257), (139, 102, 200, 177), (64, 48, 1, 1), (64, 48, 64, 48), (50, 40, 1, 7),
                (50, 40, 9, 1), (33, 21, 66, 42), (1920, 1080, 1791, 1008)]


def pyramid_resize_cases(w, h, sbin, interval):
    """the pyramid's real ratios 2^(-i / interval): (w, h, ow, oh) of every resized level"""
    g = geometry_def(w, h, sbin, interval)
    return [(w, h, int(g["img_w"][i]), int(g["img_h"][i])) for i in range(interval)]


def checkerboard(w, h, cn=3, square=3):
    yy, xx = np.mgrid[0:h, 0:w]
    b = ((((xx // square) + (yy // square)) & 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(b[:, :, None], 3, axis=2)) if cn == 3 else b


def channel_ties(w, h):
    """Three bands; in each, the three channels carry gradients of EQUAL magnitude (central differences (6, 8), (10, 0), (0, 10): 100
    each) in different directions, the patterns rotated through the channels from band to band — the R, then G, then B preference
    (interleaved channel 2 first, a later one only when strictly greater) decides every interior pixel."""
    assert w <= 30 and h <= 30, "3x + 4y must stay below 256"
    yy, xx = np.mgrid[0:h, 0:w]
    pats = [3 * xx + 4 * yy, 5 * xx, 5 * yy]
    im = np.zeros((h, w, 3), np.uint8)
    for band in range(3):
        sl = slice(band * w // 3, (band + 1) * w // 3)
        for c in range(3):
            im[:, sl, c] = pats[(c + band) % 3][:, sl]
    return im


def single_bright(w, h, cn=3):
    im = np.full((h, w, 3), 7, np.uint8)
    im[h // 2, w // 3] = (255, 200, 90)
    return im if cn == 3 else np.ascontiguousarray(im[..., 0])


def noise(seed, w, h, cn=3):
    im = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return im if cn == 3 else np.ascontiguousarray(im[..., 0])


def fixture_frames():
    """(name, image, sbin) of tests/golden/ref_hog_v1.npz, in order"""
    return [
        ("img72x56_s8", make_image(11, 72, 56), 8),
        ("img33x21_s4", make_image(12, 33, 21), 4),
        ("img50x70_s8", make_image(13, 50, 70), 8),          # 50 / 8 = 6.25 -> 6, 70 / 8 = 8.75 -> 9: visible 72 > 70, the rows-2 clamp
        ("img13x13_s4", make_image(14, 13, 13), 4),          # one output cell
        ("grey61x47_s4", make_image(15, 61, 47, 1), 4),      # grey, replicated into three planes for features.cc
        ("checker40x52_s4", checkerboard(40, 52), 4),
        ("ties30x27_s4", channel_ties(30, 27), 4),
        ("noise44x36_s8", noise(16, 44, 36), 8),             # 44 / 8 = 5.5 -> 6, 36 / 8 = 4.5 -> 5: both clamps, the 0.2 clip
        ("wide16u_37x29_s4", make_wide_image(np.uint16, 17, 37, 29), 4),
        ("wide64f_37x29_s4", make_wide_image(np.float64, 18, 37, 29), 4),
    ]


def hog_frames_u8(big=True):
    """(name, image, sbin): the 8-bit HOG cases of the definition tests"""
    out = []
    for s in (4, 8):
        for n in (49, 50, 51) if s == 4 else (98, 100, 102):         # n / s = k + 0.25 .. k + 0.75 around the k + 0.5 rounding
            out.append((f"img{n}x{n + s // 2 + 1}_s{s}", make_image(n, n, n + s // 2 + 1), s))
        for n in (s * 6 + s // 2 - 1, s * 6 + s // 2, s * 6 + s // 2 + 1):   # exactly below / at / above k + 0.5
            out.append((f"img{n}x{n}_s{s}", make_image(n + 1, n, n), s))
            out.append((f"grey{n}x{2 * n}_s{s}", make_image(n + 2, n, 2 * n, 1), s))
        out.append((f"zero_cells_s{s}", make_image(3, 2 * s, 2 * s), s))        # 8 x 8 at sbin 4: two blocks, no output cell
        out.append((f"one_cell_s{s}", make_image(4, 3 * s, 3 * s + 1), s))
        out.append((f"flat_s{s}", np.full((40, 52, 3), 93, np.uint8), s))
        out.append((f"checker_s{s}", checkerboard(52, 40), s))
        out.append((f"checker_grey_s{s}", checkerboard(45, 38, 1, square=2), s))
        out.append((f"bright_s{s}", single_bright(50, 44), s))
        out.append((f"ties_s{s}", channel_ties(30, 29), s))
        out.append((f"noise_s{s}", noise(5, 70, 59), s))
        out.append((f"noise_grey_s{s}", noise(6, 61, 50, 1), s))
    if big:
        out.append(("img640x480_s4", make_image(0, 640, 480), 4))
        out.append(("img640x480_s8", make_image(0, 640, 480), 8))
        out.append(("img1920x1080_s8", make_image(1, 1920, 1080), 8))
        out.append(("grey1920x1080_s4", make_image(2, 1920, 1080, 1), 4))
    return out


# seeds of hog_frames_wide, per depth: chosen ON THE CPU, from hog_def's own margins alone, so that on no level of the frame's pyramid
# (interval 5) a pixel's orientation margin lies within the float error of the comparison (hog_ref.excused_cells): small levels have
# so few cells that one such pixel would exceed the 0.1 % cap.  The cap is fixed; the frames are chosen to respect it.
WIDE_SEEDS = {"uint16": (21, 21, 21, 25), "float32": (22, 21, 21, 22), "float64": (21, 21, 21, 22)}
WIDE_DETECT_FRAME = (55, 160, 120)   # (seed, w, h) of the 16-bit frame of the detect_image case, chosen the same way for EVERY level of its
                                     # interval-10 pyramid (16-bit gradients reach 1.3e5, where the float error of a dot is 0.03: on 320 x 240
                                     # no seed of 87 tried kept all 36 levels free of near-ties)


def hog_frames_wide():
    """(name, image, sbin): 16-bit / float / double frames (make_wide_image)"""
    out = []
    for kind in (np.uint16, np.float32, np.float64):
        nm = np.dtype(kind).name
        sd = WIDE_SEEDS[nm]
        out.append((f"{nm}_100x75_s4", make_wide_image(kind, sd[0], 100, 75), 4))
        out.append((f"{nm}_101x77_s8", make_wide_image(kind, sd[1], 101, 77), 8))
        out.append((f"{nm}_grey90x70_s4", make_wide_image(kind, sd[2], 90, 70, 1), 4))
        out.append((f"{nm}_200x150_s4", make_wide_image(kind, sd[3], 200, 150), 4))
    return out
