"""The boundary-padding step (pbd_set_boundary_pad) restated in numpy, and the detection it should give composed from the oracle's
stage functions as they are.

The step: every pyramid level's feature map is surrounded by `pad` cells that hold 0 in channels 0..30 and 1 in channel 31
(copyMakeBorder + boundaryOcclusionFeature, src/HOGFeatures.cpp:147-148, body :57-79); the filter bank, the DP and the back-tracking
run on the padded planes unchanged; a part's box origin is (Point(x, y) - Point(1 + pad, 1 + pad)) * scale
(src/DynamicProgram.cpp:239 with the compensation of matlab/detection/detect.m:266-267).

Not a test module: tests/test_boundary_pad_cpu.py checks this restatement against first principles, tests/test_gpu_boundary_pad.py
compares the device with it."""
import numpy as np

from oracle import orc
from partsbaseddetector_amd import capi

FLEN = 32


def pad_features(feat, pad):
    """feat [H, W, 32] -> [H + 2 pad, W + 2 pad, 32]: zero cells around it, channel 31 of every border cell = 1.  A level without
    cells stays as it is."""
    feat = np.asarray(feat)
    H, W, flen = feat.shape
    if pad == 0 or H == 0 or W == 0:
        return feat.copy()
    out = np.zeros((H + 2 * pad, W + 2 * pad, flen), feat.dtype)
    out[pad:pad + H, pad:pad + W] = feat
    out[:pad, :, flen - 1] = 1
    out[pad + H:, :, flen - 1] = 1
    out[:, :pad, flen - 1] = 1
    out[:, pad + W:, flen - 1] = 1
    return out


def boundary_occlusion_literal(feature, flen, padsize):
    """src/HOGFeatures.cpp:64-79 transcribed line by line on the reference's 2-D layout (rows x cols * flen), in place."""
    M, N = feature.shape
    fmstart = padsize - 1
    fnstart = padsize * flen - 1
    fmstop = M - padsize
    fnstop = N - padsize * flen
    for m in range(M):
        for n in range(0, N, flen):
            if m > fmstart and m < fmstop and n > fnstart and n < fnstop:
                continue
            feature[m, n + flen - 1] = 1
    return feature


def copy_make_border_literal(feature2d, top, bottom, left, right):
    """copyMakeBorder(src, dst, top, bottom, left, right, BORDER_CONSTANT, 0) on a 2-D matrix"""
    M, N = feature2d.shape
    out = np.zeros((M + top + bottom, N + left + right), feature2d.dtype)
    out[top:top + M, left:left + N] = feature2d
    return out


def boxes_from_locs(model, comp, locs, scale, pad, dtype=np.float32):
    """locs [n, max_parts, 3] (x, y, mixture) of component `comp` at one level -> boxes [n, max_parts, 4] (x, y, width, height):
    src/DynamicProgram.cpp:238-240 with the origin moved back by the padding; Point * T rounds like cvRound (half to even), the size
    is the chosen mixture's filter rows for both sides (include/Parts.hpp:185-187)."""
    T = np.dtype(dtype).type
    locs = np.asarray(locs)
    n, mp, _ = locs.shape
    boxes = np.zeros((n, mp, 4), np.int32)
    s = T(np.float32(scale))
    org = 1 + pad
    for i in range(n):
        for p in range(model.nparts(comp)):
            x, y, m = (int(v) for v in locs[i, p])
            rows = model.filtersw[model.filterid[comp][p][m]].shape[0]
            sz = int(np.rint(T(rows) * s))
            x1, y1 = int(np.rint(T(x - org) * s)), int(np.rint(T(y - org) * s))
            x2, y2 = x1 + sz - 1, y1 + sz - 1
            boxes[i, p] = (min(x1, x2), min(y1, y2), max(x1, x2) - min(x1, x2), max(y1, y2) - min(y1, y2))
    return boxes


class Composed:
    """The padded detection of one frame, stage by stage: feat[l] [H, W, 32], resp[l] [nf, H, W], rootv[l] / rooti[l] [ncomp, H, W]
    (None for a level without cells), scales[l], and the candidates (heads, boxes, locs) in the device's order (level, component,
    row-major root location)."""


def compose(model, im, pad, dtype=np.float32, correct_ptr=0, levels=None, capacity=8192):
    """Per level: orc.hog of the oracle's level image -> pad -> orc.pdf_level -> orc.dp_min_level -> orc.dp_argmin_level; boxes
    recomputed from locs with the shifted origin.  levels: only these (default: all)."""
    im = np.ascontiguousarray(im)
    cn = 1 if im.ndim == 2 else im.shape[2]
    desc = model.to_desc()
    _, _, _, _, fr = orc.detect(model, im, capacity=1, keep=True, correct_ptr=correct_ptr, desc=desc, dtype=dtype)
    out = Composed()
    out.pad, out.nlevels = pad, fr.nlevels
    out.feat, out.resp, out.rootv, out.rooti, out.scales = [], [], [], [], []
    H_, B_, L_ = [], [], []
    for l in range(fr.nlevels):
        scale = fr.dims[l][4]
        out.scales.append(scale)
        feat = pad_features(orc.hog(fr.image(l, cn, im.dtype if im.dtype in orc.DEPTHS else np.uint8), model.sbin, dtype), pad)
        out.feat.append(feat)
        if feat.shape[0] == 0 or feat.shape[1] == 0 or (levels is not None and l not in levels):
            out.resp.append(None); out.rootv.append(None); out.rooti.append(None)
            continue
        resp = orc.pdf_level(feat, model.filtersw, dtype)
        out.resp.append(resp)
        rvs, ris = [], []
        for c in range(model.ncomponents):
            Ix, Iy, Ik, rv, ri = orc.dp_min_level(desc, c, resp, correct_ptr, dtype)
            rvs.append(rv); ris.append(ri)
            h, b, lc = orc.dp_argmin_level(desc, c, l, scale, rv, ri, Ix, Iy, Ik, capacity=capacity, dtype=dtype)
            H_.append(h); L_.append(lc); B_.append(boxes_from_locs(model, c, lc, scale, pad, dtype))
            out.oracle_boxes = getattr(out, "oracle_boxes", []) + [b]
        out.rootv.append(np.stack(rvs)); out.rooti.append(np.stack(ris))
    fr.free()
    mp = model.max_parts
    out.heads = np.concatenate(H_) if H_ else np.zeros(0, capi.HEAD_DTYPE)
    out.boxes = np.concatenate(B_) if B_ else np.zeros((0, mp, 4), np.int32)
    out.locs = np.concatenate(L_) if L_ else np.zeros((0, mp, 3), np.int32)
    out.oracle_boxes = np.concatenate(out.oracle_boxes) if H_ else np.zeros((0, mp, 4), np.int32)
    return out


def occlusion_trained(model):
    """The synthetic models draw their last channel's weights around -0.1 (the HOG truncation feature is penalised).  A model trained on
    a padded pyramid (matlab/detection/featpyramid.m:37-44) learns that channel as "this cell lies outside the image"; for frames in
    which objects are cut by the border its weights are positive.  This turns a synthetic model into such a one, in place."""
    for f in model.filtersw:
        v = f.reshape(f.shape[0], -1, FLEN)
        v[..., FLEN - 1] = np.abs(v[..., FLEN - 1])
    model._keep = []
    return model
