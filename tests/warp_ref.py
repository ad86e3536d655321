"""The warped positives (include/pbd_c.h "warped positives") restated in numpy: warppos.m's crop rectangle, the contributions
algorithm of imresize(window, cropsize, 'bilinear') as the header states it, and the window.  Every double operation is one IEEE
operation in the stated order: numpy's elementwise +, *, / round once and nothing is fused; the tap sums run over p in ascending order
from +0.0.  Boxes are (x1, y1, x2, y2) in the .m files' 1-based inclusive pixel coordinates."""
import numpy as np

F64 = np.float64


def round_away(v):
    """round(), halves away from zero (v - trunc(v) is exact in double)"""
    v = float(v)
    r = float(np.trunc(v))
    if abs(v - r) >= 0.5:
        r += 1.0 if v > 0 else -1.0
    return int(r)


def geometry(box, kh, kw, sbin):
    """-> dict(rect=(X1, Y1, X2, Y2), cw, ch, ow, oh, rows_first, py, px)"""
    x1, y1, x2, y2 = (F64(v) for v in box)
    sb = F64(sbin)
    padx = sb * (x2 - x1 + F64(1)) / F64(kw * sbin)
    pady = sb * (y2 - y1 + F64(1)) / F64(kh * sbin)
    X1, X2 = round_away(x1 - padx), round_away(x2 + padx)
    Y1, Y2 = round_away(y1 - pady), round_away(y2 + pady)
    cw, ch, ow, oh = X2 - X1 + 1, Y2 - Y1 + 1, (kw + 2) * sbin, (kh + 2) * sbin
    sy, sx = F64(oh) / F64(ch), F64(ow) / F64(cw)
    return dict(rect=(X1, Y1, X2, Y2), cw=cw, ch=ch, ow=ow, oh=oh, rows_first=bool(sy <= sx), py=ntaps(ch, oh), px=ntaps(cw, ow))


def ntaps(n_in, n_out):
    s = F64(n_out) / F64(n_in)
    width = F64(2) / s if s < 1 else F64(2)
    return int(np.ceil(width)) + 2


def taps(n_in, n_out):
    """one axis -> (index [n_out, P] int32: 0-based inside the crop, the mirror resolved; weight [n_out, P] float64, normalised)"""
    s = F64(n_out) / F64(n_in)
    width = F64(2) / s if s < 1 else F64(2)
    P = int(np.ceil(width)) + 2
    x = np.arange(1, n_out + 1, dtype=F64)
    u = x / s + F64(0.5) * (F64(1) - F64(1) / s)
    left = np.floor(u - width / F64(2))
    ind = left[:, None] + np.arange(P, dtype=F64)[None, :]
    if s < 1:
        w = s * np.maximum(F64(0), F64(1) - np.abs(s * (u[:, None] - ind)))
    else:
        w = np.maximum(F64(0), F64(1) - np.abs(u[:, None] - ind))
    tot = np.add.accumulate(w, axis=1)[:, -1]          # left to right
    w = w / tot[:, None]
    m = np.mod(ind.astype(np.int64) - 1, 2 * n_in)      # aux = [1 .. n_in, n_in .. 1]
    idx = np.where(m < n_in, m, 2 * n_in - 1 - m)
    return idx.astype(np.int32), w


def _resample(a, idx, w, axis):
    """sum over the taps p = 0 .. P - 1, in that order, from +0.0, of w[:, p] * a[idx[:, p]] along `axis`"""
    a = np.moveaxis(a, axis, 0)
    acc = np.zeros((idx.shape[0],) + a.shape[1:], F64)
    for p in range(idx.shape[1]):
        acc = acc + w[:, p].reshape((-1,) + (1,) * (a.ndim - 1)) * a[idx[:, p]]
    return np.moveaxis(acc, 0, axis)


def crop(im, rect):
    """subarray.m with pad = 1: the replicated-border crop, float64 [ch, cw, 3] (a grey frame replicated to three planes)"""
    im = np.asarray(im)
    if im.ndim == 2:
        im = np.repeat(im[:, :, None], 3, axis=2)
    H, W = im.shape[:2]
    X1, Y1, X2, Y2 = rect
    ys = np.clip(np.arange(Y1, Y2 + 1), 1, H) - 1
    xs = np.clip(np.arange(X1, X2 + 1), 1, W) - 1
    return im[np.ix_(ys, xs)].astype(F64)


def window(im, box, kh, kw, sbin):
    """warppos.m's window of one box: float64 [oh, ow, 3]"""
    g = geometry(box, kh, kw, sbin)
    c = crop(im, g["rect"])
    iy, wy = taps(g["ch"], g["oh"])
    ix, wx = taps(g["cw"], g["ow"])
    if g["rows_first"]:
        return _resample(_resample(c, iy, wy, 0), ix, wx, 1)
    return _resample(_resample(c, ix, wx, 1), iy, wy, 0)


def column_ref(model, feat, filter, bias, id, cpos, wreg, w0, k):
    """qp_poswrite (train.m:152-161) through tests/qp_ref.py's standardisation: the column of one window's features [kh, kw, 32] ->
    (x [k] float32, ids [5] int32, b float32, d float64)"""
    from tests import qp_ref
    lay = model.feature_layout()
    x = np.zeros(k, np.float32)
    C = F64(cpos)
    bl = [(lay["bias"] + int(bias), np.ones(1, F64)), (int(lay["filters"][filter]), np.asarray(feat).ravel().astype(F64))]
    x[0] = len(bl)
    xp, norm, bs = 1, 0.0, 1.0
    for s, v in bl:
        xs = (C * v) / wreg[s:s + len(v)]
        x[xp], x[xp + 1] = s + 1, s + len(v)
        x[xp + 2:xp + 2 + len(v)] = xs.astype(np.float32)
        norm = norm + qp_ref.block_sum(xs * xs)
        bs = bs - qp_ref.block_sum(w0[s:s + len(v)] * v)
        xp += 2 + len(v)
    return x, np.array([1, id, 0, 0, 0], np.int32), np.float32(C * F64(bs)), F64(norm)
