"""The feature vector of a detection (pbd_feature_block, include/pbd_c.h), restated in numpy from the contract there.

For a record at plan level n of component c with part locations (x_p, y_p, m_p) and q the parent of p, part p contributes one block:
  bias_id   = biasid[p][m_p] + m_q; the root: biasid[0][0].  Value 1.
  def_id    = defid[p][m_p]; -1 for the root.
  def       = (-(dx dx), -dx, -(dy dy), -dy), dx = x_q + anchor_x - x_p, dy alike, the anchor of the same defid: integers, negated as
              integers, widened to double; zeros for the root.
  filter_id = filterid[p][m_p], kh x kw that filter's size.
  window    : win[i][j][ch] = feat[n](y_p - kh // 2 + i, x_p - kw // 2 + j, ch); a cell outside the plane reads 0 in channels
              0 .. flen - 2 and 1 in channel flen - 1.  The feature values themselves, in T.

The window bound.  The oracle's response (oracle/pbd_oracle_T.inc orc_pdf_one, the order of src/filter.cpp + pdf += pdfc) is, per
channel, s = sum over the kh kw taps of f v accumulated in T from 0, then out += s over the flen channels.  A product f v is rounded
once, then takes part in at most kh kw - 1 additions of its channel's chain (the first one, 0 + f v, is exact) and at most flen - 1
additions of the channel chain (the first is exact again): fewer than n = kh kw + flen roundings (1 + d_k), |d_k| <= u, the unit
roundoff of T.  So computed = sum f v (1 + t), |t| <= g_{n-1} (Higham, Accuracy and Stability, Lemma 3.1), and
|computed - exact| <= g_{n-1} sum |f v|.  dot64 below returns the exact sum rounded ONCE to double (error <= u64 sum |f v|), so
|computed - dot64| <= g_n sum |f v| = n u / (1 - n u) sum |f v| for float and double alike.  Nothing here is a measured number."""
import math

import numpy as np

FLEN = 32
F64 = np.float64
BLOCK_DTYPE = np.dtype([("bias_id", np.int32), ("def_id", np.int32), ("filter_id", np.int32), ("kh", np.int32), ("kw", np.int32),
                        ("reserved", np.int32), ("def", np.float64, (4,))])
SLIPS = ("anchor", "border", "swap", "defid", "sign")   # the five slips tests/test_feature_vector_cpu.py must notice


def unit_roundoff(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.dtype(np.float64) else 2.0 ** -24


def window_ref(feat, x, y, kh, kw, slip=None):
    """[kh, kw * flen] in feat's dtype.  slip: "anchor" = (k - 1) // 2, "border" = 0 in the last channel, "swap" = x and y swapped"""
    H, W, flen = feat.shape
    ay, ax = (((kh - 1) // 2, (kw - 1) // 2) if slip == "anchor" else (kh // 2, kw // 2))
    if slip == "swap":
        x, y = y, x
    win = np.zeros((kh, kw, flen), feat.dtype)
    if slip != "border":
        win[:, :, flen - 1] = 1
    y0, x0 = y - ay, x - ax
    i0, i1, j0, j1 = max(0, -y0), min(kh, H - y0), max(0, -x0), min(kw, W - x0)
    if i0 < i1 and j0 < j1:
        win[i0:i1, j0:j1] = feat[y0 + i0:y0 + i1, x0 + j0:x0 + j1]
    return win.reshape(kh, kw * flen)


def _products(filt, win):
    """the products f v as float64 numbers whose sum is exact: a float32 f times a float32 v is a double; a double v is split into a
    26-bit head and the tail (Veltkamp), each times f exact"""
    f = np.asarray(filt, np.float32).astype(F64).ravel()
    v = np.asarray(win)
    if v.dtype == np.float32:
        return f * v.astype(F64).ravel()
    v = v.astype(F64).ravel()
    c = v * (2.0 ** 27 + 1.0)
    hi = c - (c - v)
    return np.concatenate([f * hi, f * (v - hi)])


def dot64(filt, win):
    """filter . window: the exact sum of the products, rounded once to double"""
    return math.fsum(_products(filt, win).tolist())


def window_bound(filt, win, dtype):
    """n u / (1 - n u) sum |f v|, n = kh kw + flen, u = the unit roundoff of T (derived in the module docstring)"""
    f = np.asarray(filt, np.float32).astype(F64)
    n = f.size // FLEN + FLEN
    u = unit_roundoff(dtype)
    return n * u / (1.0 - n * u) * float(np.abs(f.ravel() * np.asarray(win, F64).ravel()).sum())


def feature_vector_ref(model, feat_of_level, heads, locs, dtype, slip=None):
    """(blocks [n, max_parts] BLOCK_DTYPE, windows [n, max_parts, wmax] dtype) as pbd_candidates_features returns them: a smaller
    window at the front of its slot, the tail zero; part slots beyond nparts hold ids -1 and zeros.  feat_of_level(l) -> [H, W, 32].
    slip: one of SLIPS ("defid": the PARENT's mixture selects defid and anchor; "sign": def without the minus)"""
    n, mp = len(heads), model.max_parts
    sizes = model.filter_sizes()
    wmax = int((sizes[:, 0] * sizes[:, 1]).max()) * model.flen
    blocks = np.zeros((n, mp), BLOCK_DTYPE)
    for k in ("bias_id", "def_id", "filter_id"):
        blocks[k] = -1
    windows = np.zeros((n, mp, wmax), dtype)
    anchors = np.asarray(model.anchors, np.int64).reshape(-1, 2)
    cache = {}
    for i in range(n):
        c, l = int(heads["component"][i]), int(heads["level"][i])
        if l not in cache:
            cache[l] = np.asarray(feat_of_level(l))
            assert cache[l].dtype == np.dtype(dtype)
        feat = cache[l]
        P = model.nparts(c)
        assert int(heads["nparts"][i]) == P
        for p in range(P):
            x, y, m = (int(v) for v in locs[i, p])
            b = blocks[i, p]
            f = model.filterid[c][p][m]
            kh, kw = int(sizes[f, 0]), int(sizes[f, 1])
            b["filter_id"], b["kh"], b["kw"] = f, kh, kw
            windows[i, p, :kh * kw * model.flen] = window_ref(feat, x, y, kh, kw, slip).ravel()
            if p == 0:
                b["bias_id"] = model.biasid[c][0][0]
                continue
            q = model.parentid[c][p]
            xq, yq, mq = (int(v) for v in locs[i, q])
            b["bias_id"] = model.biasid[c][p][m] + mq
            did = model.defid[c][p][min(mq, len(model.defid[c][p]) - 1) if slip == "defid" else m]
            dx = xq + int(anchors[did, 0]) - x
            dy = yq + int(anchors[did, 1]) - y
            sgn = 1 if slip == "sign" else -1
            b["def_id"] = did
            b["def"] = [F64(sgn * (dx * dx)), F64(sgn * dx), F64(sgn * (dy * dy)), F64(sgn * dy)]
    return blocks, windows


def wx(w, x):
    """w . x per record, each the exact sum of its float64 products rounded once; and sum |w x| (the "terms")"""
    w = np.asarray(w, F64)
    out, mag = np.zeros(len(x), F64), np.zeros(len(x), F64)
    for i, xi in enumerate(np.asarray(x, F64)):
        nz = np.flatnonzero(xi)
        t = w[nz] * xi[nz]
        out[i], mag[i] = math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())
    return out, mag


def window_bounds(model, blocks, windows, dtype):
    """per record: the sum of window_bound over its parts"""
    out = np.zeros(len(blocks), F64)
    for i in range(len(blocks)):
        for p in range(blocks.shape[1]):
            f = int(blocks[i, p]["filter_id"])
            if f >= 0:
                filt = np.asarray(model.filtersw[f])
                out[i] += window_bound(filt, windows[i, p, :filt.size], dtype)
    return out
