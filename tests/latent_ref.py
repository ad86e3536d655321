"""Test helper: latent detection by definition (include/pbd_c.h "latent detection"; matlab/detection/detect.m:18-23, 60-101, 342-376) in
numpy float64 on top of the oracle's DP.  No GPU import.

  window of (part p, mixture m, cell (x, y)) at a level of scale s: sz = rint(T(rows) * s), x1 = rint(T(x - org) * s), y1 alike,
      org = 1 + pad, rows = the rows of the mixture's filter, products in T (the box DynamicProgram::argmin reports there);
  overlap with the truth (tx, ty, tw, th), which covers tx .. tx + tw: w = max(0, min(x2, bx2) - max(x1, bx1) + 1), h alike,
      inter = h w, area = sz sz, box = (tw + 1)(th + 1), admissible iff inter / (area + box - inter) > overlap;
  mask: inadmissible cells of plane (p, m) become -1e10; with mix[p] = m0 every other plane of p is -1e10 throughout;
  skip: a (level, component) pair in which some part has no admissible cell in any mixture yields nothing;
  result: the largest root score over the remaining pairs, ties to the smallest (level, component, y, x), back-tracked by the
      oracle's argmin on the masked tables.

SLIPS: the same with one mistake each (tests/test_latent_cpu.py shows that each changes a result)."""
import copy

import numpy as np

NEG = -1e10
SLIPS = ("no_plus1", "ge", "size_mix0", "org_nopad")


def dp_model(model):
    """the model as the oracle's DP stages read it: filters of one size (the DP never reads them; a mixed bank has no uniform desc)"""
    st = copy.copy(model)
    st.filtersw = [np.zeros((5, 5 * model.flen), np.float32) for _ in model.filtersw]
    return st


def window(model, comp, p, m, H, W, scale, pad, dtype, slip=None):
    """x1 [W], y1 [H], sz of the windows of plane (p, m) on an H x W level"""
    T = np.dtype(dtype).type
    s = T(np.float32(scale))
    rows = model.filtersw[model.filterid[comp][p][0 if slip == "size_mix0" else m]].shape[0]
    org = 1 if slip == "org_nopad" else 1 + pad
    sz = int(np.rint(T(rows) * s))
    x1 = np.rint((np.arange(W) - org).astype(dtype) * s).astype(np.int64)
    y1 = np.rint((np.arange(H) - org).astype(dtype) * s).astype(np.int64)
    return x1, y1, sz


def overlap_grid(x1, y1, sz, box, slip=None):
    """[H, W] float64 overlap of every window with box = (tx, ty, tw, th)"""
    one = 0.0 if slip == "no_plus1" else 1.0
    tx, ty, tw, th = (float(v) for v in box)
    x1, y1 = x1.astype(np.float64), y1.astype(np.float64)
    x2, y2 = x1 + float(sz) - 1.0, y1 + float(sz) - 1.0
    w = np.maximum(0.0, np.minimum(x2, tx + tw) - np.maximum(x1, tx) + one)
    h = np.maximum(0.0, np.minimum(y2, ty + th) - np.maximum(y1, ty) + one)
    inter = h[:, None] * w[None, :]
    area = float(sz) * float(sz)
    bx = (tw + 1.0) * (th + 1.0)
    return inter / (area + bx - inter)


def admissible(model, comp, p, m, H, W, scale, pad, dtype, box, overlap, slip=None):
    ov = overlap_grid(*window(model, comp, p, m, H, W, scale, pad, dtype, slip), box, slip)
    return ov >= overlap if slip == "ge" else ov > overlap


def mask_level(model, resp, scale, truth, overlap, mix=None, component=-1, pad=0, slip=None):
    """resp [nf, H, W] -> (masked copy, flags[c][p]: part p of component c has an admissible cell); components that are not searched
    keep their planes and get no flag"""
    out = np.array(resp, copy=True)
    dtype = out.dtype
    _, H, W = out.shape
    flags = [[False] * model.nparts(c) for c in range(model.ncomponents)]
    for c in range(model.ncomponents):
        if component >= 0 and c != component:
            continue
        for p in range(model.nparts(c)):
            forced = -1 if mix is None else int(mix[p])
            for m, f in enumerate(model.filterid[c][p]):
                if forced >= 0 and m != forced:
                    out[f] = NEG
                    continue
                adm = admissible(model, c, p, m, H, W, scale, pad, dtype, truth[p], overlap, slip)
                out[f][~adm] = NEG
                flags[c][p] = flags[c][p] or bool(adm.any())
    return out, flags


def boxes_of(model, comp, locs, scale, pad, dtype):
    """[P, 4] (x, y, width, height) of one configuration: src/DynamicProgram.cpp:238-240 with the origin moved back by the padding"""
    P = model.nparts(comp)
    out = np.zeros((P, 4), np.int32)
    for p in range(P):
        x, y, m = (int(v) for v in locs[p])
        H, W = y + 1, x + 1
        x1, y1, sz = window(model, comp, p, m, H, W, scale, pad, dtype)
        a, b = int(x1[x]), int(y1[y])
        a2, b2 = a + sz - 1, b + sz - 1
        out[p] = (min(a, a2), min(b, b2), max(a, a2) - min(a, a2), max(b, b2) - min(b, b2))
    return out


def detect(orc, model, scales, resp_of_level, truth, overlap, mix=None, component=-1, pad=0, dtype=np.float32, correct_ptr=0,
           slip=None, levels=None):
    """-> dict(found, score (T), component, level, locs [P, 3], boxes [P, 4], admissible [L, C] int32, masked[l] [nf, H, W],
    tables[l][c] = (Ix, Iy, Ik, rootv, rooti) of every pair that was run).  resp_of_level(l) -> [nf, H, W] of type dtype, or None
    for a level without cells."""
    st = dp_model(model)
    st.thresh = -3.0e38
    desc = st.to_desc()
    L = len(scales)
    adm = np.zeros((L, model.ncomponents), np.int32)
    masked, tables = {}, {}
    best = None
    for l in (range(L) if levels is None else levels):
        resp = resp_of_level(l)
        if resp is None or resp.size == 0:
            continue
        resp = np.ascontiguousarray(resp, dtype)
        mk, flags = mask_level(model, resp, scales[l], truth, overlap, mix, component, pad, slip)
        masked[l] = mk
        tables[l] = {}
        for c in range(model.ncomponents):
            t = orc.dp_min_level(desc, c, mk, correct_ptr=correct_ptr, dtype=dtype)
            tables[l][c] = t
            if not all(flags[c]):
                continue
            adm[l, c] = 1
            rv = t[3]
            i = int(np.argmax(rv))                       # the first maximum in row-major order: the smallest (y, x)
            if best is None or rv.flat[i] > best[0]:     # strict: the smallest (level, component) among equals
                best = (rv.flat[i], l, c, i)
    if best is None:
        return dict(found=0, admissible=adm, masked=masked, tables=tables)
    v, l, c, i = best
    Ix, Iy, Ik, rv, ri = tables[l][c]
    H, W = rv.shape
    heads, _, locs = orc.dp_argmin_level(desc, c, l, scales[l], rv, ri, Ix, Iy, Ik, capacity=H * W, dtype=dtype)
    assert len(heads) == H * W                           # every root is above the threshold: record i is the root at cell i
    lc = locs[i][:model.nparts(c)]
    assert (int(lc[0][0]), int(lc[0][1])) == (i % W, i // W)
    return dict(found=1, score=v, component=c, level=l, locs=lc, boxes=boxes_of(model, c, lc, scales[l], pad, dtype),
                admissible=adm, masked=masked, tables=tables)


def truth_at(model, comp, scale, cells, pad=0, dtype=np.float32):
    """truth boxes [max_parts, 4]: the windows of mixture 0 of every part of `comp` at cells[p] = (x, y) of a level of that scale"""
    out = np.zeros((model.max_parts, 4), np.int32)
    locs = [(x, y, 0) for x, y in cells]
    out[:model.nparts(comp)] = boxes_of(model, comp, locs, scale, pad, dtype)
    return out
