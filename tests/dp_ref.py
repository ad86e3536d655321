"""Test helper: the message passing of DynamicProgram<T>::min (src/DynamicProgram.cpp:95-171) for ONE pyramid
level, in numpy on top of the oracle's distance transform (orc.dt2d), keeping every intermediate map — the
accumulated part scores and the distance-transformed child scores that the oracle's C entry point does not
return.  Used to CLASSIFY part-location differences between the MFMA filter bank and the reference-order
filter bank as near-ties: at the first part where two back-tracked configurations diverge, how
far apart were the two alternatives in the reference's own numbers?

Checked against orc.dp_min_level bit for bit (tests/test_oracle_cpu.py::test_dp_ref_matches_oracle).
"""
import numpy as np


def level_maps(orc, model, comp, resp, dtype=np.float32):
    """resp [nf, H, W] -> dict(score_in[p][mm], sdt[p][mm], weighted-argmax inputs, rootv, rooti)."""
    T = np.dtype(dtype).type
    P = model.nparts(comp)
    fid, did, bid, par = model.filterid[comp], model.defid[comp], model.biasid[comp], model.parentid[comp]
    acc = {}                                     # ncscores[filterid] (:93): filled lazily (:155)
    score_in = [None] * P
    sdt = [None] * P
    ix = [None] * P
    iy = [None] * P
    for p in range(P - 1, 0, -1):                # :95
        K = len(fid[p])
        score_in[p], sdt[p], ix[p], iy[p] = [], [], [], []
        for mm in range(K):
            src = acc.get(fid[p][mm], resp[fid[p][mm]])          # :115-119
            w = model.defw[did[p][mm]]
            a = model.anchors[did[p][mm]]
            out, x_, y_ = orc.dt2d(src, -float(w[0]), -float(w[1]), -float(w[2]), -float(w[3]), int(a[0]), int(a[1]),
                                   dtype=dtype)                  # :125-128
            score_in[p].append(np.array(src, dtype))
            sdt[p].append(out); ix[p].append(x_); iy[p].append(y_)
        pp = par[p]
        for m in range(len(fid[pp])):                            # :134-156
            best = None
            for mm in range(K):
                wv = (sdt[p][mm] + T(model.biasw[bid[p][mm] + m])).astype(dtype)
                if K == 1:
                    best = wv
                elif best is None:
                    best = np.where(wv > T(-np.inf), wv, T(-np.inf)).astype(dtype)
                else:
                    best = np.where(wv > best, wv, best)
            f = fid[pp][m]
            base = acc.get(f, resp[f]).astype(dtype)
            acc[f] = (base + best).astype(dtype)
    K0 = len(fid[0])
    bias = T(model.biasw[bid[0][0]])                             # root.bias(0)[0] (:165)
    rv, ri = None, None
    for m in range(K0):
        wv = (acc.get(fid[0][m], resp[fid[0][m]]).astype(dtype) + bias).astype(dtype)
        if K0 == 1:
            rv, ri = wv, np.zeros(wv.shape, np.int32)
        elif rv is None:
            rv, ri = np.where(wv > T(-np.inf), wv, T(-np.inf)).astype(dtype), np.zeros(wv.shape, np.int32)
        else:
            take = wv > rv
            rv, ri = np.where(take, wv, rv), np.where(take, m, ri).astype(np.int32)
    return dict(score_in=score_in, sdt=sdt, ix=ix, iy=iy, rootv=rv, rooti=ri)


def backtrack(model, comp, maps, x, y):
    """argmin (:219-245) for one root location from level_maps' composed pointers -> locs [P, 3]."""
    P = model.nparts(comp)
    fid, bid, par = model.filterid[comp], model.biasid[comp], model.parentid[comp]
    locs = np.zeros((P, 3), np.int32)
    locs[0] = (x, y, maps["rooti"][y, x])
    T = maps["rootv"].dtype.type
    for p in range(1, P):
        px, py, pm = locs[par[p]]
        K = len(fid[p])
        best, bi = None, 0
        for mm in range(K):
            wv = T(maps["sdt"][p][mm][py, px] + T(model.biasw[bid[p][mm] + pm]))
            if best is None or wv > best:
                best, bi = wv, mm
        if K == 1:
            bi = 0
        locs[p] = (maps["ix"][p][bi][py, px], maps["iy"][p][bi][py, px], bi)
    return locs


def _subtree_size(par, p):
    n, P = 0, len(par)
    inside = [False] * P
    inside[p] = True
    for q in range(p, P):
        if q == p or (par[q] >= 0 and inside[par[q]]):
            inside[q] = True
            n += 1
    return n


def divergence_margin(model, comp, maps, locs_ref, locs_got):
    """First part (in index order; parents precede children) whose (x, y, mixture) differs while its parent's
    agree, and the gap between the two alternatives in the REFERENCE's numbers (`maps` from the reference-order
    responses).  The reference picks, at the parent location (px, py) with parent mixture pm:
      mm = argmax_mm sdt[mm](py,px) + bias(mm)[pm]                          (Math::reduceMax, :143)
      x  = argmax_n' in_mm[py, n'] + fx(px + ax - n')                       (x pass, DistanceTransform.hpp:216-218)
      y  = argmax_m' tmp_mm[m', x] + fy(py + ay - m')                       (y pass read at column x, :233-244)
    Returns (part, kind, margin >= 0, subtree size) or None when the configurations are equal."""
    par = model.parentid[comp]
    fid, did, bid = model.filterid[comp], model.defid[comp], model.biasid[comp]
    for p in range(1, model.nparts(comp)):
        if np.array_equal(locs_ref[p], locs_got[p]):
            continue
        if not np.array_equal(locs_ref[par[p]], locs_got[par[p]]):
            continue
        px, py, pm = (int(v) for v in locs_ref[par[p]])
        xo, yo, mo = (int(v) for v in locs_ref[p])
        xg, yg, mg = (int(v) for v in locs_got[p])
        sub = _subtree_size(par, p)
        if mo != mg:
            wo = float(maps["sdt"][p][mo][py, px]) + float(model.biasw[bid[p][mo] + pm])
            wg = float(maps["sdt"][p][mg][py, px]) + float(model.biasw[bid[p][mg] + pm])
            return p, "mixture", abs(wo - wg), sub
        w = model.defw[did[p][mo]].astype(np.float64)
        ax_, ay_ = (int(v) for v in model.anchors[did[p][mo]])
        src = maps["score_in"][p][mo].astype(np.float64)
        H, W = src.shape
        nn = np.arange(W, dtype=np.float64)
        if xo != xg:
            d = px + ax_ - nn
            obj = src[py] - w[0] * d * d - w[1] * d
            return p, "x", abs(float(obj[xo] - obj[xg])), sub
        # same column x: y-pass objective over the x-pass output of column x
        d = (xo + ax_) - nn[None, :]             # x pass at output column xo, every row
        tmp = (src - w[0] * d * d - w[1] * d).max(axis=1)
        mmv = np.arange(H, dtype=np.float64)
        dy = py + ay_ - mmv
        obj = tmp - w[2] * dy * dy - w[3] * dy
        return p, "y", abs(float(obj[yo] - obj[yg])), sub
    return None


def pointer_planes(model, comp, maps):
    """Ix, Iy, Ik [planes, H, W] in the oracle's plane order (plane of (p, m) = sum of the parents' mixture counts of the parts
    1 .. p-1, plus m) from level_maps' intermediates: Ik is the FIRST maximum over the child's K weighted maps for parent
    mixture m (Math::reduceMax: strict >; K == 1: 0), Ix / Iy the chosen mixture's DT pointers (reducePickIndex)."""
    fid, bid, par = model.filterid[comp], model.biasid[comp], model.parentid[comp]
    T = maps["rootv"].dtype.type
    Ix, Iy, Ik = [], [], []
    for p in range(1, model.nparts(comp)):
        K = len(fid[p])
        ix, iy = np.stack(maps["ix"][p]), np.stack(maps["iy"][p])
        for m in range(len(fid[par[p]])):
            wv = np.stack([(maps["sdt"][p][mm] + T(model.biasw[bid[p][mm] + m])).astype(T) for mm in range(K)])
            k = np.zeros(wv.shape[1:], np.int32) if K == 1 else np.argmax(wv, axis=0).astype(np.int32)
            Ik.append(k)
            Ix.append(np.take_along_axis(ix, k[None], 0)[0]); Iy.append(np.take_along_axis(iy, k[None], 0)[0])
    H, W = maps["rootv"].shape
    if not Ik:
        return (np.zeros((0, H, W), np.int32),) * 3
    return np.stack(Ix), np.stack(Iy), np.stack(Ik)


# ---------------------------------------------------------------- the plain statement, and the same with one slip
SLIPS = ("zero_order", "ge", "bias_after_max", "anchor_clamp", "child_count")


def dt_definition(src, ax, bx, ay, by, osx, osy, dtype, clamp=False):
    """DistanceTransform<T>::compute by definition: the x pass out(m, n) = max_n' T(ax d^2 + bx d + src(m, n')), d = n + osx - n' (the
    quadratic evaluated in double as a sq + b d + y, left to right, then narrowed: Quadratic::operator()), the FIRST maximum as pointer; the y
    pass the same down the columns of the x pass's output; Iy composed as the reference does (Iy'(m, n) = Iy(m, Ix(m, n)), :233-244).
    clamp (a slip): the read-out position n + os clamped to the map."""
    def one_pass(a2, a, b, os_):
        R, N = a2.shape
        pos = np.arange(N) + os_
        if clamp:
            pos = np.clip(pos, 0, N - 1)
        d = (pos[:, None] - np.arange(N)[None, :]).astype(np.float64)                   # [n, n']
        with np.errstate(over="ignore"):
            v = ((a * (d * d) + b * d)[None] + a2.astype(np.float64)[:, None, :]).astype(dtype)   # [r, n, n']
        ptr = np.argmax(v, axis=2).astype(np.int32)
        return np.take_along_axis(v, ptr[..., None], 2)[..., 0], ptr
    src = np.ascontiguousarray(src, dtype)
    tmp, ix = one_pass(src, ax, bx, osx)
    outT, iyT = one_pass(np.ascontiguousarray(tmp.T), ay, by, osy)
    out, iy = np.ascontiguousarray(outT.T), np.ascontiguousarray(iyT.T)
    return out, ix, np.take_along_axis(iy, ix, 1)


def _reduce(wvs, how):
    """Math::reduceMax over a list of maps -> (max, index).  how: "gt" the first maximum under `>` (K == 1: a copy); slips: "ge" the last,
    "zero_order" -0.0 ordered below +0.0 (a hardware max, or integer keys)"""
    if len(wvs) == 1:
        return wvs[0], np.zeros(wvs[0].shape, np.int32)
    T = wvs[0].dtype.type
    best, idx = np.where(wvs[0] > T(-np.inf), wvs[0], T(-np.inf)), np.zeros(wvs[0].shape, np.int32)
    for k in range(1, len(wvs)):
        wv = wvs[k]
        take = wv >= best if how == "ge" else wv > best
        if how == "zero_order":
            take = take | ((wv == best) & np.signbit(best) & ~np.signbit(wv))
        best, idx = np.where(take, wv, best), np.where(take, k, idx).astype(np.int32)
    return best, idx


def plain_level(model, comp, resp, dtype=np.float32, orc=None, slip=None):
    """DynamicProgram<T>::min for one level as brute-force max-plus: the distance transform by definition (dt_definition; `orc`: the
    oracle's orc.dt2d instead), the first maximum over the child's mixtures, a deformation row per (part, mixture), any anchor.
    -> Ix, Iy, Ik [planes, H, W] in the oracle's plane order, rootv, rooti.  slip: one of SLIPS, the statement with that one mistake."""
    assert slip is None or slip in SLIPS
    T = np.dtype(dtype).type
    P = model.nparts(comp)
    fid, did, bid, par = model.filterid[comp], model.defid[comp], model.biasid[comp], model.parentid[comp]
    how = slip if slip in ("ge", "zero_order") else "gt"
    acc = {}
    planes = {}
    for p in range(P - 1, 0, -1):
        K, L = len(fid[p]), len(fid[par[p]])
        sdt, ix, iy = [], [], []
        for mm in range(K):
            src = np.asarray(acc.get(fid[p][mm], resp[fid[p][mm]]), dtype)
            w, a = model.defw[did[p][mm]], model.anchors[did[p][mm]]
            q = (-float(w[0]), -float(w[1]), -float(w[2]), -float(w[3]), int(a[0]), int(a[1]))
            o, x_, y_ = orc.dt2d(src, *q, dtype=dtype) if orc is not None and slip != "anchor_clamp" else \
                dt_definition(src, *q, dtype, clamp=slip == "anchor_clamp")
            sdt.append(o); ix.append(x_); iy.append(y_)
        ix, iy = np.stack(ix), np.stack(iy)
        planes[p] = []
        with np.errstate(over="ignore"):
            for m in range(L):
                mb = min(m, K - 1) if slip == "child_count" else m          # the slip: K columns of biases where the parent has L
                if slip == "bias_after_max":
                    best, k = _reduce(sdt, how)
                    best = (best + np.asarray(model.biasw, dtype)[np.asarray(bid[p])[k] + mb]).astype(dtype)
                else:
                    best, k = _reduce([(sdt[mm] + T(model.biasw[bid[p][mm] + mb])).astype(dtype) for mm in range(K)], how)
                planes[p].append((np.take_along_axis(ix, k[None], 0)[0], np.take_along_axis(iy, k[None], 0)[0], k))
                f = fid[par[p]][m]
                acc[f] = (np.asarray(acc.get(f, resp[f]), dtype) + best).astype(dtype)
    bias = T(model.biasw[bid[0][0]])
    with np.errstate(over="ignore"):
        rv, ri = _reduce([(np.asarray(acc.get(f, resp[f]), dtype) + bias).astype(dtype) for f in fid[0]], how)
    flat = [t for p in range(1, P) for t in planes[p]]
    H, W = rv.shape
    if not flat:
        return (np.zeros((0, H, W), np.int32),) * 3 + (rv, ri)
    return tuple(np.stack([t[i] for t in flat]) for i in range(3)) + (rv, ri)


def rescore(model, comp, resp, locs):
    """(score, sum of |terms|) of one configuration locs [P, 3] = (x, y, mixture) in float64: responses at the part locations, the
    deformation cost of every (parent, child) pair and the biases (matlab/detection/detect.m:139-145)"""
    fid, did, bid, par = model.filterid[comp], model.defid[comp], model.biasid[comp], model.parentid[comp]
    terms = [float(model.biasw[bid[0][0]])]
    for p in range(model.nparts(comp)):
        x, y, k = (int(v) for v in locs[p])
        terms.append(float(resp[fid[p][k], y, x]))
        if p > 0:
            px, py, pm = (int(v) for v in locs[par[p]])
            w = np.asarray(model.defw[did[p][k]], np.float64)
            ax_, ay_ = (int(v) for v in model.anchors[did[p][k]])
            dx, dy = px + ax_ - x, py + ay_ - y
            terms += [-w[0] * dx * dx, -w[1] * dx, -w[2] * dy * dy, -w[3] * dy, float(model.biasw[bid[p][k] + pm])]
    import math
    return math.fsum(terms), math.fsum(abs(t) for t in terms)
