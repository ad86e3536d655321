"""numpy restatement of matlab/learning/k_means.m and clusterparts.m, and of the model assembly around them (initmodel.m, data_def.m,
mergemodels.m, buildmodel.m), written from the MATLAB files: the library's own definition is held to this.

k_means: `sums="literal"` adds as the files do (sum / mean: left to right over the rows); `sums="block"` uses the library's block sum
(include/pbd_c.h "part mixtures": element i to partial i mod 64, i ascending, partials from +0.0, folded s[t] += s[t + h], h = 32 .. 1).
The random start (k_means.m:78) and the iteration cap are the header's stated deviations and are restated from the header.  So is the
centroid of a cluster of ONE point: k_means.m:103's mean(X(gIdx==t,:)) of a single 1 x m row runs along the row in MATLAB and spreads
the mean of the point's coordinates over c(t,:); here, as in the header, the mean is per coordinate for any count.  mergemodels below
appends every bias of a model; mergemodels.m:12 indexes model.bias(nb+1) inside its loop over i and so keeps only the last bias of a
model that has several (its callers pass one-bias models, where both agree): the restatement follows the library's stated reading."""
import numpy as np

M64 = (1 << 64) - 1


def splitmix64(state):
    """-> (value, new state): include/pbd_c.h "QP solver" """
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31), state


def stream_start(seed, p, R, r):
    return (seed ^ ((0xD1B54A32D192ED03 * (p * R + r + 1)) & M64)) & M64


def start_rows(n, k, state):
    rows = []
    for _ in range(k):
        v, state = splitmix64(state)
        rows.append(v % n)
    return rows


def _sum_literal(v):
    """left to right (np.cumsum accumulates sequentially)"""
    v = np.asarray(v, np.float64)
    return np.cumsum(v)[-1] if v.size else np.float64(0.0)


def _sum_block(v, index):
    """the block sum of the elements v, which sit at positions `index` (ascending) of the point axis.  The 64 partials advance together,
    one row of 64 positions at a time; a position that holds no element contributes +0.0, which leaves a partial that started at +0.0
    unchanged in every bit — the same as adding nothing."""
    index = np.asarray(index, np.int64)
    rows = (int(index.max()) // 64 + 1) if index.size else 0
    full = np.zeros(rows * 64, np.float64)
    full[index] = v
    part = np.zeros(64, np.float64)
    for row in full.reshape(rows, 64):
        part = part + row
    h = 32
    while h >= 1:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return part[0]


def _min_rows(D):
    """[z, i] = min(D, [], 2): NaN ignored, the first of equal minima; an all-NaN row: (NaN, 0)"""
    n, k = D.shape
    z, idx = D[:, 0].copy(), np.zeros(n, np.int64)
    for t in range(1, k):
        take = (D[:, t] < z) | (np.isnan(z) & ~np.isnan(D[:, t]))
        z[take] = D[take, t]
        idx[take] = t
    return z, idx


def k_means(X, c, sums="literal", max_iter=1000):
    """k_means.m:71-114 with given start centroids c [k, m] -> dict(idx 0-based, c, sumdist, iters, capped)"""
    X = np.asarray(X, np.float64)
    c = np.array(c, np.float64)
    n, m = X.shape
    k = len(c)
    g0, gidx = np.full(n, -2), np.full(n, -1)   # :82-83, ones against zeros
    iters = 0
    with np.errstate(invalid="ignore"):
        while np.any(g0 != gidx) and iters < max_iter:
            g0 = gidx
            D = np.zeros((n, k))
            for t in range(k):
                d = np.zeros(n)
                for s in range(m):
                    d = d + (X[:, s] - c[t, s]) ** 2
                D[:, t] = d
            z, gidx = _min_rows(D)
            for t in range(k):
                sel = np.flatnonzero(gidx == t)
                if len(sel) == 0:
                    c[t, :] = np.nan
                    continue
                for s in range(m):
                    tot = _sum_literal(X[sel, s]) if sums == "literal" else _sum_block(X[sel, s], sel)
                    c[t, s] = tot / np.float64(len(sel))
            iters += 1
    sumdist = _sum_literal(z) if sums == "literal" else _sum_block(z, range(n))
    return dict(idx=gidx.astype(np.int32), c=c, sumdist=float(sumdist), iters=iters, capped=int(np.any(g0 != gidx)))


def k_means_seeded(X, k, state, sums="block", max_iter=1000):
    X = np.asarray(X, np.float64)
    return k_means(X, X[start_rows(len(X), k, state)], sums, max_iter)


def part_points(deffeat, parents, p):
    """clusterparts.m:9-17, 0-based"""
    if parents[p] < 0:
        i = 0
        while parents[i] != p:
            i += 1
        return deffeat[i] - deffeat[p]
    return deffeat[p] - deffeat[parents[p]]


def clusterparts(deffeat, parents, K, R, seed, sums="block", max_iter=1000):
    """clusterparts.m -> dict(idx [P, n], centres (a list of [K[p], 2]), sumdist [P], best_trial [P], trial_sumdist [P, R],
    trial_iters [P, R], capped)"""
    deffeat = np.asarray(deffeat, np.float64)
    P, n = deffeat.shape[:2]
    out = dict(idx=np.zeros((P, n), np.int32), centres=[], sumdist=np.zeros(P), best_trial=np.zeros(P, np.int32),
               trial_sumdist=np.zeros((P, R)), trial_iters=np.zeros((P, R), np.int32), capped=0)
    for p in range(P):
        X = part_points(deffeat, parents, p)
        trials = [k_means_seeded(X, int(K[p]), stream_start(seed, p, R, r), sums, max_iter) for r in range(R)]
        sd = np.array([t["sumdist"] for t in trials])
        best = int(_min_rows(sd[None, :])[1][0])   # [dummy ind] = min(sumdist); ind(1)
        out["idx"][p] = trials[best]["idx"]
        out["centres"].append(trials[best]["c"])
        out["sumdist"][p], out["best_trial"][p] = sd[best], best
        out["trial_sumdist"][p] = sd
        out["trial_iters"][p] = [t["iters"] for t in trials]
        out["capped"] += sum(t["capped"] for t in trials)
    return out


# ---- the model assembly around it, in the MATLAB files' own (1-based, struct) terms ---------------------------------------------------
def initmodel(w, h, sbin, tsize=None):
    """initmodel.m -> dict(tsize, maxsize, len, bias=[(w, i)], filters=[(w, i)], component)"""
    w, h = np.asarray(w, np.float64), np.asarray(h, np.float64)
    if tsize is None:
        areas = np.sort(h * w)
        area = areas[int(np.floor(len(areas) * 0.05)) - 1]
        nw = np.sqrt(area / 1)
        nh = nw * 1
        tsize = (int(np.floor(nh / sbin)), int(np.floor(nw / sbin)), 32)
    return dict(tsize=tuple(tsize), maxsize=tuple(tsize[:2]), len=1 + int(np.prod(tsize)), sbin=sbin, interval=10,
                bias=[(0.0, 1)], filters=[(np.zeros(tsize), 2)], component=dict(biasid=1, defid=[], filterid=1, parent=0))


def data_def(points, w, h, maxsize):
    """data_def.m: points [n, P, 2] -> a list of P arrays [n, 2]"""
    points = np.asarray(points, np.float64)
    w, h = np.asarray(w, np.float64), np.asarray(h, np.float64)
    scale = np.sqrt(w * h) / np.sqrt(np.float64(maxsize[0] * maxsize[1]))
    return [points[:, p, :] / scale[:, None] for p in range(points.shape[1])]


def mergemodels(models):
    """mergemodels.m — every bias appended (nb+i, like :20 and :28; the file's :12 writes nb+1 for each i) — on dicts(len, maxsize, bias=[(w, i)], filters=[(w, i)], defs=[(w, i, anchor)], components=[[part dicts]]), ids 1-based"""
    import copy
    model = copy.deepcopy(models[0])
    for mm in models[1:]:
        nb, nf, nd = len(model["bias"]), len(model["filters"]), len(model["defs"])
        model["bias"] += [(w, i + model["len"]) for w, i in mm["bias"]]
        model["filters"] += [(w, i + model["len"]) for w, i in mm["filters"]]
        model["defs"] += [(w, i + model["len"], a) for w, i, a in mm["defs"]]
        for comp in mm["components"]:
            model["components"].append([dict(biasid=[[b + nb for b in row] for row in x["biasid"]], defid=[d + nd for d in x["defid"]],
                                             filterid=[f + nf for f in x["filterid"]], parent=x["parent"]) for x in comp])
        model["maxsize"] = tuple(np.maximum(model["maxsize"], mm["maxsize"]).tolist())
        model["len"] += mm["len"]
    return model


def matlab_round(v):
    """MATLAB round: half away from zero"""
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def buildmodel(part_filters, deffeat, idx, pa):
    """buildmodel.m:19-80 in its own terms: pa and every id 1-based, idx 1-based labels; part_filters[i][k] the weights model.filters(k).w
    loaded for child i.  -> dict(bias, filters, defs, components, len) like the file's jointmodel"""
    jm = dict(bias=[], filters=[], defs=[], components=[], len=0)
    for i in range(1, len(pa) + 1):
        child, parent = i, pa[i - 1]
        assert parent < child
        p = dict(biasid=[], filterid=[], defid=[], parent=parent)
        if parent == 0:
            jm["bias"].append((0.0, jm["len"] + 1))
            jm["len"] += 1
            p["biasid"] = [[len(jm["bias"])]]
        else:
            Kc, Lp = int(max(idx[child - 1])), int(max(idx[parent - 1]))
            p["biasid"] = [[0] * Kc for _ in range(Lp)]
            for k in range(1, Kc + 1):
                for l in range(1, Lp + 1):
                    jm["bias"].append((0.0, jm["len"] + 1))
                    jm["len"] += 1
                    p["biasid"][l - 1][k - 1] = len(jm["bias"])
        for k in range(1, int(max(idx[child - 1])) + 1):
            fw = part_filters[child - 1][k - 1]
            jm["filters"].append((fw, jm["len"] + 1))
            jm["len"] += fw.size
            p["filterid"].append(len(jm["filters"]))
        if parent > 0:
            for k in range(1, int(max(idx[child - 1])) + 1):
                sel = np.asarray(idx[child - 1]) == k
                with np.errstate(invalid="ignore"):
                    x = _sum_literal(deffeat[child - 1][sel, 0] - deffeat[parent - 1][sel, 0]) / np.float64(sel.sum())
                    y = _sum_literal(deffeat[child - 1][sel, 1] - deffeat[parent - 1][sel, 1]) / np.float64(sel.sum())
                anchor = matlab_round(np.array([x + 1, y + 1, 0.0]))
                jm["defs"].append((np.array([0.01, 0, 0.01, 0]), jm["len"] + 1, anchor))
                jm["len"] += 4
                p["defid"].append(len(jm["defs"]))
        jm["components"].append(p)
    return jm
