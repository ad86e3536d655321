"""The training example cache (include/pbd_c.h "training example cache") restated in numpy: the write (column format,
standardisation, d and b in the library's stated order, ids), score (matlab/mex/score.cc), lincomb (matlab/mex/lincomb.cc) and keep
(matlab/learning/qp_prune.m:18-25).  Every double operation is one IEEE operation in the stated order: numpy's elementwise * and /
round once, np.add.accumulate adds strictly left to right."""
import numpy as np

F64 = np.float64
FLEN = 32


def seq_sum(terms, start=0.0):
    """start + t0 + t1 + ... strictly in that order"""
    return float(np.add.accumulate(np.concatenate([[start], np.asarray(terms, F64)]))[-1])


def block_sum(terms):
    """the library's sum of a block's terms: 64 partial sums — partial t starts at +0.0 and adds terms t, t + 64, ... in that order —
    folded s[t] += s[t + h] for h = 32, 16, .. 1"""
    terms = np.asarray(terms, F64)
    rows = -(-len(terms) // 64)
    t = np.zeros((rows + 1, 64), F64)             # row 0: the partials' +0.0 start; a partial that starts at +0.0 is never -0.0, so the
    t.ravel()[64:64 + len(terms)] = terms         # +0.0 padding of the last row changes no bit
    s = np.add.accumulate(t, axis=0)[-1]
    h = 32
    while h >= 1:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return float(s[0])


def sparselen(model):
    """k: 1 + 2 * blocks + values of a pose, the largest component, a part at its largest mixture's filter (train.m:207-239)"""
    sizes = model.filter_sizes()
    k = 1
    for c in range(model.ncomponents):
        np_ = model.nparts(c)
        kc = 1 + 2 * (3 * np_ - 1)
        for p in range(np_):
            kc += 1 + (4 if p > 0 else 0) + max(int(sizes[f, 0] * sizes[f, 1]) * model.flen for f in model.filterid[c][p])
        k = max(k, kc)
    return k


def example_blocks(model, blocks, windows):
    """one record's blocks in detect.m:272-308's order: [(0-based dense start, float64 values)] from its pbd_feature_block row and
    its windows [max_parts, wmax] — root: bias, window; every later part: bias, deformation, window"""
    lay = model.feature_layout()
    out = []
    for p in range(len(blocks)):
        b = blocks[p]
        if b["bias_id"] < 0:
            continue
        out.append((lay["bias"] + int(b["bias_id"]), np.ones(1, F64)))
        if p > 0:
            out.append((lay["deform"] + 4 * int(b["def_id"]), np.asarray(b["def"], F64)))
        n = int(b["kh"]) * int(b["kw"]) * model.flen
        out.append((int(lay["filters"][int(b["filter_id"])]), np.asarray(windows[p][:n]).astype(F64)))
    return out


def write_ref(model, heads, locs, blocks, windows, label, id, cpos, cneg, wreg, w0, k):
    """qp_write.m:49-72 of every record -> (x [n, k] float32, ids [n, 5] int32, b [n] float32, d [n] float64)"""
    n = len(heads)
    x, ids = np.zeros((n, k), np.float32), np.zeros((n, 5), np.int32)
    b, d = np.zeros(n, np.float32), np.zeros(n, F64)
    C = F64(cpos if label > 0 else cneg)
    locs = np.asarray(locs).reshape(n, -1, 3)
    for i in range(n):
        bl = example_blocks(model, blocks[i], windows[i])
        starts = sorted(s for s, _ in bl)
        assert all(s0 != s1 for s0, s1 in zip(starts, starts[1:])), "qp_write.m:34-35: a block index repeats"
        x[i, 0] = len(bl)
        xp, norm, bias = 1, 0.0, 1.0
        for s, v in bl:
            if label <= 0:
                v = -v
            xs = (C * v) / wreg[s:s + len(v)]
            x[i, xp], x[i, xp + 1] = s + 1, s + len(v)
            x[i, xp + 2:xp + 2 + len(v)] = xs.astype(np.float32)
            norm = norm + block_sum(xs * xs)
            bias = bias - block_sum(w0[s:s + len(v)] * v)
            xp += 2 + len(v)
        d[i] = norm
        b[i] = np.float32(C * F64(bias))
        ids[i] = (label, id, heads["level"][i], locs[i, 0, 0], locs[i, 0, 1])
    return x, ids, b, d


def parse(col):
    out, xp = [], 1
    for _ in range(int(col[0])):
        s = int(col[xp]) - 1
        n = int(col[xp + 1]) - s
        out.append((s, n, xp + 2))
        xp += 2 + n
    return out


def score_ref(x, w, inds, summation="sequential"):
    """score.cc: y = sum over the blocks, in storage order, of w[j] * (double)x — each product rounded, added left to right.
    summation = "pairwise" / "strided": the same products summed as a tree / as 64 lane-strided partials (what the fixture must tell
    from the sequential sum)"""
    w = np.asarray(w, F64)
    out = np.zeros(len(inds), F64)
    for o, i in enumerate(inds):
        col = x[int(i)]
        prods = [w[s:s + n] * col[xo:xo + n].astype(F64) for s, n, xo in parse(col)]
        p = np.concatenate(prods) if prods else np.zeros(0, F64)
        if summation == "sequential":
            out[o] = seq_sum(p)
        elif summation == "strided":
            out[o] = block_sum(p)
        else:
            out[o] = pairwise(p)
    return out


def pairwise(p):
    p = np.asarray(p, F64)
    if len(p) == 0:
        return 0.0
    while len(p) > 1:
        if len(p) % 2:
            p = np.concatenate([p, [0.0]])
        p = p[0::2] + p[1::2]
    return float(p[0])


def lincomb_ref(x, a, inds, length, summation="sequential"):
    """lincomb.cc: w = 0; for i in inds, in order: w[j] += a[i] * (double)x — each product rounded.  "pairwise": per element the same
    products summed as a tree over the examples"""
    w = np.zeros(length, F64)
    if summation == "sequential":
        for i in inds:
            col = x[int(i)]
            for s, n, xo in parse(col):
                w[s:s + n] = w[s:s + n] + F64(a[int(i)]) * col[xo:xo + n].astype(F64)
        return w
    terms = [[] for _ in range(length)]
    for i in inds:
        col = x[int(i)]
        for s, n, xo in parse(col):
            p = F64(a[int(i)]) * col[xo:xo + n].astype(F64)
            for j in range(n):
                terms[s + j].append(p[j])
    return np.array([pairwise(t) for t in terms], F64)


def keep_ref(cache, inds):
    """qp_prune.m:18-25: (x, ids, b, d) of the kept examples, in order"""
    inds = np.asarray(inds, np.int64)
    return tuple(v[inds] for v in cache)
