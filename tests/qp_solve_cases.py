"""Synthetic caches with solver state for the QP solver's tests (include/pbd_c.h "QP solver"): the inputs of
tests/golden/make_ref_qp_one.py (which records what the compiled matlab/mex/qp_one_sparse.cc makes of them), of
tests/test_qp_solve_cpu.py and of tests/test_gpu_qp_solve.py.  Everything comes from seeds; nothing here runs a pass.

A case: dict(x [n, K] float32, ids [n, 5] int32, b [n] float32, d [n] float64, a [n] float64, w [LEN] float64, l, noneg int32,
passes, seed).  Columns are in pbd_qp_put's format, K wide over LEN dense elements (tests/qp_cases.py), every column's blocks
ascending, so that the reference file's merge walk is complete on them.  Examples come in id groups of 4.

Two value scalings: "free", where the per-id constraint sum(a) <= 1 never binds, and "binding", where it does and the pair branch
runs.  The binding case starts from multipliers that violate the constraints slightly in places, which is what the file's clamps
(:178-179) and the clip against A[i2] - C are for.

LARGE_CASES hold two more of the binding kind at the sizes of a real cache: "manyblock", 48 columns of 77 blocks (a pose of the person
model), and "manyids", 2400 examples of 1200 ids under a noneg list of 1600 entries (tests/golden/ref_qp_one_v2.npz)."""
import math

import numpy as np

from tests.qp_cases import K, LEN, column
from tests.qp_ref import lincomb_ref

F64 = np.float64
GROUP = 4


def _blocks(rng, kind):
    """ascending blocks of one example: lengths 1, 4, 63 / 64 / 65, a few hundred, and now and then one above 4096, at offsets that
    make the blocks of different examples intersect partially"""
    if kind == "none":
        return []
    out = [(int(rng.integers(0, 10)), 1)]
    if kind == "one":
        return out
    full = kind in ("full", "long")
    if rng.random() < .7 or full:
        out.append((16 + 4 * int(rng.integers(0, 8)), 4))
    if rng.random() < .8 or full:
        out.append((100 + int(rng.integers(0, 200)), int(rng.choice([63, 64, 65]))))
    if rng.random() < .8 or full:
        out.append((500 + int(rng.integers(0, 100)), int(rng.choice([129, 300, 800]))))
    if kind == "long" or rng.random() < .06:
        out.append((1500 + int(rng.integers(0, 300)), 4100))
    return out


def _norms(x):
    """x'x of the stored values, correctly rounded (an input: any nearby value serves)"""
    d = np.zeros(len(x), F64)
    for i, col in enumerate(x):
        xp, tot = 1, []
        for _ in range(int(col[0])):
            s, e = int(col[xp]), int(col[xp + 1])
            tot.extend(float(v) * float(v) for v in col[xp + 2:xp + 2 + e - s + 1])
            xp += 2 + e - s + 1
        d[i] = math.fsum(tot)
    return d


def _refreshed(x, b, a, noneg):
    """w and l as qp_refresh.m makes them of a (so a cache brought to a by set_state and refresh holds exactly this): the examples
    with a > 0 sorted by a, stable (none: example 0), each product rounded, added in that order; then the noneg clamp"""
    I = np.flatnonzero(a > 0)
    I = I[np.argsort(a[I], kind="stable")] if len(I) else np.array([0])
    w = lincomb_ref(x, a, I, LEN)
    l = F64(0.0)
    for i in I:
        l = l + F64(b[i]) * a[i]
    w[noneg] = np.where(w[noneg] < 0.0, 0.0, w[noneg])
    return w, l


def make_case(seed, n_ex, scale, passes, violate):
    """violate: also an example without blocks (d = 0: the file divides by it), one with a single value, and starting multipliers"""
    rng = np.random.default_rng(seed)
    kinds = ["any" if violate else "full"] * n_ex     # "full": every example has a few hundred values, so no a comes near 1
    kinds[14] = "long"
    if violate:
        kinds[5], kinds[9] = "none", "one"
    x = np.stack([column(rng, _blocks(rng, kind), lambda n: (scale * rng.normal(.3, 1.0, n)).astype(np.float32)) for kind in kinds])
    assert x.shape == (n_ex, K)
    ids = np.zeros((n_ex, 5), np.int32)
    for i in range(n_ex):
        g = i // GROUP
        # words beyond one byte, so that memcmp order and numeric order differ
        ids[i] = (1 if g % 3 else -1, 250 + 7 * g, g % 5, 3 * g, 1000 - g)
    perm = rng.permutation(n_ex)                      # groups are not contiguous in the cache
    x, ids = x[perm], ids[perm]
    b = (.6 * rng.uniform(.5, 1.5, n_ex)).astype(np.float32)
    d = _norms(x)
    a = np.zeros(n_ex, F64)
    if violate:
        for g in range(0, n_ex // GROUP, 3):          # every third id starts with multipliers, some summing above 1
            m = np.flatnonzero((ids[:, 1] == 250 + 7 * g))
            a[m[0]], a[m[1]] = .7, (.5 if g % 2 else .3)
    noneg = np.unique(np.concatenate([rng.integers(500, 1400, 40), rng.integers(16, 48, 6), rng.integers(100, 460, 20)])).astype(np.int32)
    w, l = _refreshed(x, b, a, noneg)
    return dict(x=x, ids=ids, b=b, d=d, a=a, w=w, l=l, noneg=noneg, passes=passes, seed=seed)


PARTS = 26          # a pose of the person model: 3 * 26 - 1 = 77 blocks
REGION = 340        # dense elements a "part" of the manyblock case owns: 26 * 340 <= LEN


def _pose_blocks(rng):
    """77 ascending blocks: per part a 1-element block, for parts > 0 a 4-element block, and a window of 63 / 64 / 65 / 70 elements at
    an offset of its own, so that the windows of different examples intersect partially"""
    out = []
    for p in range(PARTS):
        base = p * REGION
        out.append((base + int(rng.integers(0, 4)), 1))
        if p > 0:
            out.append((base + 8 + 4 * int(rng.integers(0, 4)), 4))
        out.append((base + 30 + int(rng.integers(0, 200)), int(rng.choice([63, 64, 65, 70]))))
    return out


def _two_blocks(rng):
    """a 1-element block and a block of 3 .. 39 elements inside the first 3000 dense elements"""
    return [(int(rng.integers(0, 40)), 1), (60 + int(rng.integers(0, 2900)), int(rng.integers(3, 40)))]


def make_large_case(seed, n_ex, group, blocks, scale, passes, n_noneg, lo, hi):
    """a case like make_case's with violate, of n_ex examples in id groups of `group`, every column blocks(rng); noneg: n_noneg
    distinct dense indices of [lo, hi)"""
    rng = np.random.default_rng(seed)
    x = np.stack([column(rng, blocks(rng), lambda n: (scale * rng.normal(.3, 1.0, n)).astype(np.float32)) for _ in range(n_ex)])
    ids = np.zeros((n_ex, 5), np.int32)
    for i in range(n_ex):
        g = i // group
        ids[i] = (1 if g % 3 else -1, 250 + 7 * g, g % 5, 3 * g, 1000 - g)
    perm = rng.permutation(n_ex)
    x, ids = x[perm], ids[perm]
    b = (.6 * rng.uniform(.5, 1.5, n_ex)).astype(np.float32)
    d = _norms(x)
    a = np.zeros(n_ex, F64)
    for g in range(0, n_ex // group, 3):              # every third id starts with multipliers, some summing above 1
        m = np.flatnonzero((ids[:, 1] == 250 + 7 * g))
        a[m[0]], a[m[1]] = .7, (.5 if g % 2 else .3)
    noneg = np.sort(rng.choice(np.arange(lo, hi), n_noneg, replace=False)).astype(np.int32)
    w, l = _refreshed(x, b, a, noneg)
    return dict(x=x, ids=ids, b=b, d=d, a=a, w=w, l=l, noneg=noneg, passes=passes, seed=seed)


CASES = {
    "free": lambda: make_case(301, 72, .3, 4, False),
    "binding": lambda: make_case(302, 100, .03, 6, True),
}

# beyond one trip of the pass kernel's loops (k_qp_solve.hip: 16 wavefronts over a column's blocks, the loss in chunks of 1024 ids, the
# clamp in strides of the block size): columns of 77 blocks; 1200 ids under a noneg list of 1600 entries
LARGE_CASES = {
    "manyblock": lambda: make_large_case(303, 48, 4, _pose_blocks, .01, 4, 400, 0, PARTS * REGION),
    "manyids": lambda: make_large_case(304, 2400, 2, _two_blocks, .2, 2, 1600, 0, 3000),
}


def next_order(case, p, sv):
    """the order of pass p: a permutation of find(sv), on odd passes of a subset of it"""
    rng = np.random.default_rng(1000 * case["seed"] + p)
    I = np.flatnonzero(np.asarray(sv)[:len(case["x"])])
    if p % 2 == 1:
        I = I[rng.random(len(I)) < .7]
    return rng.permutation(I).astype(np.int32)


def nonascending_pair(seed=7):
    """two columns in detect.m's block order (bias, window, bias, def, window): not ascending in the dense layout"""
    rng = np.random.default_rng(seed)

    def vals(n):
        return rng.normal(.3, 1.0, n).astype(np.float32)
    x1 = column(rng, [(3, 1), (2000, 800), (5, 1), (40, 4), (3000, 800)], vals)
    x2 = column(rng, [(3, 1), (2400, 500), (5, 1), (40, 4), (2900, 640)], vals)
    return x1, x2


def dense(col):
    out = np.zeros(LEN, F64)
    xp = 1
    for _ in range(int(col[0])):
        s, e = int(col[xp]) - 1, int(col[xp + 1])
        out[s:e] = col[xp + 2:xp + 2 + e - s]
        xp += 2 + e - s
    return out
