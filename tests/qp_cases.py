"""Synthetic example caches in the column format of the training example cache (include/pbd_c.h; qp.x of matlab/learning/qp_write.m),
with weight vectors, multipliers and index lists: the inputs of tests/golden/make_ref_qp.py (which records what the compiled
matlab/mex/score.cc and lincomb.cc make of them), of tests/test_qp_cpu.py and of tests/test_gpu_qp.py.  Everything comes from seeds;
nothing here computes a score.

A case: dict(x [n, K] float32 columns, w [LEN] float64, a [n] float64, inds: {name: int32 index list}).  The columns are K wide and
address a dense space of LEN elements; a cache with a larger k / len takes them zero-padded (the tail of a column is zero anyway)."""
import numpy as np

LEN = 9000    # dense elements the cases address
K = 7000      # column length


def decades(rng, n, lo=-6.0, hi=6.0):
    """n values spanning about 12 decades, both signs"""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n)


def column(rng, blocks, values):
    """blocks: [(0-based dense start, length)], values(length) -> the block's float32 values"""
    x = np.zeros(K, np.float32)
    x[0] = len(blocks)
    xp = 1
    for s, n in blocks:
        assert s >= 0 and s + n <= LEN and xp + 2 + n <= K
        x[xp], x[xp + 1] = s + 1, s + n          # 1-based inclusive bounds
        x[xp + 2:xp + 2 + n] = values(n)
        xp += 2 + n
    return x


def disjoint_blocks(rng, lengths):
    """blocks of the given lengths at random non-overlapping places, in random (not ascending) order"""
    gaps = rng.multinomial(LEN - sum(lengths), np.ones(len(lengths) + 1) / (len(lengths) + 1))
    order = rng.permutation(len(lengths))
    starts, pos = {}, 0
    for slot, j in enumerate(order):
        pos += int(gaps[slot])
        starts[j] = pos
        pos += lengths[j]
    return [(starts[j], lengths[j]) for j in range(len(lengths))]


def case_mixed(seed=101):
    """lengths that are no multiple of 64, one above 4096, a one-block example of length 1, an example without blocks"""
    rng = np.random.default_rng(seed)
    w = decades(rng, LEN)
    plans = [[1], [63, 65, 1, 100], [4100, 130, 7], [64, 64, 191], [], [5, 4, 800, 1, 4, 450, 1, 4, 1250], [2500, 129], [33]]
    x = []
    for lengths in plans:
        blocks = disjoint_blocks(rng, lengths)

        def values(n, blocks=blocks):
            return decades(rng, n, -3.0, 3.0).astype(np.float32)
        x.append(column(rng, blocks, values))
    x = np.stack(x)
    # cancellation: example 2's long block is rewritten so that consecutive products nearly cancel under w
    xp = 3
    s = int(x[2, 1]) - 1
    n = int(x[2, 2]) - s
    v = x[2, xp:xp + n].astype(np.float64)
    v[1::2] = -(v[0::2][:len(v[1::2])] * w[s:s + n:2][:len(v[1::2])]) / w[s + 1:s + n:2]
    x[2, xp:xp + n] = v.astype(np.float32)
    n_ex = len(x)
    a = rng.normal(0.0, 1.0, n_ex) * 10.0 ** rng.uniform(-4, 4, n_ex)
    a[[1, 4]] = 0.0
    a[[0, 5]] = -np.abs(a[[0, 5]])
    inds = dict(all=np.arange(n_ex), empty=np.zeros(0, np.int64), unsorted=np.array([5, 2, 7, 0, 2, 6, 3, 1, 2, 5, 4]),
                one=np.array([0]), reversed=np.arange(n_ex)[::-1])
    return dict(x=x, w=w, a=a, inds={k_: v_.astype(np.int32) for k_, v_ in inds.items()})


def case_overlap(seed=202, n_ex=70):
    """more examples than a wavefront, every example's blocks inside one shared region, so that lincomb adds many examples into the
    same dense elements with cancellation: example 2j+1 is nearly the negative of example 2j"""
    rng = np.random.default_rng(seed)
    w = decades(rng, LEN)
    x = []
    for i in range(n_ex):
        if i % 2 == 0:
            lengths = [int(rng.integers(1, 300)), int(rng.integers(1, 300)), 257]
            blocks = [(100, lengths[0]), (1000 + int(rng.integers(0, 50)), lengths[1]), (3000, 257)]
            vals = [decades(rng, n, -4.0, 4.0).astype(np.float32) for _, n in blocks]
        else:   # the same blocks, values negated and perturbed in the last bits
            vals = [(-v * np.float32(1 + 2.0 ** -20 * rng.integers(-3, 4))).astype(np.float32) for v in vals]
        it = iter(vals)
        x.append(column(rng, blocks, lambda n: next(it)))
    x = np.stack(x)
    a = np.ones(n_ex) + rng.normal(0.0, 1e-6, n_ex)
    a[rng.integers(0, n_ex, 5)] = 0.0
    a[rng.integers(0, n_ex, 5)] *= -1.0
    inds = dict(all=np.arange(n_ex), unsorted=rng.integers(0, n_ex, 100), sorted_by_a=np.argsort(a, kind="stable"))
    return dict(x=x, w=w, a=a, inds={k_: v_.astype(np.int32) for k_, v_ in inds.items()})


CASES = {"mixed": case_mixed, "overlap": case_overlap}


def parse(col):
    """[(0-based start, length, offset of the values in the column)] of one column"""
    out, xp = [], 1
    for _ in range(int(col[0])):
        s = int(col[xp]) - 1
        n = int(col[xp + 1]) - s
        out.append((s, n, xp + 2))
        xp += 2 + n
    return out
