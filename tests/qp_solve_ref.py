"""The QP solver (include/pbd_c.h "QP solver") restated in numpy: matlab/mex/qp_one_sparse.cc's pass, qp_refresh.m, qp_one.m,
qp_opt.m with its loss, qp_prune.m and qp_w.m over a cache (x, ids, b, d) in the column format of tests/qp_ref.py.

Two summation orders and two dots:
  summation = "sequential": every sum strictly left to right, as the compiled reference file adds;
  summation = "strided":    the library's — a block's terms through the block sum (64 lane-strided partials, folded), the blocks' sums
                            added in block order;
  dot = "merge":    the reference file's merge walk over the two columns' blocks (complete only when both are ascending);
  dot = "complete": every pair of blocks, x's outer and x2's inner.
sequential / merge is the compiled file bit for bit (tests/golden/ref_qp_one_v1.npz); strided / complete is the library bit for bit.
Every scalar is a numpy float64, so each operation is one IEEE operation and a division by zero is the hardware's."""
import numpy as np

from tests import qp_ref
from tests.qp_ref import block_sum, parse, seq_sum

F64 = np.float64
ZERO, ONE = F64(0.0), F64(1.0)
EPS = F64(1e-12)
MASK = (1 << 64) - 1


def MAX(A, B):
    return B if A < B else A


def MIN(A, B):
    return B if A > B else A


class State:
    """the solver's state as the library holds it; a and sv by example over the capacity"""

    def __init__(self, capacity, length, n=0, noneg=(), nfix=0):
        self.a, self.sv, self.w = np.zeros(capacity, F64), np.zeros(capacity, np.uint8), np.zeros(length, F64)
        self.sv[:n] = 1
        self.l = self.lb = self.lb_old = self.ub = ZERO
        self.ww = ZERO
        self.noneg, self.nfix = np.asarray(noneg, np.int64), nfix

    def stats(self):
        return np.array([self.l, self.lb, self.lb_old, self.ub], F64)

    def copy(self):
        s = State(len(self.a), len(self.w), 0, self.noneg, self.nfix)
        s.a, s.sv, s.w = self.a.copy(), self.sv.copy(), self.w.copy()
        s.l, s.lb, s.lb_old, s.ub, s.ww = self.l, self.lb, self.lb_old, self.ub, self.ww
        return s


def new_counters():
    return dict(pair=0, clip_C_minus_Ai=0, clip_Ai2=0, clip_minus_Ai=0, clip_Ai2_minus_C=0, sv_clear=0, pg_zero=0, clamp=0, err=0,
                single=0, err_past_1024=0)      # (err_past_1024: non-zero entries of a pass's err at indices >= 1024)


def score(W, col, summation):
    y = ZERO
    for s, n, xo in parse(col):
        p = W[s:s + n] * col[xo:xo + n].astype(F64)
        y = F64(seq_sum(p, y)) if summation == "sequential" else y + F64(block_sum(p))
    return y


def _sum_into(res, p, summation, collect=None):
    if collect is not None:
        collect.extend(p.tolist())                 # (the products themselves, for an exact sum by the caller)
    return F64(seq_sum(p, res)) if summation == "sequential" else res + F64(block_sum(p))


def dot_merge(x, y, summation="sequential", collect=None):
    """qp_one_sparse.cc:31-73, its indices as they are (1-based bounds; a column without blocks reads its zero tail)"""
    res = ZERO
    xnum, ynum = int(x[0]), int(y[0])
    yb = xb = 0
    yi = xi = 1
    yj1, yj2 = int(y[yi]), int(y[yi + 1])
    yi += 2
    xj1, xj2 = int(x[xi]), int(x[xi + 1])
    xi += 2
    while True:
        if xj2 >= yj1 and yj2 >= xj1:
            j1, j2 = max(xj1, yj1), min(xj2, yj2)
            xp, yp, cnt = xi + j1 - xj1, yi + j1 - yj1, j2 - j1 + 1
            res = _sum_into(res, x[xp:xp + cnt].astype(F64) * y[yp:yp + cnt].astype(F64), summation, collect)
        if yj2 <= xj2:
            yb += 1
            if yb >= ynum:
                break
            yi += yj2 - yj1 + 1
            yj1, yj2 = int(y[yi]), int(y[yi + 1])
            yi += 2
        else:
            xb += 1
            if xb >= xnum:
                break
            xi += xj2 - xj1 + 1
            xj1, xj2 = int(x[xi]), int(x[xi + 1])
            xi += 2
    return res


def dot_complete(x, y, summation="strided", collect=None):
    """every block of x in order, every block of y in order: a non-empty intersection's products summed and added to the result"""
    res = ZERO
    by = parse(y)
    for s, n, xo in parse(x):
        for s2, n2, xo2 in by:
            j1, j2 = max(s, s2), min(s + n, s2 + n2)
            if j1 < j2:
                p = x[xo + j1 - s:xo + j2 - s].astype(F64) * y[xo2 + j1 - s2:xo2 + j2 - s2].astype(F64)
                res = _sum_into(res, p, summation, collect)
    return res


def add(W, col, a):
    """add(W, x, a): per element one rounded product and one rounded sum; blocks in storage order"""
    for s, n, xo in parse(col):
        W[s:s + n] = W[s:s + n] + a * col[xo:xo + n].astype(F64)


def clamp(st, cnt=None):
    if len(st.noneg) == 0:
        return
    old = st.w[st.noneg]
    new = np.where(old < 0.0, 0.0, old)            # MAX(W, 0): (W < 0) ? 0 : W — keeps -0.0 and NaN
    if cnt is not None and new.tobytes() != old.tobytes():
        cnt["clamp"] += 1
    st.w[st.noneg] = new


def sum_alpha(ids, a, order):
    """sumAlpha (:90-124): groups in memcmp order of the id's bytes, ties in the order of `order`"""
    n = len(order)
    keys = [ids[int(i)].tobytes() for i in order]
    srt = sorted(range(n), key=lambda t: keys[t])
    idC, idP, idI = np.zeros(n, F64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    num, t0 = 0, srt[0]
    for j in srt:
        i1 = int(order[j])
        if keys[j] != keys[t0]:
            num += 1
        idP[j] = num + 1
        idC[num] = idC[num] + a[i1]
        t0 = j
        if a[i1] > 0:
            idI[num] = i1 + 1
    return idC, idP, idI


def pass_ref(cache, st, order, summation="strided", dot="complete", cnt=None):
    """qp_one_sparse.cc:161-260 with C = 1; st.a, st.sv, st.w and st.l change in place; returns the loss"""
    x, ids, b, d = cache
    cnt = new_counters() if cnt is None else cnt
    order = np.asarray(order, np.int64)
    n = len(order)
    if n == 0:
        return ZERO
    C = ONE
    A, W, SV = st.a, st.w, st.sv
    L = F64(st.l)
    dotf = dot_merge if dot == "merge" else dot_complete
    err = np.zeros(n, F64)
    idC, idP, idI = sum_alpha(ids, A, order)
    with np.errstate(all="ignore"):
        for c in range(n):
            i, j = int(order[c]), int(idP[c]) - 1
            col = x[i]
            A[i] = MAX(MIN(A[i], C), ZERO)
            Ci = MAX(MIN(idC[j], C), A[i])
            G = score(W, col, summation) - F64(b[i])
            PG = G
            if (A[i] == 0 and G >= 0) or (Ci >= C and G <= 0):
                PG = ZERO
                cnt["pg_zero"] += 1
            if -G > err[j]:
                err[j] = -G
                cnt["err"] += 1
            if A[i] == 0 and G > 0:
                SV[i] = 0
                cnt["sv_clear"] += 1
            if Ci >= C and G < -EPS and A[i] < C and idI[j] - 1 != i and idI[j] > 0:
                i2 = int(idI[j]) - 1
                col2 = x[i2]
                cnt["pair"] += 1
                G = G - (score(W, col2, summation) - F64(b[i2]))
                if A[i] == 0 and G > 0:
                    G = ZERO
                    SV[i] = 0
                    cnt["sv_clear"] += 1
                if G > EPS or G < -EPS:
                    dA = -G / (d[i] + d[i2] - F64(2.0) * dotf(col, col2, summation))
                    if dA > 0:
                        t = MIN(dA, C - A[i])
                        cnt["clip_C_minus_Ai"] += int(dA > C - A[i])
                        cnt["clip_Ai2"] += int(t > A[i2])
                        dA = MIN(t, A[i2])
                    else:
                        t = MAX(dA, -A[i])
                        cnt["clip_minus_Ai"] += int(dA < -A[i])
                        cnt["clip_Ai2_minus_C"] += int(t < A[i2] - C)
                        dA = MAX(t, A[i2] - C)
                    A[i] = A[i] + dA
                    A[i2] = A[i2] - dA
                    L = L + dA * (F64(b[i]) - F64(b[i2]))
                    add(W, col, dA)
                    add(W, col2, -dA)
                    clamp(st, cnt)
            elif PG > EPS or PG < -EPS:
                cnt["single"] += 1
                dA = A[i]
                maxA = C - (Ci - dA)
                A[i] = MIN(MAX(A[i] - G / d[i], ZERO), maxA)
                dA = A[i] - dA
                L = L + dA * F64(b[i])
                idC[j] = MIN(MAX(Ci + dA, ZERO), C)
                add(W, col, dA)
                clamp(st, cnt)
            if A[i] > 0:
                idI[j] = i + 1
    st.l = L
    cnt["err_past_1024"] += int(np.count_nonzero(err[1024:]))
    return F64(seq_sum(err))


def wnorm(w, summation):
    return F64(seq_sum(w * w)) if summation == "sequential" else F64(block_sum(w * w))


def refresh_ref(cache, st, summation="strided"):
    """qp_refresh.m; the lincomb is lincomb.cc's in both orders (the library's kernel has the reference's bits)"""
    x, ids, b, d = cache
    I = np.flatnonzero(st.a > 0)
    if len(I) == 0:
        I = np.array([0])
    I = I[np.argsort(st.a[I], kind="stable")]
    l = ZERO
    for i in I:
        l = l + F64(b[i]) * st.a[i]
    st.l = l
    st.w = qp_ref.lincomb_ref(x, st.a, I, len(st.w))
    clamp(st)
    st.ww = wnorm(st.w, summation)
    st.lb_old = st.lb
    st.lb = st.l - st.ww * F64(.5)


def one_ref(cache, st, order, summation="strided", dot="complete", cnt=None):
    loss = pass_ref(cache, st, order, summation, dot, cnt)
    refresh_ref(cache, st, summation)
    st.sv[:st.nfix] = 1
    st.lb_old = st.lb
    st.lb = st.l - st.ww * F64(.5)
    st.ub = st.ww * F64(.5) + loss


def loss_ref(cache, st, n):
    """computeloss (qp_opt.m:56-86) over examples 0 .. n - 1; slack in double"""
    x, ids, b, d = cache
    sc = qp_ref.score_ref(x, st.w, np.arange(n))
    J = np.lexsort(ids[:n].T[::-1])                 # sortrows: ascending numeric lexicographic, stable
    loss, v, pending = ZERO, ZERO, False
    for t, i in enumerate(J):
        slack = F64(b[i]) - sc[i]
        if t == 0 or (ids[i] != ids[J[t - 1]]).any():
            if pending:
                loss = loss + v
            v = slack
            pending = bool(v > 0)
            if not pending:
                v = ZERO
        elif slack > v:
            v, pending = slack, True
    if pending:
        loss = loss + v
    return loss


def splitmix64(seed):
    state = [seed & MASK]

    def nxt():
        state[0] = (state[0] + 0x9E3779B97F4A7C15) & MASK
        z = state[0]
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        return z ^ (z >> 31)
    return nxt


def shuffle(v, nxt):
    """Fisher-Yates as the header states it"""
    v = list(v)
    for t in range(len(v) - 1, 0, -1):
        j = nxt() % (t + 1)
        v[t], v[j] = v[j], v[t]
    return np.asarray(v, np.int32)


def opt_ref(cache, st, n, tol=.05, max_iter=1000, seed=0, summation="strided", dot="complete"):
    """qp_opt.m -> (lb, ub, passes)"""
    refresh_ref(cache, st, summation)
    half = F64(.5)
    ub = st.ww * half + loss_ref(cache, st, n)
    lb = st.lb
    st.sv[:n] = 1
    nxt = splitmix64(seed)
    t = 0
    with np.errstate(all="ignore"):
        while t < max_iter:
            one_ref(cache, st, shuffle(np.flatnonzero(st.sv[:n]), nxt), summation, dot)
            t += 1
            lb = st.lb
            ub_est = np.fmin(st.ub, ub)
            if lb > 0 and 1 - lb / ub_est < tol:
                ub = np.fmin(ub, st.ww * half + loss_ref(cache, st, n))
                if 1 - lb / ub < tol:
                    break
                st.sv[:n] = 1
    st.ub = ub
    return lb, ub, t


def prune_ref(cache, st, n, summation="strided"):
    """qp_prune.m -> (the pruned cache, its n); st changes in place"""
    x, ids, b, d = cache
    sv = st.sv.copy()
    if sv.all():
        sv = (st.a > 0).astype(np.uint8)
        sv[:st.nfix] = 1
    I = np.flatnonzero(sv[:n])
    assert len(I) > 0
    m = len(I)
    cache = qp_ref.keep_ref(cache, I)
    a = np.zeros_like(st.a)
    a[:m] = st.a[I]
    st.a = a
    st.sv[:] = 0
    st.sv[:m] = 1
    l = ZERO
    for j in range(m):
        l = l + F64(cache[2][j]) * st.a[j]
    st.l = l
    st.w = qp_ref.lincomb_ref(cache[0], st.a, np.arange(m), len(st.w))
    clamp(st)
    st.ww = wnorm(st.w, summation)
    st.lb = st.l - st.ww * F64(.5)
    return cache, m


def weights_ref(st, wreg, w0):
    return st.w / wreg + w0


# ---- drivers shared by the CPU and GPU tests ---------------------------------------------------------------------------------------------
def start_state(c, capacity=None, length=None):
    """a case's starting state (tests/qp_solve_cases.py) over a cache of the given capacity and dense length"""
    n = len(c["x"])
    st = State(capacity or n, length or len(c["w"]), n, c["noneg"])
    st.a[:n], st.l = c["a"], c["l"]
    st.w[:len(c["w"])] = c["w"]
    return st


def run_passes(c, summation, dot, capacity=None, length=None):
    """the case's consecutive passes -> ([per pass dict(loss, a, w, sv, l, order)], counters)"""
    from tests.qp_solve_cases import next_order
    cache = (c["x"], c["ids"], c["b"], c["d"])
    st, cnt, out = start_state(c, capacity, length), new_counters(), []
    for p in range(c["passes"]):
        order = next_order(c, p, st.sv)
        loss = pass_ref(cache, st, order, summation, dot, cnt)
        out.append(dict(loss=np.array([loss]), a=st.a.copy(), w=st.w.copy(), sv=st.sv.copy(), l=np.array([st.l]), order=order))
    return out, cnt


def opt_run(c, summation, dot, seed=11, tol=.05, capacity=None, length=None):
    """qp_opt from a = 0 on a case's cache -> (lb, ub, passes, state)"""
    n = len(c["x"])
    st = State(capacity or n, length or len(c["w"]), n, c["noneg"])
    lb, ub, t = opt_ref((c["x"], c["ids"], c["b"], c["d"]), st, n, tol, 1000, seed, summation, dot)
    return lb, ub, t, st
