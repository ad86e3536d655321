"""Hard-negative mining (include/pbd_c.h "hard-negative mining") restated in numpy: the upper bound's per-frame sum and the action,
as tests/qp_solve_ref.py restates the solver.  No GPU, nothing of the library."""
import numpy as np

PBD_MINE_NONE, PBD_MINE_ONE, PBD_MINE_OPT = 0, 1, 2


def ub_terms(scores, cneg):
    """detect.m:135 per record: cneg * max(1 + (double)score, 0), the sum and the product each rounded to float64"""
    s = np.asarray(scores, np.float32).astype(np.float64)
    return np.float64(cneg) * np.maximum(np.float64(1.0) + s, np.float64(0.0))


def block_sum(t):
    """the library's block sum: 64 lane-strided partials starting at +0.0, each added up in index order, folded s[i] += s[i + h] for
    h = 32 .. 1"""
    t = np.asarray(t, np.float64)
    part = np.zeros(64, np.float64)
    for lane in range(64):
        acc = np.float64(0.0)
        for v in t[lane::64]:
            acc = acc + v
        part[lane] = acc
    h = 32
    while h >= 1:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return np.float64(part[0])


def ub_term_sum(scores, cneg):
    """S_f of a frame whose records, in record order, have these scores"""
    return block_sum(ub_terms(scores, cneg))


def action(lb, ub, n, capacity):
    """detect.m:148-149 and :315-324: lb < 0 or a full cache -> OPT; else 1 - lb / ub > .05 -> ONE; else NONE.  ub == 0 divides as
    IEEE does (MATLAB's rule): +-inf, or NaN, which compares false"""
    lb, ub = np.float64(lb), np.float64(ub)
    if lb < 0 or n == capacity:
        return PBD_MINE_OPT
    with np.errstate(divide="ignore", invalid="ignore"):
        return PBD_MINE_ONE if np.float64(1.0) - lb / ub > np.float64(.05) else PBD_MINE_NONE
