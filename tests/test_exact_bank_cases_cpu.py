"""The exact filter-bank cases (tests/exact_bank_cases.py) are what they claim to be — no GPU:
agreement with the oracle bit for bit, exactness in any summation order under the split banks' arithmetic (the numpy model of
test_split_arith_cpu.py), SENSITIVITY (a bank that loses any one partial product, operand part or the border constant differs from the
reference at every filter slot and channel group) and the level geometry the GPU test runs on."""
import itertools

import numpy as np
import pytest

from tests import exact_bank_cases as X
from tests.test_split_arith_cpu import split2_f16, split3

BANK_IDS = [f"{nf}x{kh}x{kw}" for nf, kh, kw in X.BANKS] + ["mixed"]
BANK_SIZES = [[(kh, kw)] * nf for nf, kh, kw in X.BANKS] + [X.mixed_sizes()]


def levels_of(orc, frame):
    g = orc.geometry(frame[0], frame[1], X.SBIN, X.INTERVAL)
    return [(int(h), int(w)) for h, w in zip(g["cell_h"], g["cell_w"])]


def _cpu_levels(orc):
    """the levels the properties below are proved on: the second frame's without its largest (58 x 16 cells down to 17 x 4) — none of the
    properties depends on a level's size, and the generators draw every level from one distribution"""
    return levels_of(orc, X.FRAMES[1])[1:]


def test_geometry_coverage(orc):
    """What the GPU test's levels must contain: the height residues are where the wavefronts' 4-row units and the two-wavefront variants'
    8-row halves break, the width residues where a 16-cell unit is ragged.  (The issue asked for a 1 x 1 level: the pyramid cannot make one —
    its last level is at least 5 sbin pixels = 3 cells on the short side — so the smallest possible side, 3, stands in for it.)"""
    lv = [l for f in X.FRAMES for l in levels_of(orc, f)]
    assert min(min(l) for l in lv) == 3
    assert any(cw < 16 for _, cw in lv)
    assert {1, 15, 0} <= {cw % 16 for _, cw in lv}
    assert {1, 4, 5, 8, 9} <= {ch % 16 for ch, _ in lv}
    assert any(ch > 32 and cw > 32 for ch, cw in lv)                   # 3 x 3 tiles of 16 x 16 cells
    assert sum(ch * cw for ch, cw in lv) < 10000                       # (the GPU test reads every plane of every level)


def _oracle(orc, case, l, dtype):
    """orc.pdf_level per size group (the oracle's bank is uniform)"""
    out = np.zeros(case.ref[l].shape, dtype)
    for sz in set(case.sizes):
        idx = [n for n, s in enumerate(case.sizes) if s == sz]
        out[idx] = orc.pdf_level(case.feats[l], [case.filters[n] for n in idx], dtype)
    return out


@pytest.mark.parametrize("sizes", BANK_SIZES, ids=BANK_IDS)
def test_reference_is_the_oracles(orc, sizes):
    """ref_pdf == oracle.orc.pdf_level, bit for bit, on every case of every kind: in float32 and float64 for the float banks' cases, in
    float32 for the binary16 bank's and in float64 for the double handles'"""
    _reference_is_the_oracles(orc, _cpu_levels(orc), sizes)


def _only(cases, only):
    return [c for c in cases if only is None or c.name.startswith(tuple(only))]


def _reference_is_the_oracles(orc, lv, sizes, kinds=("f32", "f16", "f64"), only=None, build=X.build_cases, which=None):
    """which: the levels compared (all); the oracle is one call per (case, level, scalar type), whatever the level's size"""
    for kind, dtypes in (("f32", (np.float32, np.float64)), ("f16", (np.float32,)), ("f64", (np.float64,))):
        for case in _only(build(lv, sizes, kind), only) if kind in kinds else ():
            for l in which or range(len(lv)):
                for dt in dtypes:
                    assert np.array_equal(_oracle(orc, case, l, dt).astype(np.float64), case.ref[l]), (kind, case.name, l, dt)


# ---- the split banks' arithmetic as numpy planes ------------------------------------------------------------------------------------
BF16_PRODUCTS = [(1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0)]      # (feature part, weight part): k_conv_split32's sweeps
F16_PRODUCTS = [(0, 1), (1, 0), (0, 0)]


class SplitModel:
    """planes[(a, b)][l] = the exact contribution of product (feature part a x weight part b) to every response of level l (border included:
    the border constant is part h of a feature, 1 — 4096 scaled — in channel 31); border[b][l] = the border constant's share of planes[(0, b)]"""

    def __init__(self, case, kind):
        self.case, self.kind = case, kind
        if kind == "f16":
            self.products, one = F16_PRODUCTS, 4096.0
            fparts = [split2_f16(f, 12)[:2] for f in case.feats]
            e = [14 - int(np.frexp(np.abs(w).max())[1]) for w in case.filters]
            wparts = [split2_f16(w, ee)[:2] for w, ee in zip(case.filters, e)]
            self.scale = np.exp2(-(12.0 + np.array(e)))[:, None, None]
        else:
            self.products, one = BF16_PRODUCTS, 1.0
            fparts = [split3(f)[0] for f in case.feats]
            wparts = [split3(w)[0] for w in case.filters]
            self.scale = 1.0
        sz = case.sizes
        self.planes = {(a, b): [ref_b * self.scale for ref_b in (X.ref_pdf(fp[a], [w[b] for w in wparts], sz, border=one if a == 0 else 0.0) for fp in fparts)]
                       for a, b in self.products}
        self.border = {b: [X.ref_pdf(np.zeros_like(f), [w[b] for w in wparts], sz, border=one) * self.scale for f in case.feats]
                       for a, b in self.products if a == 0}
        self.fabs = [sum(np.abs(p.astype(np.float64)) for p in fp) for fp in fparts]
        self.wabs = [sum(np.abs(p.astype(np.float64)) for p in w) for w in wparts]
        self.nlev = len(case.feats)

    def total(self, l, keep=None):
        return sum(self.planes[p][l] for p in (keep if keep is not None else self.products))

    def deletions(self):
        """name -> per level: what the bank returns with that one thing lost"""
        P, nl = self.products, self.nlev
        out = {}
        for p in P:
            out[f"product f{p[0]} x w{p[1]}"] = [self.total(l, [q for q in P if q != p]) for l in range(nl)]
        for a in sorted({a for a, _ in P}):       # a feature part (the border constant is written by the tile staging, not by the feature's writer)
            kept = [[self.total(l, [q for q in P if q[0] != a])] + ([self.border[b][l] for fa, b in P if fa == 0] if a == 0 else []) for l in range(nl)]
            out[f"feature part {a}"] = [sum(k) for k in kept]
        for b in sorted({b for _, b in P}):
            out[f"weight part {b}"] = [self.total(l, [q for q in P if q[1] != b]) for l in range(nl)]
        out["border constant"] = [self.total(l) - sum(self.border[b][l] for a, b in P if a == 0) for l in range(nl)]
        return out


def _kinds():
    return [("f32", "bf16"), ("f16", "f16")]


@pytest.mark.parametrize("sizes", BANK_SIZES, ids=BANK_IDS)
def test_exact_in_any_order(orc, sizes):
    """The model's retained products add up to ref_pdf exactly; family A: every subset sum of a response's non-zero partial products is an fp32
    number; family B: sum over the window of (sum of |parts| of f) x (sum of |parts| of w) < 2^24 units — no partial sum of any subset of part
    products, in any order, leaves the integers that fp32 holds exactly."""
    _exact_in_any_order(orc, _cpu_levels(orc), sizes)


def _exact_in_any_order(orc, lv, sizes, only=None, models=None, build=X.build_cases):
    """models: a dict that takes the family-A cases' SplitModel by (kind, case name), for _unnoticed on the same levels and bank"""
    for kind, _ in _kinds():
        for case in _only(build(lv, sizes, kind), only):
            m = SplitModel(case, kind)
            if models is not None and case.delta is not None:
                models[kind, case.name] = m
            for l in range(len(lv)):
                assert np.array_equal(m.total(l), case.ref[l]), (kind, case.name, l)
                if case.delta is not None:
                    live = [p for p in m.products if m.planes[p][l].any()]
                    for k in range(1, len(live)):
                        for sub in itertools.combinations(live, k):
                            assert X.is_fp32(m.total(l, list(sub))).all(), (kind, case.name, l, sub)
                else:
                    scale = m.scale if kind == "f16" else 1.0
                    worst = (X.ref_pdf(m.fabs[l], m.wabs, case.sizes, border=4096.0 if kind == "f16" else 1.0) * scale).max() / case.unit
                    assert worst < 2.0 ** 24, (kind, case.name, l, worst)


def _unnoticed(orc, sizes, kind, families="A", drop=(), lv=None, models=None, build=X.build_cases):
    """deletion -> the (filter, channel group) pairs at which NO family-A case tells the damaged bank from the reference.  (A one-tap filter
    reads no cell outside the level: the border constant is no part of its responses, and nothing is asked of it there.)"""
    lv = lv or _cpu_levels(orc)
    cases = [c for c in build(lv, sizes, kind, families) if not c.name.startswith(tuple(drop) or ("\0",))]
    nf = len(sizes)
    seen = {}
    for case in cases:
        tap, chan = case.delta
        for name, planes in (models[kind, case.name] if models else SplitModel(case, kind)).deletions().items():
            hit = np.zeros(nf, bool)
            for l in range(len(lv)):
                hit |= (planes[l] != case.ref[l]).reshape(nf, -1).any(axis=1)
            seen.setdefault(name, set()).update((n, int(chan[n]) // 8) for n in np.flatnonzero(hit))
    want = {(n, g) for n in range(nf) for g in range(4)}
    border = {(n, 3) for n in range(nf) if sizes[n][0] * sizes[n][1] > 1}
    return {name: sorted((want if name != "border constant" else border) - got) for name, got in seen.items()}


@pytest.mark.parametrize("kind,parts", _kinds(), ids=["bf16x6", "f16x3"])
@pytest.mark.parametrize("sizes", BANK_SIZES, ids=BANK_IDS)
def test_sensitivity(orc, sizes, kind, parts):
    """Delete, in the model, each retained partial product, each part of the features, each part of the weights and the border constant of
    channel 31: family A must then differ from ref_pdf at every (filter slot mod 32, n-tile) = filter and every 8-channel group (the border
    constant: channel 31's group)."""
    _sensitive(orc, sizes, kind)


def _sensitive(orc, sizes, kind, lv=None, models=None, build=X.build_cases):
    missing = _unnoticed(orc, sizes, kind, lv=lv, models=models, build=build)
    assert len(missing) == (13 if kind == "f32" else 8)
    assert not any(missing.values()), {k: v[:8] for k, v in missing.items() if v}


def test_sensitivity_needs_every_family(orc):
    """the proof above is not vacuous: without A1 nothing sees a lost l part of the features, without A2 a lost l part of the weights, without
    A3 the lost m x m product"""
    sizes = [(5, 5)] * 33
    for drop, lost in (("A1", "feature part 2"), ("A2", "weight part 2"), ("A3", "product f1 x w1")):
        missing = _unnoticed(orc, sizes, "f32", drop=(drop,))
        assert missing[lost], (drop, lost)


# ---- the split banks' instantiation matrix and the sweep of the 81 filter sizes -----------------------------------------------------
# (tests/test_gpu_split_bank_matrix.py, tests/test_gpu_filter_sizes.py: the same proofs on their banks, on the levels those tests run)
MATRIX_IDS = [f"{nf}x{kh}x{kw}" for nf, kh, kw in X.MATRIX_BANKS] + ["mixed"]
MATRIX_SIZES = [[(kh, kw)] * nf for nf, kh, kw in X.MATRIX_BANKS] + [X.matrix_mixed_sizes()]
MATRIX_FAMILIES = ("A1", "A2", "A3", "B2")


def _matrix_levels(orc):
    """the matrix's second frame (6 x 6, 4 x 5, 3 x 3 cells); the sweep: the three smallest levels of its frame (6 x 6, 5 x 5, 3 x 3:
    on fewer cells a corner tap of a 9 x 9 filter meets too few in-level features to notice every lost part).  As in _cpu_levels, the
    properties proved here hold level by level, and the banks do not depend on the levels at all"""
    return levels_of(orc, X.MATRIX_FRAMES[1])


def _sweep_levels(orc):
    return levels_of(orc, X.SWEEP_FRAME)[-3:]


def _prove(orc, lv, sizes, kinds, only, oracle_levels=None):
    """the three proofs above on one bank, its cases built once per kind"""
    built = {}

    def build(lv_, sizes_, kind, families="AB"):
        assert lv_ is lv and sizes_ is sizes
        if kind not in built:
            built[kind] = X.build_cases(lv, sizes, kind)
        return [c for c in built[kind] if c.name[0] in families]

    _reference_is_the_oracles(orc, lv, sizes, kinds=kinds, only=only, build=build, which=oracle_levels)
    models = {}
    _exact_in_any_order(orc, lv, sizes, only=only, models=models, build=build)
    for kind, _ in _kinds():
        assert sum(k == kind for k, _ in models) == 3 * X.ROUNDS
        _sensitive(orc, sizes, kind, lv=lv, models=models, build=build)


def test_one_tap_filters_stay_in_the_level():
    """a 1 x 1 filter's delta stays at its only tap, the anchor, in every round (the border round included); every other size keeps the
    border round away from the anchor"""
    tap, chan = X.placements([(1, 1)] * 17 + [(1, 2)] * 17 + [(2, 1)] * 17)
    assert (tap[:, :17] == 0).all() and (chan[X.ROUNDS - 1] == X.FLEN - 1).all()
    assert (tap[X.ROUNDS - 1, 17:34] == 0).all() and (tap[X.ROUNDS - 1, 34:] == 0).all()      # anchors (0, 1) and (1, 0): tap 1 of both


@pytest.mark.parametrize("sizes", MATRIX_SIZES, ids=MATRIX_IDS)
def test_matrix_banks_prove_themselves(orc, sizes):
    """the reference is the oracle's, the cases are exact in any order under both split arithmetics, and a bank that loses one product, part
    or the border constant differs at every filter and channel group — on the matrix's banks and families"""
    _prove(orc, _matrix_levels(orc), sizes, ("f32", "f16"), MATRIX_FAMILIES)


@pytest.mark.parametrize("kh,kw", X.SWEEP_SIZES, ids=[f"{kh}x{kw}" for kh, kw in X.SWEEP_SIZES])
def test_sweep_sizes_prove_themselves(orc, kh, kw):
    """the same for 33 filters of every documented size, for every kind of handle and every family (the oracle on the 6 x 6 level: cells
    whose window leaves the level on one side, on two and, from 8 x 8 on, on all four)"""
    _prove(orc, _sweep_levels(orc), [(kh, kw)] * X.SWEEP_FILTERS, ("f32", "f16", "f64"), None, oracle_levels=[0])
