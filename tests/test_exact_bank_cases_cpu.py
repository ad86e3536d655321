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
    lv = _cpu_levels(orc)
    for kind, dtypes in (("f32", (np.float32, np.float64)), ("f16", (np.float32,)), ("f64", (np.float64,))):
        for case in X.build_cases(lv, sizes, kind):
            for l in range(len(lv)):
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
    lv = _cpu_levels(orc)
    for kind, _ in _kinds():
        for case in X.build_cases(lv, sizes, kind):
            m = SplitModel(case, kind)
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


def _unnoticed(orc, sizes, kind, families="A", drop=()):
    """deletion -> the (filter, channel group) pairs at which NO family-A case tells the damaged bank from the reference"""
    lv = _cpu_levels(orc)
    cases = [c for c in X.build_cases(lv, sizes, kind, families) if not c.name.startswith(tuple(drop) or ("\0",))]
    nf = len(sizes)
    seen = {}
    for case in cases:
        tap, chan = case.delta
        for name, planes in SplitModel(case, kind).deletions().items():
            hit = np.zeros(nf, bool)
            for l in range(len(lv)):
                hit |= (planes[l] != case.ref[l]).reshape(nf, -1).any(axis=1)
            seen.setdefault(name, set()).update((n, int(chan[n]) // 8) for n in np.flatnonzero(hit))
    want = {(n, g) for n in range(nf) for g in range(4)}
    return {name: sorted((want if name != "border constant" else {(n, 3) for n in range(nf)}) - got) for name, got in seen.items()}


@pytest.mark.parametrize("kind,parts", _kinds(), ids=["bf16x6", "f16x3"])
@pytest.mark.parametrize("sizes", BANK_SIZES, ids=BANK_IDS)
def test_sensitivity(orc, sizes, kind, parts):
    """Delete, in the model, each retained partial product, each part of the features, each part of the weights and the border constant of
    channel 31: family A must then differ from ref_pdf at every (filter slot mod 32, n-tile) = filter and every 8-channel group (the border
    constant: channel 31's group)."""
    missing = _unnoticed(orc, sizes, kind)
    assert len(missing) == (13 if kind == "f32" else 8)
    assert not any(missing.values()), {k: v[:8] for k, v in missing.items() if v}


def test_sensitivity_needs_every_family(orc):
    """the proof above is not vacuous: without A1 nothing sees a lost l part of the features, without A2 a lost l part of the weights, without
    A3 the lost m x m product"""
    sizes = [(5, 5)] * 33
    for drop, lost in (("A1", "feature part 2"), ("A2", "weight part 2"), ("A3", "product f1 x w1")):
        missing = _unnoticed(orc, sizes, "f32", drop=(drop,))
        assert missing[lost], (drop, lost)
