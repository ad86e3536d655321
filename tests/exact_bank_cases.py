"""Operands on which the filter bank (SpatialConvolutionEngine::pdf) has an EXACT answer, and that answer — plain numpy, no GPU, no oracle.

Every response of every case is an fp32 number, and so is every partial sum on the way to it, in any summation order and under the
split banks' decomposition into partial products (k_conv_split.hip).  Whatever bank computes them — the ordered fp32 chain, the fp32 /
fp64 MFMA chains, six bfloat16 products, three binary16 products — must return the bits of `ref_pdf`; a lost part, product, tap, channel,
filter slot or border constant is a bit difference at a known (level, y, x, filter).

Family A — delta filters: filter n has ONE non-zero weight w_n at tap t_n, channel c_n, so a response is one product (under the border:
w_n * 1 for channel 31, else 0) and a k-step's matrix instruction adds at most one non-zero product to its accumulator.
  A1  feature parts: features with full 24-bit mantissas in [2^-3, 2^-1), ~30 % next to bfloat16 rounding boundaries (parts of both signs),
      w_n = +-2^k: the product's parts are the feature's.
  A2  weight parts: features 2^-(1 + (x + 2 y + c) % 4), w_n with a full mantissa; the channel-31 round pins the border's 1 against all weight parts.
  A3  cross products: features of exactly 11 significant bits, weights of exactly 12 (parts h and m non-zero, l = 0, product <= 23 bits):
      h h, h m, m h and m m are all needed.
  kind "f16" (PBD_CONV_SPLIT_F16, two binary16 parts of the scaled operand): A1 / A2 with 22-bit mantissas, A3 with 11 x 11 bits (the
      mode drops m m by design); every scaled part is a normal binary16.
  kind "f64" adds AF: 24-bit features x 24-bit weights, a 48-bit product — exact in fp64 only (double handles).
  Placement: (t_n, c_n) rotate with n and with the round r; over the ROUNDS banks of a size every tap and channel occurs, every filter slot
  sees all four 8-channel groups (both k-steps x both k-groups) in rounds 0-3 and channel 31 in the last round — at a tap other than the
  anchor, so that the weight meets the border's 1 (a 1 x 1 filter has the anchor only: no response of it reads outside the level).
Family B — dense small integers (multiples of one unit u, sum |f| |w| / u < 2^24 over the worst window, border included): exact in any
  order, whole-K accumulation.  B1: 6-bit features x 4-bit weights; B2: 11-bit features x {0, +-1, +-2} 2^j; B3: 11-bit weights x {1, 2} 2^j."""
import numpy as np

FLEN = 32
SBIN, INTERVAL = 4, 3
FRAMES = [(174, 161), (88, 299)]          # w x h; tests/test_exact_bank_cases_cpu.py checks what their levels cover
BANKS = [(16, 5, 5), (33, 5, 5), (161, 5, 5), (33, 3, 3), (33, 9, 9), (33, 3, 7), (33, 6, 4)]   # (filters, kh, kw)
MIXED_SIZES = [(3, 3)] * 20 + [(5, 5)] * 37 + [(3, 7)] * 12      # size groups of 20 / 37 / 12: both boundaries inside an n-tile
ROUNDS = 5
# The split banks' instantiation matrix (tests/test_gpu_split_bank_matrix.py; what these banks reach in k_conv_split32: tests/split_bank_census.py,
# asserted by tests/test_split_bank_matrix_cpu.py).  32-filter n-tiles run in groups of five, then a remainder launch.
MATRIX_FRAMES = [(76, 76), (33, 32)]      # w x h: levels 17 x 17 .. 4 x 4 (every count of M-tiles per wavefront) and 6 x 6, 4 x 5, 3 x 3
MATRIX_BANKS = [(16, 6, 4), (65, 5, 5), (96, 6, 4), (97, 3, 7), (128, 2, 2), (160, 6, 4),      # first launches of 1, 3, 3, 4, 4, 5 n-tiles
                (193, 3, 3), (225, 3, 3), (257, 3, 3), (321, 3, 3),                           # 5 + 2, 5 + 3, 5 + 4, two groups of 5 and 1 more
                (17, 1, 1), (33, 1, 1), (17, 1, 2), (17, 2, 1), (33, 1, 2)]                   # the shortest K loops on 1 and 2 n-tiles
MATRIX_MIXED = [(3, 3)] * 65 + [(5, 5)] * 97 + [(3, 7)] * 161 + [(6, 4)] * 16 + [(1, 1)] * 33     # size groups of 3, 4, 5 + 1, 1 and 2 n-tiles
SWEEP_FRAME = (52, 52)                    # tests/test_gpu_filter_sizes.py: levels 11 x 11 .. 3 x 3, every one under a 16 x 16 unit
SWEEP_FILTERS = 33
SWEEP_SIZES = [(kh, kw) for kh in range(1, 10) for kw in range(1, 10)]      # include/pbd_c.h: kh, kw in 1..9
BF16_EDGES = np.array([0x7FFF, 0x8000, 0x8001, 0x7F80, 0x807F, 0xFFFF], np.uint32)      # low 16 bits next to a bfloat16 rounding boundary
F16_EDGES = np.array([0x0FFC, 0x1000, 0x1004, 0x0004, 0x1FFC, 0x0FF8], np.uint32)       # low 13 bits (22-bit mantissa) next to a binary16 one


def mixed_sizes():
    """MIXED_SIZES in a fixed shuffled order: the caller's filter order is not the library's size-sorted one"""
    return [MIXED_SIZES[i] for i in np.random.default_rng(5).permutation(len(MIXED_SIZES))]


def matrix_mixed_sizes():
    """MATRIX_MIXED in a fixed shuffled order"""
    return [MATRIX_MIXED[i] for i in np.random.default_rng(6).permutation(len(MATRIX_MIXED))]


def is_fp32(a):
    a = np.asarray(a, np.float64)
    return a.astype(np.float32).astype(np.float64) == a


def ref_pdf(feat, filters, sizes, border=1.0):
    """float64 direct correlation with the bank's rules: feat [H, W, 32], filters[n] kh_n x (kw_n * 32), sizes[n] = (kh_n, kw_n); anchor
    (kh / 2, kw / 2); outside the level every channel reads 0, channel 31 reads `border`.  -> [n, H, W] float64"""
    feat = np.asarray(feat, np.float64)
    H, W, _ = feat.shape
    out = np.zeros((len(filters), H, W), np.float64)
    for kh, kw in sorted(set(map(tuple, sizes))):
        idx = [n for n, s in enumerate(sizes) if tuple(s) == (kh, kw)]
        wg = np.stack([np.asarray(filters[n], np.float64).reshape(kh, kw, FLEN) for n in idx])
        pad = np.zeros((H + kh - 1, W + kw - 1, FLEN), np.float64)
        pad[..., FLEN - 1] = border
        pad[kh // 2:kh // 2 + H, kw // 2:kw // 2 + W] = feat
        acc = np.zeros((len(idx), H, W), np.float64)
        for dy in range(kh):
            for dx in range(kw):
                nz = np.flatnonzero(np.any(wg[:, dy, dx, :] != 0, axis=1))          # (zero taps add nothing)
                if len(nz):
                    acc[nz] += np.tensordot(wg[nz, dy, dx, :], pad[dy:dy + H, dx:dx + W, :], axes=([1], [2]))
        out[idx] = acc
    return out


class Case:
    """One bank and one set of level features.  delta: (tap, channel) of every filter for family A, None for family B."""

    def __init__(self, name, feats, filters, sizes, delta=None, unit=None):
        self.name, self.feats, self.filters, self.sizes, self.delta, self.unit = name, feats, filters, sizes, delta, unit
        self.ref = [ref_pdf(f, filters, sizes) for f in feats]
        for l, r in enumerate(self.ref):
            assert is_fp32(r).all() or name.startswith("AF"), (name, l)               # a badly built case fails itself
            assert np.isfinite(r).all()


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def _mant(rng, shape, bits, elo, ehi, exact_bits=False):
    """positive float32 with at most `bits` significant bits (exact_bits: leading and trailing bit set), magnitude in [2^elo, 2^ehi)"""
    m = rng.integers(1 << (bits - 1), 1 << bits, shape)
    if exact_bits:
        m |= 1
    e = rng.integers(elo, ehi, shape)
    return np.ldexp(m.astype(np.float64), e - bits + 1).astype(np.float32)


def bf16_parts(x):
    """three exact bfloat16 parts of float32 x (round to nearest even) — the generators' own copy of the split, used to BUILD operands only"""
    parts, r = [], np.asarray(x, np.float32).copy()
    for _ in range(3):
        u = r.view(np.uint32).astype(np.uint64)
        p = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
        parts.append(p)
        r = (r - p).astype(np.float32)
    return parts


def _subsets_ok(x):
    """every sum of a subset of x's three bfloat16 parts is an fp32 number"""
    h, m, l = (p.astype(np.float64) for p in bf16_parts(x))
    ok = np.ones(x.shape, bool)
    for s in (h + m, h + l, m + l, h + m + l):
        ok &= is_fp32(s)
    return ok


def _full(rng, shape, elo, ehi, kind, all_parts=False):
    """full-mantissa operands (24 bits; kind "f16": 22), ~30 % of them next to the parts' rounding boundaries, every subset sum of the parts
    an fp32 number (the rare value whose h part rounds up into the next binade while l is odd and positive is drawn again).  all_parts: no
    part is zero (a bank's few weights must each notice a lost part; among a level's thousands of features the zero parts are welcome)"""
    def ok(x):
        if kind == "f16":
            return (x.view(np.uint32) & np.uint32(0x1FFC)) != 0 if all_parts else np.ones(x.shape, bool)
        good = _subsets_ok(x)
        if all_parts:
            good &= np.logical_and.reduce([p != 0 for p in bf16_parts(x)])
        return good
    x = _mant(rng, shape, 24, elo, ehi)
    u = x.view(np.uint32).copy()
    pick = rng.random(shape) < 0.3
    if kind == "f16":
        u &= np.uint32(0xFFFFFFFC)
        u[pick] = (u[pick] & np.uint32(0xFFFFE000)) | rng.choice(F16_EDGES, int(pick.sum()))
    else:
        u[pick] = (u[pick] & np.uint32(0xFFFF0000)) | rng.choice(BF16_EDGES, int(pick.sum()))
    x = u.view(np.float32).copy()
    for _ in range(64):
        bad = ~ok(x)
        if not bad.any():
            return x
        fresh = _mant(rng, int(bad.sum()), 24, elo, ehi)
        x[bad] = (fresh.view(np.uint32) & np.uint32(0xFFFFFFFC)).view(np.float32) if kind == "f16" else fresh
    raise AssertionError("could not draw operands whose parts sum exactly")


def placements(sizes):
    """tap[r][n], chan[r][n] of the delta filters of round r; asserts the coverage the docstring promises"""
    nf = len(sizes)
    tap, chan = np.zeros((ROUNDS, nf), int), np.zeros((ROUNDS, nf), int)
    rank = {n: (j, sum(tuple(s) == tuple(sz) for s in sizes)) for sz in set(map(tuple, sizes))
            for j, n in enumerate(m for m, s in enumerate(sizes) if tuple(s) == sz)}     # n -> (rank inside its size group, the group's size)
    for r in range(ROUNDS):
        for n, (kh, kw) in enumerate(sizes):
            k = r * nf + n
            tap[r, n] = (r * rank[n][1] + rank[n][0] + r) % (kh * kw)
            if r == ROUNDS - 1 and kh * kw > 1:                      # the border round: any tap but the anchor (which never leaves the level);
                anchor = (kh // 2) * kw + kw // 2                    # a one-tap filter has no other: its channel-31 weight meets in-level features only
                tap[r, n] = tap[r, n] % (kh * kw - 1)
                tap[r, n] += tap[r, n] >= anchor
            chan[r, n] = FLEN - 1 if r == ROUNDS - 1 else 8 * ((n + r) % 4) + (k // 4 + n // 32) % 8
    assert set(chan.ravel()) == set(range(FLEN))
    for sz in set(map(tuple, sizes)):
        idx = [n for n, s in enumerate(sizes) if tuple(s) == sz]
        assert set(tap[:, idx].ravel()) == set(range(sz[0] * sz[1])), sz
    assert all(set(chan[:4, n] // 8) == {0, 1, 2, 3} for n in range(nf)) and (chan[4] == FLEN - 1).all()
    return tap, chan


def _delta_bank(sizes, tap, chan, w):
    filters = []
    for n, (kh, kw) in enumerate(sizes):
        f = np.zeros((kh, kw, FLEN), np.float32)
        f[tap[n] // kw, tap[n] % kw, chan[n]] = w[n]
        filters.append(f.reshape(kh, kw * FLEN))
    return filters


def family_a(levels, sizes, kind="f32", seed=0):
    """levels: [(ch, cw)]; sizes: (kh, kw) per filter; kind "f32" | "f16" | "f64" -> list of Case (A1, A2, A3 [, AF] x ROUNDS)"""
    nf = len(sizes)
    tap, chan = placements(sizes)
    n = np.arange(nf)
    cases = []
    for r in range(ROUNDS):
        rng, wrng = np.random.default_rng([seed, r, nf]), np.random.default_rng([seed, r, nf, 1])   # (the bank does not depend on the levels)
        sign = np.where((n // 2 + r) % 2, -1.0, 1.0)
        # A1: the feature's parts
        w = sign * np.exp2((n + r) % 10 - 6.0)
        feats = [_full(rng, (ch, cw, FLEN), -3, -1, kind) for ch, cw in levels]
        cases.append(Case(f"A1.r{r}", feats, _delta_bank(sizes, tap[r], chan[r], w), sizes, (tap[r], chan[r])))
        # A2: the weight's parts
        w = sign * _full(wrng, nf, -6, 3, kind, all_parts=True)
        feats = []
        for ch, cw in levels:
            y, x, c = np.ogrid[0:ch, 0:cw, 0:FLEN]
            feats.append(np.exp2(-(1.0 + (x + 2 * y + c) % 4)).astype(np.float32))
        cases.append(Case(f"A2.r{r}", feats, _delta_bank(sizes, tap[r], chan[r], w), sizes, (tap[r], chan[r])))
        # A3: the cross products
        w = sign * _mant(wrng, nf, 11 if kind == "f16" else 12, -6, 3, exact_bits=True)
        feats = [_mant(rng, (ch, cw, FLEN), 11, -3, -1, exact_bits=True) for ch, cw in levels]
        cases.append(Case(f"A3.r{r}", feats, _delta_bank(sizes, tap[r], chan[r], w), sizes, (tap[r], chan[r])))
        if kind == "f64":
            w = sign * _full(wrng, nf, -6, 3, kind)
            feats = [_full(rng, (ch, cw, FLEN), -3, -1, kind) for ch, cw in levels]
            cases.append(Case(f"AF.r{r}", feats, _delta_bank(sizes, tap[r], chan[r], w), sizes, (tap[r], chan[r])))
    return cases


LIMIT = float(1 << 24)


def family_b(levels, sizes, seed=0):
    """-> [B1, B2, B3].  Features are integers x 2^-fbits (so the border's 1 is 2^fbits units, no larger than the largest feature allowed),
    weights integers x 2^-6; the widths shrink until ntaps x 32 x max |f| x max |w| < 2^24 for the bank's largest filter."""
    nf = len(sizes)
    terms = max(kh * kw for kh, kw in sizes) * FLEN
    rng, wrng = np.random.default_rng([seed, 77, nf]), np.random.default_rng([seed, 77, nf, 1])
    uw = 2.0 ** -6

    def widths(fbits, wmax_of_j):
        """largest (fbits', j) with terms * 2^fbits' * wmax(j) < 2^24, fbits' <= fbits, j >= 0 preferred large"""
        for fb in range(fbits, 0, -1):
            js = [j for j in range(0, 12) if terms * (1 << fb) * wmax_of_j(j) < LIMIT]
            if js:
                return fb, max(js)
        raise AssertionError("no exact range for this filter size")

    def bank(draw):
        return [(draw((kh, kw, FLEN)) * uw).astype(np.float32).reshape(kh, kw * FLEN) for kh, kw in sizes]

    def check(case, uf):
        worst = max(float(ref_pdf(np.abs(f), [np.abs(w) for w in case.filters], sizes).max()) for f in case.feats) / (uf * uw)
        assert worst < LIMIT, (case.name, worst)
        case.unit = uf * uw
        return case

    cases = []
    # B1: 6-bit features x 4-bit weights
    fb, _ = widths(6, lambda j: 15)
    feats = [rng.integers(1, 1 << fb, (ch, cw, FLEN)) * 2.0 ** -fb for ch, cw in levels]
    cases.append(check(Case("B1", [f.astype(np.float32) for f in feats],
                            bank(lambda s: wrng.integers(1, 16, s) * wrng.choice([-1, 1], s)), sizes), 2.0 ** -fb))
    # B2: 11-bit features (parts h and m) x {0, +-1, +-2} 2^j
    fb, jm = widths(11, lambda j: 2 << j)
    feats = [(rng.integers(1 << (fb - 1), 1 << fb, (ch, cw, FLEN)) | 1) * 2.0 ** -fb for ch, cw in levels]
    cases.append(check(Case("B2", [f.astype(np.float32) for f in feats],
                            bank(lambda s: wrng.choice([0, 1, -1, 2, -2], s) * (1 << wrng.integers(0, jm + 1, s))), sizes), 2.0 ** -fb))
    # B3: the mirror — 11-bit weights x features {1, 2} 2^j, the largest feature = 1 = the border's constant
    wb, jm = widths(11, lambda j: 2 << j)         # (the same product bound with the roles swapped: wb weight bits, features up to 2 2^jm units)
    uf = 2.0 ** -(jm + 1)
    feats = [rng.choice([1, 2], (ch, cw, FLEN)) * (1 << rng.integers(0, jm + 1, (ch, cw, FLEN))) * uf for ch, cw in levels]
    cases.append(check(Case("B3", [f.astype(np.float32) for f in feats],
                            bank(lambda s: (wrng.integers(1 << (wb - 1), 1 << wb, s) | 1) * wrng.choice([-1, 1], s)), sizes), uf))
    return cases


def build_cases(levels, sizes, kind="f32", families="AB"):
    """every case of one bank geometry: kind "f32" (EXACT, MFMA, SPLIT on float handles), "f16" (PBD_CONV_SPLIT_F16), "f64" (double handles)"""
    cases = []
    if "A" in families:
        cases += family_a(levels, sizes, kind)
    if "B" in families:
        cases += family_b(levels, sizes)
    return cases
