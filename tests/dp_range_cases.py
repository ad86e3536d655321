"""Test helper: DP cases at the edges of the domain — signed zeros (Z), magnitudes (M), extreme quadratics (Q) and anchors at or beyond
the level's size (A).  No GPU import.  A case is dict(name, family, model, resp=(rng, model, H, W, dtype) -> [nfilters, H, W], dp_mode,
exact, dtypes): a model of make_tree_model_k whose deformations, anchors and biases are overwritten in place.  `exact`: every sum of the DP
is exact in float (and so in double), so re-scoring a configuration in float64 reproduces its score bit for bit.

Everything here is FINITE by construction (tests/test_dp_range_cpu.py proves it on the oracle for every case before a GPU sees one):
tree_bound() is the largest magnitude any partial sum over the tree can reach, and every case keeps it below max(T) / 2."""
import numpy as np

from partsbaseddetector_amd.model import make_tree_model_k

FRAME = (100, 80)            # w, h of the GPU tests' frame: 21 levels, from 23 x 18 cells down to 4 x 3
DTYPES = (np.float32, np.float64)

# the tree shapes and mixture counts of TIE_CASES (tests/test_gpu_mixture_counts.py): fold widths M = 1, 4, 6, 8, siblings of every count
# (the three-kernel structure runs them with dp_mode 1), K > 8
TREES = {
    "M1": ([-1, 0, 1, 1, 0], [1, 1, 1, 1, 1]),
    "M4": ([-1, 0, 1, 1, 0], [4, 2, 4, 3, 1]),
    "M6": ([-1, 0, 1, 2, 0, 4], [6, 1, 6, 2, 5, 3]),
    "M8": ([-1, 0, 0, 0, 0, 0, 0, 0, 0], [2, 1, 2, 3, 4, 5, 6, 7, 8]),
    "K10": ([-1, 0, 1, 0], [3, 10, 4, 2]),
}
CLIP = 6.0                   # N(0, 1) draws are clipped to +-CLIP so that the magnitude bound is a proof, not a likelihood


def _model(tree, seed, **kw):
    parents, Ks = TREES[tree]
    m = make_tree_model_k(parents, Ks, seed=seed, **kw)
    m.defw = np.array(m.defw, np.float32)
    m.anchors = np.array(m.anchors, np.int32)
    m.biasw = np.array(m.biasw, np.float32)
    return m


def _normal(scale=1.0):
    def make(rng, model, H, W, dtype):
        r = np.clip(rng.normal(0, 1, (len(model.filtersw), H, W)), -CLIP, CLIP)
        return (r * scale).astype(dtype)
    return make


def _quant(rng, model, H, W, dtype):
    return (rng.integers(-4, 5, (len(model.filtersw), H, W)) * 0.25).astype(dtype)


def _zeros(values, weights):
    def make(rng, model, H, W, dtype):
        return np.asarray(values, dtype)[rng.choice(len(values), (len(model.filtersw), H, W), p=weights)]
    return make


def def_diag(model, H, W):
    """the largest |deformation cost| any (parent, child) pair of an H x W level can meet: |a| d^2 + |b| d at the farthest distance
    d = side + |anchor| on each axis, maximised over the deformation rows"""
    w = np.abs(np.asarray(model.defw, np.float64).reshape(-1, 4))
    a = np.abs(np.asarray(model.anchors, np.float64).reshape(-1, 2))
    dx, dy = W + a[:, 0], H + a[:, 1]
    return float((w[:, 0] * dx * dx + w[:, 1] * dx + w[:, 2] * dy * dy + w[:, 3] * dy).max())


def tree_bound(model, resp, comp=0):
    """parts x (|response| + |bias| + deformation at the level's diagonal): no partial sum of the DP exceeds it in magnitude"""
    _, H, W = resp.shape
    return model.nparts(comp) * (float(np.abs(resp).max()) + float(np.abs(model.biasw).max()) + def_diag(model, H, W))


def _case(name, family, model, resp, dp_mode=0, exact=False, dtypes=DTYPES, **extra):
    return dict(name=name, family=family, model=model, resp=resp, dp_mode=dp_mode, exact=exact, dtypes=tuple(dtypes), **extra)


# ---------------------------------------------------------------- Z: signed zeros
def _z_cases():
    """Planes of zeros of both signs (and +-1/4), biases 0.0 and -0.0, the root's bias -0.0 (x + 0.0 is +0.0 for both zeros: a +0.0 root
    bias would wipe the sign off every root score), quantised deformations.  a d^2 + b d + y at d = 0 is (-0.0) + (b * 0) + y: a linear
    weight w1 >= 0 (b = -w1 <= -0.0) keeps the sign of y, w1 < 0 turns -0.0 into +0.0 — the model's rows hold both kinds, so the K
    weighted maps of a reduce hold both zeros at one cell and tie under `>`.  A sum is -0.0 only where EVERY addend is: -0.0 is the
    likelier draw in the planes (80 %) and the biases (70 %), and the first mixture of every part has bias(0)[0] = -0.0 and linear
    weights >= 0 (the other rows: 30 % negative), so that root scores of a nine-part tree still hold -0.0 — where the first mixtures'
    planes are all -0.0 and win their ties with the +0.0 of later mixtures only because they come first."""
    out = []
    kinds = {"zeros": ((-0.0, 0.0), (0.8, 0.2)), "zq": ((-0.0, 0.0, -0.25, 0.25), (0.6, 0.2, 0.196, 0.004))}
    plan = [("M1", "zeros", 0), ("M4", "zq", 0), ("M6", "zeros", 0), ("M8", "zq", 0), ("M8", "zeros", 1), ("K10", "zq", 0), ("M4", "zeros", 2)]
    for i, (tree, kind, mode) in enumerate(plan):
        m = _model(tree, 300 + i, quantised=True)
        rng = np.random.default_rng(310 + i)
        m.biasw = np.where(rng.random(len(m.biasw)) < 0.7, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        m.biasw[0] = np.float32(-0.0)
        lin = np.abs(m.defw[:, [1, 3]])
        lin[rng.random(lin.shape) < 0.3] *= np.float32(-1.0)
        m.defw[:, [1, 3]] = lin
        for p in range(1, m.nparts(0)):          # the path through every first mixture keeps the sign: bias(0)[0] = -0.0, w1, w3 >= 0
            m.biasw[m.biasid[0][p][0]] = np.float32(-0.0)
            m.defw[m.defid[0][p][0], [1, 3]] = np.abs(m.defw[m.defid[0][p][0], [1, 3]])
        out.append(_case(f"Z_{kind}_{tree}_mode{mode}", "Z", m, _zeros(*kinds[kind]), mode, exact=True))
    return out


# ---------------------------------------------------------------- M: magnitudes
# 2^k per type: 0, about +- half the exponent range, and the top: parts (<= 9) x (CLIP 2^k + ...) < 2^4 x 2^3 x 2^k = 2^(k + 7) must stay
# below max(T) / 2 = 2^127 (2^1023): k = 120 (1016).  tree_bound() of the actual planes is asserted against max(T) / 2 on the CPU.
M_K = {np.float32: dict(half=60, top=120, sub=-143), np.float64: dict(half=500, top=1016, sub=-1068)}


def _scaled(which, sign=1):
    def make(rng, model, H, W, dtype):
        k = sign * M_K[np.dtype(dtype).type][which]
        with np.errstate(under="ignore"):
            return np.ldexp(np.clip(rng.normal(0, 1, (len(model.filtersw), H, W)), -CLIP, CLIP), k).astype(dtype)
    return make


def _cancel(rng, model, H, W, dtype):
    """the children of the root in pairs: the second's planes are the exact negatives of the first's plus noise 2^-20 of their size"""
    k = M_K[np.dtype(dtype).type]["half"]
    r = np.ldexp(np.clip(rng.normal(0, 1, (len(model.filtersw), H, W)), -CLIP, CLIP), k).astype(dtype)
    kids = [p for p in range(1, model.nparts(0)) if model.parentid[0][p] == 0]
    for p, q in zip(kids[0::2], kids[1::2]):
        for j, f in enumerate(model.filterid[0][q]):
            src = model.filterid[0][p][j % len(model.filterid[0][p])]
            r[f] = (-r[src] + np.ldexp(np.clip(rng.normal(0, 1, (H, W)), -CLIP, CLIP), k - 20)).astype(dtype)
    return r


def _m_cases():
    out = [_case("M_k0_M4", "M", _model("M4", 400), _normal()),
           _case("M_half_up_M6", "M", _model("M6", 401), _scaled("half")),
           _case("M_half_down_M8_mode1", "M", _model("M8", 402), _scaled("half", -1), 1),
           _case("M_top_K10", "M", _model("K10", 403), _scaled("top")),
           _case("M_subnormal_M4", "M", _model("M4", 405), _scaled("sub")),
           _case("M_cancel_M8", "M", _model("M8", 406), _cancel)]
    # biases scaled with the responses: one model per type (Model.biasw is float: the double case scales to the float top as well —
    # the format cannot carry a bias of 1e300)
    m = _model("M6", 404)
    m.biasw = np.ldexp(m.biasw, M_K[np.float32]["top"] - 3).astype(np.float32)      # N(0, 0.1) 2^117: below CLIP 2^120
    out.append(_case("M_top_biasscaled_M6_mode2", "M", m, _scaled("top"), 2, dtypes=(np.float32,)))
    m = _model("M6", 404)
    m.biasw = np.ldexp(m.biasw, M_K[np.float32]["top"] - 3).astype(np.float32)
    out.append(_case("M_half_biasscaled_M6_mode2", "M", m, _scaled("half"), 2, dtypes=(np.float64,)))
    return out


# ---------------------------------------------------------------- Q: quadratics
def _scale_a(m, fx, fy=None):
    m.defw[:, 0] *= np.float32(fx)
    m.defw[:, 2] *= np.float32(fx if fy is None else fy)
    return m


def _set_b(m, f, W, rng):
    """|b| = f x a x W, random sign per row and axis: f = 0.5 moves the vertex of the parabola half a level away, 10 far outside"""
    s = rng.choice([-1.0, 1.0], (len(m.defw), 2))
    m.defw[:, 1] = (s[:, 0] * f * m.defw[:, 0] * W).astype(np.float32)
    m.defw[:, 3] = (s[:, 1] * f * m.defw[:, 2] * W).astype(np.float32)
    return m


def _q_cases(W):
    rng = np.random.default_rng(500)
    out = [_case("Q_a1e-6_M6", "Q", _scale_a(_model("M6", 500), 1e-6), _normal()),        # one cell wins the whole map
           _case("Q_a1e-3_M1", "Q", _scale_a(_model("M1", 501), 1e-3), _normal()),
           _case("Q_a1_b0_M4_mode2", "Q", _set_b(_model("M4", 502), 0.0, W, rng), _normal(), 2),
           _case("Q_a1e3_M4", "Q", _scale_a(_model("M4", 503), 1e3), _normal()),          # every cell its own maximum
           _case("Q_axy1e6_M8_mode1", "Q", _scale_a(_model("M8", 504), 1e-3, 1e3), _normal(), 1),
           _case("Q_ayx1e6_K10", "Q", _scale_a(_model("K10", 505), 1e3, 1e-3), _normal()),
           _case("Q_b0.5_M4", "Q", _set_b(_model("M4", 506), 0.5, W, rng), _normal()),
           _case("Q_b10_K10", "Q", _set_b(_model("K10", 507), 10.0, W, rng), _normal())]  # every arg-max at a border
    # a different deformation per mixture of one part: rows cycle through the scales and the |b| factors
    m = _model("M8", 508)
    for d in range(len(m.defw)):
        m.defw[d, 0] *= np.float32((1e-6, 1e-3, 1.0, 1e3)[d % 4])
        m.defw[d, 2] *= np.float32((1e3, 1.0, 1e-6, 1e-3)[d % 4])
        f = (0.0, 0.5, 10.0)[d % 3]
        m.defw[d, 1] = np.float32(f * m.defw[d, 0] * W * (-1) ** d)
        m.defw[d, 3] = np.float32(f * m.defw[d, 2] * W * (-1) ** (d // 2))
    out.append(_case("Q_permix_M8_mode2", "Q", m, _normal(), 2))
    # the same mix with dyadic numbers (quantised model: a in {1/32, 1/16}, responses and biases multiples of 1/4): a x 2^-3, 1, 2^3 and
    # |b| in {0, 4 a}: the quantum is 2^-8, a term at most 2^-1 x 27^2 < 2^9, a sum over six parts and two axes below 2^13 — 21 bits.
    # tests/test_dp_range_cpu.py::test_exact_cases_are_exact holds the float statement to the double one on these planes
    m = _model("M6", 509, quantised=True)
    for d in range(len(m.defw)):
        m.defw[d, 0] *= np.float32((2.0 ** -3, 1.0, 2.0 ** 3)[d % 3])
        m.defw[d, 2] *= np.float32((2.0 ** 3, 2.0 ** -3, 1.0)[d % 3])
        m.defw[d, 1] = np.float32((0.0, 4.0)[d % 2] * m.defw[d, 0] * (-1) ** (d // 2))
        m.defw[d, 3] = np.float32((4.0, 0.0)[d % 2] * m.defw[d, 2] * (-1) ** (d // 3))
    out.append(_case("Q_quant_permix_M6", "Q", m, _quant, 0, exact=True))
    # positive `a` (a negative deformation weight): pbd_create accepts it — the reference's stack algorithm runs as written
    m = _model("M4", 510)
    m.defw[::2, 0] *= np.float32(-1.0)
    m.defw[1::2, 2] *= np.float32(-1.0)
    out.append(_case("Q_positive_a_M4", "Q", m, _normal(), 0, positive_a=True))
    return out


# ---------------------------------------------------------------- A: anchors
def anchor_values(W):
    return [W - 1, -(W - 1), W, -W, 2 * W, -2 * W]


def _set_anchors(m, W, rng):
    """every deformation row one of +-(W - 1), +-W, +-2W on each axis, drawn so that all six occur on each axis, signs mixed between x and y,
    a different anchor per mixture"""
    n = len(m.defw)
    vals = np.asarray(anchor_values(W), np.int32)
    for axis in range(2):
        pick = np.concatenate([rng.permutation(6), rng.integers(0, 6, max(0, n - 6))])[:n]
        m.anchors[:, axis] = vals[rng.permutation(pick)]
    return m


def _a_cases(Ws, Wl):
    rng = np.random.default_rng(600)
    out = [_case("A_small_M6", "A", _set_anchors(_model("M6", 600), Ws, rng), _normal(), 0, anchor_W=Ws),
           _case("A_large_M4_mode1", "A", _set_anchors(_model("M4", 601), Wl, rng), _normal(), 1, anchor_W=Wl),
           _case("A_small_quant_M8", "A", _set_anchors(_model("M8", 602, quantised=True), Ws, rng), _quant, 0, exact=True, anchor_W=Ws),
           _case("A_large_quant_K10_mode2", "A", _set_anchors(_model("K10", 603, quantised=True), Wl, rng), _quant, 2, exact=True, anchor_W=Wl)]
    m = _model("M4", 604)       # every child 2W of the largest level away: every read-out of every level starts from the far end
    m.anchors[:, 0] = 2 * Wl
    m.anchors[:, 1] = -2 * Wl
    out.append(_case("A_all_2W_M4", "A", m, _normal(), 0))
    return out


LEVEL_W = (23, 4)            # cells across the largest and the smallest of FRAME's 21 levels (sbin 4, interval 10): asserted against the
#                              pyramid geometry by tests/test_dp_range_cpu.py and by every GPU test


def build_cases():
    """the anchors and |b| follow the levels' widths (LEVEL_W)"""
    Wl, Ws = LEVEL_W
    return _z_cases() + _m_cases() + _q_cases(Wl) + _a_cases(Ws, Wl)


def level_rng(case, level, dtype):
    return np.random.default_rng([sum(map(ord, case["name"])), level, np.dtype(dtype).itemsize])


def responses(case, geo, level, dtype):
    return case["resp"](level_rng(case, level, dtype), case["model"], int(geo["cell_h"][level]), int(geo["cell_w"][level]), dtype)
