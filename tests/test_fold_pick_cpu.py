"""The mixture choice of a message (csrc/fold_pick.hpp) stated in numpy, against the oracle's DP.

The fold no longer stores Ik: k_backtrack and k_ik_fill pick it again from the children's kept distance-transformed scores with
fold_pick — `w[k] = sdt_k + bias(k)[m]`, start from -inf, strict `>` (the first maximum wins), K == 1 copies.  pick() below is that
function line for line, in both of its forms (K entries; register arrays of 8 entries whose tail repeats entry K - 1).  It must give
the oracle's Ik on every plane, and the two obvious other readings of "arg-max" must not."""
import numpy as np
import pytest

from partsbaseddetector_amd.model import make_tree_model_k
from tests import dp_ref
from tests.dp_range_cases import build_cases
from tests.mixture_models import level_responses

DTYPES = [np.float32, np.float64]
PARENTS, COUNTS = [-1, 0, 0, 1, 1, 2, 3], [2, 6, 1, 8, 2, 6, 1]      # K over L of parts 1..6: 6/2, 1/2, 8/6, 2/6, 6/1, 1/8
NPAD = 8                                                             # PBD_FOLD_MAXMIX


def pick(sd, bias_col, K, padded=False, how="gt"):
    """fold_pick<T, N>(sd, bias_col, K) on arrays: sd [>= K, ...] of T, bias_col [>= K] floats -> (value, index).
    padded: the N = 8 form (entries beyond K repeat entry K - 1, the loop runs to 8).  how: "gt" the function itself; "ge" and
    "from_right" are the two slips (>= for >; the maximum first, then the LAST index holding it)."""
    T = sd.dtype.type
    if padded:
        idx = np.minimum(np.arange(NPAD), K - 1)
        sd, bias_col = sd[idx], np.asarray(bias_col)[idx]
    n = NPAD if padded else K
    with np.errstate(invalid="ignore", over="ignore"):
        w0 = (sd[0] + T(bias_col[0])).astype(T)
        v = np.where(w0 > T(-np.inf), w0, T(-np.inf)).astype(T)
        bi = np.zeros(sd[0].shape, np.int32)
        ws = [w0]
        for k in range(1, n):
            wv = (sd[k] + T(bias_col[k])).astype(T)
            ws.append(wv)
            take = wv >= v if how == "ge" else wv > v
            bi = np.where(take, k, bi).astype(np.int32)
            v = np.where(take, wv, v)
        if how == "from_right":
            ws = np.stack(ws[:K])
            bi = (K - 1 - np.argmax((ws == v[None])[::-1], axis=0)).astype(np.int32)
    return (w0 if K == 1 else v), bi


def planes_by_pick(model, comp, maps, **kw):
    """Ik [planes, H, W] in the oracle's plane order, every plane by pick() from level_maps' kept scores"""
    fid, bid, par = model.filterid[comp], model.biasid[comp], model.parentid[comp]
    out = []
    for p in range(1, model.nparts(comp)):
        K = len(fid[p])
        sd = np.stack(maps["sdt"][p])
        for m in range(len(fid[par[p]])):
            out.append(pick(sd, [model.biasw[bid[p][k] + m] for k in range(K)], K, **kw)[1])
    return np.stack(out)


@pytest.fixture(scope="module")
def levels(orc):
    """(model, dtype, kind) -> (kept maps, oracle Ik) of one 11 x 9 level, computed once"""
    cache = {}

    def get(kind, dtype):
        key = (kind, np.dtype(dtype).name)
        if key not in cache:
            m = make_tree_model_k(PARENTS, COUNTS, seed=71, quantised=kind != "normal", shared=True if kind == "tied" else ())
            resp = level_responses(np.random.default_rng(72), m, 9, 11, dtype, kind)
            Ik = orc.dp_min_level(m.to_desc(), 0, resp, dtype=dtype)[2]
            cache[key] = (m, dp_ref.level_maps(orc, m, 0, resp, dtype=dtype), Ik)
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["normal", "quant", "tied"])
@pytest.mark.parametrize("padded", [False, True])
def test_pick_gives_the_oracles_ik(levels, kind, dtype, padded):
    """counts 1, 2, 6, 8 in one tree; 'quant': exact partial ties, 'tied': every mixture of a part ties (the first wins: Ik == 0)"""
    m, maps, Ik = levels(kind, dtype)
    assert sorted(set(COUNTS)) == [1, 2, 6, 8]
    got = planes_by_pick(m, 0, maps, padded=padded)
    np.testing.assert_array_equal(got, Ik)
    if kind == "tied":
        assert not got.any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("how", ["ge", "from_right"])
def test_the_other_readings_of_argmax_differ_on_ties(levels, how, dtype):
    for kind in ("quant", "tied"):
        m, maps, Ik = levels(kind, dtype)
        assert (planes_by_pick(m, 0, maps, how=how) != Ik).any(), (kind, how)
    m, maps, Ik = levels("normal", dtype)        # no ties: all readings agree — the difference above is the tie rule alone
    np.testing.assert_array_equal(planes_by_pick(m, 0, maps, how=how), Ik)


@pytest.mark.parametrize("dtype", DTYPES)
def test_signed_zero_planes(orc, dtype):
    """tests/dp_range_cases.py, family Z: planes and biases of zeros of both signs — -0.0 and +0.0 tie under `>`, the first wins"""
    for case in (c for c in build_cases() if c["family"] == "Z" and dtype in c["dtypes"]):
        m = case["model"]
        resp = case["resp"](np.random.default_rng(5), m, 7, 9, dtype)
        Ik = orc.dp_min_level(m.to_desc(), 0, resp, dtype=dtype)[2]
        maps = dp_ref.level_maps(orc, m, 0, resp, dtype=dtype)
        for padded in (False, True):
            if max(len(f) for f in m.filterid[0]) <= NPAD or not padded:
                np.testing.assert_array_equal(planes_by_pick(m, 0, maps, padded=padded), Ik, err_msg=case["name"])
    z = np.array([[-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0]], dtype)        # three mixtures, two cells
    v, bi = pick(z, [0.0, -0.0, -0.0], 3)
    assert not bi.any() and np.array_equal(np.signbit(v), np.signbit((z[0] + dtype(0.0))))
    assert pick(z, [0.0, -0.0, -0.0], 3, how="ge")[1].tolist() == [2, 2]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("padded", [False, True])
def test_infinities_and_nan(dtype, padded):
    """Math::reduceMax by hand (dp_ref._reduce is its statement): -inf planes never beat the -inf it starts from, a NaN is never
    taken and leaves -inf at k = 0; K == 1 copies its one weighted map, -inf and NaN included, index 0"""
    T = np.dtype(dtype).type
    inf, nan = T(np.inf), T(np.nan)
    cells = np.array([[-inf, -inf, 1.0, nan, -inf, 2.0],
                      [-inf, 3.0, 1.0, 0.5, nan, nan],
                      [-inf, 3.0, -inf, nan, -inf, 2.0]], dtype)
    bias = [0.25, -0.5, -0.5]
    v, bi = pick(cells, bias, 3, padded=padded)
    with np.errstate(invalid="ignore"):
        rv, ri = dp_ref._reduce([(cells[k] + T(bias[k])).astype(dtype) for k in range(3)], "gt")
    assert v.tobytes() == np.asarray(rv, dtype).tobytes() and bi.tolist() == ri.tolist()
    assert bi.tolist() == [0, 1, 0, 1, 0, 0] and v[0] == -inf and v[4] == -inf and v[3] == T(0.0)
    one = np.array([[-inf, nan, 1.5, -0.0]], dtype)
    v, bi = pick(one, [0.5], 1, padded=padded)
    assert not bi.any() and v[0] == -inf and np.isnan(v[1]) and v[2] == T(2.0)
    two = np.stack([one[0], one[0]])                                       # K = 2 on the same map: NaN leaves -inf, not NaN
    v, bi = pick(two, [0.5, 0.5], 2, padded=padded)
    assert not bi.any() and v[1] == -inf
