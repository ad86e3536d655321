"""Models whose parts have different mixture counts, on the host: the oracle's DP (orc.dp_min_level) against the independent
numpy message passing of tests/dp_ref.py, with L != K in every combination the GPU tests use; and the numpy restatement of
src/nms.cpp (tests/nms_ref.py) against orc.nms_map on planes full of ties."""
import numpy as np
import pytest

from partsbaseddetector_amd.model import make_tree_model, make_tree_model_k
from tests import dp_ref, nms_ref
from tests.mixture_models import HET, het_model, level_responses, two_profiles


def test_make_tree_model_k_layout():
    m = make_tree_model_k([-1, 0, 0, 1], [1, 3, 6, 2], seed=4, shared=[2])
    assert [len(f) for f in m.filterid[0]] == [1, 3, 6, 2]
    assert sorted(sum(m.filterid[0], [])) == list(range(12))
    # child p, parent count L: bias(k)[m] = biasw[base + k*L + m], one block of L x K per child; one def row per child mixture
    assert m.biasid[0][1] == [1, 2, 3]                       # L = 1, K = 3
    assert m.biasid[0][2] == [4] * 6                          # shared: one bias row (of L = 1) for all six mixtures
    assert m.biasid[0][3] == [5, 5 + 3] and len(m.biasw) == 5 + 3 * 2   # L = 3, K = 2
    assert m.defid[0][1] == [0, 1, 2] and m.defid[0][2] == [3] * 6 and m.defid[0][3] == [4, 5] and len(m.defw) == 6
    s2 = make_tree_model_k([-1, 0, 1], [2, 4, 3], seed=4, shared=True)
    assert s2.biasid[0][2] == [1 + 2] * 3 and np.all(s2.biasw[3:7] == s2.biasw[3])   # L = 4 entries, all equal
    # one count for every part: make_tree_model is untouched
    a, b = make_tree_model([-1, 0, 1, 1, 0], 3, seed=5), make_tree_model([-1, 0, 1, 1, 0], 3, seed=5)
    assert all(np.array_equal(x, y) for x, y in zip(a.filtersw, b.filtersw)) and a.biasid == b.biasid


def _check_level(orc, model, resp, dtype):
    desc = model.to_desc()
    for c in range(model.ncomponents):
        Ix, Iy, Ik, rv, ri = orc.dp_min_level(desc, c, resp, dtype=dtype)
        maps = dp_ref.level_maps(orc, model, c, resp, dtype=dtype)
        np.testing.assert_array_equal(maps["rootv"].view(np.uint8), rv.view(np.uint8))
        np.testing.assert_array_equal(maps["rooti"], ri)
        rx, ry, rk = dp_ref.pointer_planes(model, c, maps)
        assert rk.shape == Ik.shape
        np.testing.assert_array_equal(rk, Ik); np.testing.assert_array_equal(rx, Ix); np.testing.assert_array_equal(ry, Iy)
    return Ik, ri


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(HET) + ["two_profiles"])
def test_oracle_dp_matches_dp_ref_heterogeneous(orc, name, dtype):
    m = two_profiles() if name == "two_profiles" else het_model(name)
    rng = np.random.default_rng(3)
    for H, W, kind in ((13, 17, "normal"), (1, 9, "normal"), (11, 8, "quant")):
        _check_level(orc, m, level_responses(rng, m, H, W, dtype, kind), dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_dp_exact_ties_take_the_first_mixture(orc, dtype):
    """Every mixture of a part shares its deformation, its bias row (constant) and its response: all K weighted maps of every
    reduce and all root mixtures tie exactly, and the first maximum (mixture 0) is taken everywhere."""
    rng = np.random.default_rng(5)
    for name in ("siblings_1_to_8", "L6_child_K1", "k10_among_small"):
        m = het_model(name, shared=True, quantised=True)
        Ik, ri = _check_level(orc, m, level_responses(rng, m, 12, 15, dtype, "tied"), dtype)
        assert not Ik.any() and not ri.any()


@pytest.mark.parametrize("M,N,sz", [(1, 1, 1), (1, 40, 2), (37, 1, 3), (5, 7, 10), (16, 16, 1), (30, 41, 2), (29, 33, 5)])
def test_nms_ref_matches_oracle(orc, M, N, sz):
    rng = np.random.default_rng(M * 100 + N)
    yy, xx = np.mgrid[0:M, 0:N]
    planes = [np.zeros((M, N)), np.full((M, N), -1.5), np.full((M, N), 2.0), rng.integers(0, 3, (M, N)) * 0.5,
              (xx + yy) * 0.25, -(xx * 0.5), rng.normal(size=(M, N))]
    for a in planes:
        a = a.astype(np.float32)
        np.testing.assert_array_equal(orc.nms_map(a, sz), nms_ref.nms_map(a, sz))
