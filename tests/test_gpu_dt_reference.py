"""The distance transform on the GPU against the COMPILED reference, and its input domain.

The range cases of tests/dt_path_cases.py (RANGE_CASES, fold_f32_big: values and curvatures out to the ends of the float range, all
finite) are members of ALL_CASES and run through tests/test_gpu_dt_paths.py::test_dt_path_case: the product library against the
oracle, the probe build in a child process, scan_flags equal to the host replay's.  Here:
(a) pbd_dt2d / pbd_dt2d_f64 on the recorded 16 x 72 subset against tests/golden/ref_dt_v1.npz — the compiled reference's outputs, not
    the oracle's — and against oracle/_ref/libref_dt.so itself where it was built;
(b) the domain: every entry point that takes scores or weights from the host refuses a non-finite one with PBD_ERR_ARG before
    anything is launched, and the handle is as good as new afterwards (pbd_create's refusal of non-finite weights happens before a device
    is looked for: tests/test_dt_reference_cpu.py).  Nothing here hands a non-finite map to a kernel, nor a finite one whose x pass overflows."""
import numpy as np
import pytest

from oracle import ref_dt
from tests import dt_path_cases as dc

pytestmark = pytest.mark.gpu
BAD = [np.nan, np.inf, -np.inf]
Q = (*dc._QA, 1, -2)


_same = dc.assert_same


@pytest.fixture(scope="module")
def fixture_npz():
    return np.load(dc.REF_DT_FIXTURE)


@pytest.fixture(scope="module")
def handles(gpu_required):
    from partsbaseddetector_amd import capi
    from partsbaseddetector_amd.model import make_tree_model
    hs = {np.dtype(dt): capi.Handle(make_tree_model([-1, 0], 1, seed=1), conv_mode=capi.PBD_CONV_EXACT, dtype=dt) for dt in (np.float32, np.float64)}
    yield hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("name", [c["name"] for c in dc.RECORDED_CASES])
def test_recorded_subset_matches_the_compiled_reference(handles, fixture_npz, name):
    case = next(c for c in dc.RECORDED_CASES if c["name"] == name)
    a = case["make"]()
    got = handles[case["dtype"]].dt2d(a, *case["q"])
    _same(got, dc.recorded(fixture_npz, name), name + " against the record")
    if ref_dt.available():
        _same(got, ref_dt.dt2d(a, *case["q"], dtype=case["dtype"]), name + " against the binary")


def _refused(fn, *args):
    from partsbaseddetector_amd import capi
    with pytest.raises(capi.PbdError) as e:
        fn(*args)
    assert e.value.code == capi.PBD_ERR_ARG, e.value
    return str(e.value)


def _finite_check(h, dtype):
    """the same handle still computes a finite map bit-identically to the record"""
    fix = np.load(dc.REF_DT_FIXTURE)
    name = "rec_smooth_f32" if dtype == np.float32 else "rec_smooth_f64"
    case = next(c for c in dc.RECORDED_CASES if c["name"] == name)
    _same(h.dt2d(case["make"](), *case["q"]), dc.recorded(fix, name), "after a refusal")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dt2d_refuses_nonfinite_maps_and_quadratics(handles, dtype):
    h = handles[np.dtype(dtype)]
    base = np.random.default_rng(7).normal(0, 1.5, (16, 72)).astype(dtype)
    for bad in BAD:
        a = base.copy()
        a[9, 41] = bad                                  # ONE non-finite value
        assert "non-finite" in _refused(h.dt2d, a, *Q)
        for i in range(4):
            q = list(Q)
            q[i] = bad
            _refused(h.dt2d, base, *q)
    _finite_check(h, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_set_level_response_and_features_refuse_nonfinite_maps(gpu_required, orc, dtype):
    from partsbaseddetector_amd import capi
    from partsbaseddetector_amd.model import make_tree_model
    model = make_tree_model([-1, 0, 0], 2, seed=3)
    h = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype)
    try:
        h.begin_frame(160, 120, 3)
        g = h._geo
        rng = np.random.default_rng(11)
        nf = len(model.filtersw)
        resp = [np.round(rng.normal(0, 1.5, (nf, g["cell_h"][l], g["cell_w"][l]))).astype(dtype) for l in range(g["nlevels"])]
        for l in range(g["nlevels"]):
            for n in range(nf):
                h.set_level_response(l, n, resp[l][n])
        for bad in BAD:
            r = resp[0][1].copy()
            r[r.shape[0] // 2, r.shape[1] // 3] = bad
            assert "non-finite" in _refused(h.set_level_response, 0, 1, r)
            f = np.zeros((g["cell_h"][0], g["cell_w"][0], 32), dtype)
            f[1, 2, 3] = bad
            assert "non-finite" in _refused(h.set_level_features, 0, f)
        # the refused planes were not uploaded: the DP runs on the finite ones, bit-identical to the oracle
        h.dp_min()
        desc = model.to_desc()
        for l in range(g["nlevels"]):
            rv, ri = orc.dp_min_level(desc, 0, resp[l], dtype=dtype)[3:]
            grv, gri = h.root(l, 0)
            assert np.array_equal(grv.view(np.uint8), rv.view(np.uint8)) and np.array_equal(gri, ri), l
        _finite_check(h, dtype)
    finally:
        h.close()
