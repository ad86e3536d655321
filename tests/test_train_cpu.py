"""partsbaseddetector_amd.train without a GPU: point_to_box against tests/train_ref.py's line-by-line pointtobox.m, exact in float64; the
calls train() makes, on recording fakes, against train.m:73-121 restated; the train() calls train_model() makes against trainmodel.m; the
new exports."""
import re
import os

import numpy as np
import pytest

import partsbaseddetector_amd as pkg
from partsbaseddetector_amd import capi
from partsbaseddetector_amd.train import point_to_box, train, train_model
from tests import train_ref

NONE, ONE, OPT = capi.PBD_MINE_NONE, capi.PBD_MINE_ONE, capi.PBD_MINE_OPT


# ---- point_to_box ------------------------------------------------------------------------------------------------------------------------
def _points(n, P, seed, spread=40.0):
    rng = np.random.default_rng(seed)
    return 100.0 + spread * rng.random((n, P, 2))


CHAIN6, STAR6 = [-1, 0, 1, 2, 3, 4], [-1, 0, 0, 0, 0, 0]
# P - 1 limbs: the 0.85 quantile sits at h = .85 (P - 2) — on an order statistic for 21 limbs (h = 17), between two otherwise
POINT_CASES = {
    "chain": (_points(7, 6, 1), CHAIN6),
    "star": (_points(7, 6, 2), STAR6),
    "mixed_tree_even_count": (_points(8, 5, 3), [-1, 0, 1, 1, 0]),
    "one_instance": (_points(1, 6, 4), CHAIN6),
    "two_parts": (_points(5, 2, 5), [-1, 0]),
    "on_an_order_statistic": (_points(4, 22, 6), [-1] + list(range(21))),
    "equal_limbs": (np.stack([np.stack([np.arange(5) * 10.0 * s + 50, np.full(5, 70.0)], axis=1) for s in (1.0, 2.0, 3.5)]), [-1, 0, 1, 2, 3]),
}


@pytest.mark.parametrize("name", sorted(POINT_CASES))
def test_point_to_box_is_pointtobox_m(name):
    pts, pa = POINT_CASES[name]
    got, want = point_to_box(pts, pa), train_ref.point_to_box(pts, pa)
    assert got.shape == want.shape == (len(pts), len(pa), 4) and got.dtype == np.float64
    assert got.tobytes() == want.tobytes(), np.abs(got - want).max()
    # square boxes centred on the points, one size per instance
    size = got[:, :, 2] - got[:, :, 0]
    assert np.allclose(size, size[:, :1]) and np.allclose(got[:, :, 3] - got[:, :, 1], size) and (size > 0).all()
    assert np.allclose((got[:, :, 0] + got[:, :, 2]) / 2, pts[:, :, 0])


def test_point_to_box_equal_limbs_is_the_limb():
    pts, pa = POINT_CASES["equal_limbs"]
    got = point_to_box(pts, pa)
    # every limb of an instance has one length and every ratio is 1: the box side is that length
    assert (got[:, 0, 2] - got[:, 0, 0]).tolist() == [10.0, 20.0, 35.0]


def test_point_to_box_refuses():
    with pytest.raises(ValueError):
        point_to_box(np.zeros((3, 4)), [-1, 0, 1, 2])
    with pytest.raises(ValueError):
        point_to_box(np.zeros((3, 4, 2)), [-1, 0, 1])


# ---- the order of train()'s calls ------------------------------------------------------------------------------------------------------
WARPED = [("p0", (1.0, 2.0, 30.0, 40.0)), ("p1", (5.0, 5.0, 50.0, 60.0)), ("p2", (3.0, 4.0, 33.0, 44.0))]
LATENT = [("p0", ((1, 2, 20, 20), (5, 6, 20, 20))), ("p1", ((3, 4, 20, 20), (7, 8, 20, 20)), (0, 1))]
NEG = ["n0", "n1", "n2"]
BOUNDS = (0.5, 0.75, 7)
TRAIN_CASES = {
    "warped": dict(positives=WARPED, warp=1, script=dict(written=1, mine=[(2, ONE), (0, NONE), (3, OPT)], bounds=BOUNDS, thresh=-0.3)),
    "latent": dict(positives=LATENT, warp=0, script=dict(written=1, mine=[(4, NONE), (1, ONE), (2, NONE)], bounds=BOUNDS, thresh=0.1 + 2 ** -30),
                   kw=dict(overlap=0.7, tol=.01, max_iter=50, seed=9)),
    # 2 positives, room for 6: the second image fills the cache (1 of its 4 records fits) and the third is never mined
    "cache_fills": dict(positives=LATENT, warp=0, capacity=6, script=dict(written=1, mine=[(3, NONE), (4, OPT), (1, NONE)], bounds=BOUNDS, thresh=1.5)),
    "two_rounds": dict(positives=WARPED, warp=1, script=dict(written=1, mine=[(1, NONE), (1, ONE), (1, NONE)] * 2, bounds=BOUNDS, thresh=2.0),
                       kw=dict(iter=2)),
    "no_negatives": dict(positives=WARPED, warp=2, negatives=[], script=dict(written=1, mine=[], bounds=BOUNDS, thresh=0.0)),
}


@pytest.mark.parametrize("name", sorted(TRAIN_CASES))
def test_train_makes_train_ms_calls(name):
    case = TRAIN_CASES[name]
    kw, neg = case.get("kw", {}), case.get("negatives", NEG)
    script = dict(case["script"])
    log, report, det, err = train_ref.run_fake(train, case["positives"], neg, case["warp"], script, case.get("capacity"), **kw)
    assert err is None
    cap = case.get("capacity") or 10 * 3 * len(case["positives"])
    want = train_ref.train_calls(case["positives"], neg, case["warp"], script, cap, **kw)
    assert want.count(("clear",)) == kw.get("iter", 1)            # (the fake reads the second half of the mining script in round two)
    assert log == want, [(i, a, b) for i, (a, b) in enumerate(zip(log, want)) if a != b][:3]
    assert len(report) == kw.get("iter", 1)
    r = report[-1]
    assert (r["lb"], r["ub"], r["passes"]) == (BOUNDS[0], BOUNDS[1], [BOUNDS[2]] * 2)
    assert r["thresh"] == float(np.float32(script["thresh"])) == det.model.thresh and det.model.interval == 10
    assert len(r["n"]) == len(r["sv"]) == 3 and r["n"][0] == len(case["positives"]) and r["n"][1] == r["n"][2] >= r["n"][0]
    if name == "cache_fills":
        assert r["mined"] == [(3, 3, NONE), (4, 1, OPT)] and r["n"] == [2, 6, 6] and ("mine", "n2", 3) not in log
    if name == "no_negatives":
        assert r["mined"] == [] and not any(c[0] == "mine" for c in log)


def test_train_restores_the_interval_and_threshold_when_mining_raises():
    script = dict(written=1, mine=[(2, NONE), (1, NONE), (1, NONE)], bounds=BOUNDS, thresh=0.5, fail_at=1)
    log, report, det, err = train_ref.run_fake(train, LATENT, NEG, 0, script)
    assert isinstance(err, RuntimeError) and report is None
    assert log == train_ref.train_calls(LATENT, NEG, 0, script, 60)
    assert log[-2:] == [("setThresh", 0.25), ("setInterval", 10)] and log[-3] == ("mine", "n1", 2)
    assert det.model.interval == 10 and det.model.thresh == 0.25


# ---- the order of train_model()'s calls --------------------------------------------------------------------------------------------------
def test_train_model_makes_trainmodel_ms_calls():
    n, parents, K = 9, [-1, 0, 0], [1, 2, 3]
    images = [f"im{i}" for i in range(n)]
    points = _points(n, 3, 11)
    idx = np.array([[0] * n, [0, 1, 0, 1, 1, 0, 0, 1, 0], [2, 0, 1, 1, 2, 0, 0, 1, 2]], np.int32)
    negatives = [f"neg{i}" for i in range(130)]
    calls, clustered = [], []

    def fake_cluster(deffeat, pa, k):
        clustered.append((np.asarray(deffeat).shape, list(pa), list(k)))
        return dict(idx=idx)

    def fake_train(model, positives, negs, warp, **kw):
        calls.append((model, positives, negs, warp, kw))
        return model, [dict(round=len(calls))]

    model, reports = train_model(list(zip(images, points)), negatives, K, parents, 4, tsize=(5, 5), _train=fake_train, _cluster=fake_cluster,
                                 max_iter=200)
    boxes = train_ref.point_to_box(points, parents)
    want = train_ref.trainmodel_calls(images, boxes, idx, K, negatives)
    assert clustered == [((3, n, 2), parents, K)]
    assert len(calls) == len(want) == sum(K) + 2
    for (what, nfilters, pos, neg, warp), (m, gpos, gneg, gwarp, kw) in zip(want, calls):
        assert kw == dict(max_iter=200) and gwarp == warp and gneg == neg, what
        assert len(m.filtersw) == nfilters and m.filter_sizes().tolist() == [[5, 5]] * nfilters, what
        assert [p[0] for p in gpos] == [p[0] for p in pos], what
        if warp:                                                   # the positives of that mixture, each reduced to the part's one box
            assert all(len(g) == 2 and np.asarray(g[1]).tobytes() == np.asarray(w[1], np.float64).tobytes() for g, w in zip(gpos, pos)), what
            assert len(gneg) == 100
        else:
            for i, (g, w) in enumerate(zip(gpos, pos)):
                tr = np.asarray(g[1])
                assert tr.shape == (3, 4) and tr.dtype == np.int32
                c = np.copysign(np.floor(np.abs(boxes[i]) + .5), boxes[i])
                assert tr.tolist() == np.stack([c[:, 0] - 1, c[:, 1] - 1, c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]], 1).astype(int).tolist()
                assert (len(g) == 3 and list(g[2]) == w[1]) if w[1] is not None else len(g) == 2, (what, i)
            assert len(gneg) == 130
    # the second joint round starts from the first one's result; the part rounds all from the one-filter init model
    assert calls[-1][0] is calls[-2][0] is model
    assert sorted(reports["parts"]) == [(p, k) for p in range(3) for k in range(K[p])]
    assert reports["final1"] == [dict(round=sum(K) + 1)] and reports["final"] == [dict(round=sum(K) + 2)]
    # the joint model's layout follows from K and the tree (build_model)
    assert len(model.filtersw) == 6 and len(model.defw) == 5 and len(model.biasw) == 1 + 2 * 1 + 3 * 1
    assert model.parentid == [parents]


# ---- exports -------------------------------------------------------------------------------------------------------------------------------
def test_exports():
    L = capi.lib()
    for name in ("pbd_set_interval", "pbd_get_interval", "pbd_qp_clear", "pbd_qp_positive_threshold"):
        assert name in capi.EXPORTS and hasattr(L, name)
    assert L.pbd_abi_version() == 5 == capi.PBD_ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))), "include", "pbd_c.h")).read()
    for decl in (r"int pbd_set_interval\(pbd_handle\* h, int interval\);", r"int pbd_get_interval\(const pbd_handle\* h\);",
                 r"int pbd_qp_clear\(pbd_qp\* qp\);", r"int pbd_qp_positive_threshold\(pbd_qp\* qp, double q, double\* thresh, int\* npos\);"):
        assert re.search(decl, header), decl
    assert "a handle's interval is fixed at pbd_create" not in header
    assert pkg.train is train and pkg.train_model is train_model and pkg.point_to_box is point_to_box
    for cls, names in ((capi.Handle, ("set_interval", "interval")), (capi.QpCache, ("clear", "positive_threshold")),
                       (pkg.PartsBasedDetector, ("setInterval", "interval"))):
        assert all(hasattr(cls, nm) for nm in names)
    # a NULL handle or cache is refused before anything is touched (no GPU needed)
    assert L.pbd_set_interval(None, 2) == capi.PBD_ERR_ARG and L.pbd_get_interval(None) == 0
    assert L.pbd_qp_clear(None) == capi.PBD_ERR_ARG and L.pbd_qp_positive_threshold(None, .05, None, None) == capi.PBD_ERR_ARG
