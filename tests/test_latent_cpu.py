"""Latent detection by definition (tests/latent_ref.py), checked on the CPU against a brute-force enumeration and against four slips.
The GPU tests (tests/test_gpu_latent.py) hold the library to this reference bit for bit."""
import itertools

import numpy as np
import pytest

from partsbaseddetector_amd.model import make_tree_model_k
from tests import dp_ref
from tests import latent_ref as LR
from tests.boundary_pad_ref import boxes_from_locs

# two small levels: (H, W, scale)
LEVELS = [(5, 6, 8.0), (3, 4, 12.0)]
SCALES = [s for _, _, s in LEVELS]


def _model(seed=1, sizes=None, parents=(-1, 0, 1), Ks=(2, 2, 2)):
    m = make_tree_model_k(list(parents), list(Ks), seed=seed, quantised=True)
    if sizes is not None:      # a size per filter: only the rows matter to the windows
        m.filtersw = [np.zeros((sizes[i % len(sizes)], sizes[i % len(sizes)] * m.flen), np.float32) for i in range(len(m.filtersw))]
    return m


def _resp(model, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return [(rng.integers(-8, 9, (len(model.filtersw), H, W)) * 0.25).astype(dtype) for H, W, _ in LEVELS]


def _truth(model, level, cells, mixture=0, pad=0):
    out = np.zeros((model.max_parts, 4), np.int32)
    out[:model.nparts(0)] = LR.boxes_of(model, 0, [(x, y, mixture) for x, y in cells], SCALES[level], pad, np.float32)
    return out


def _run(orc, model, resp, truth, overlap, **kw):
    return LR.detect(orc, model, SCALES, lambda l: resp[l], truth, overlap, correct_ptr=1, **kw)


@pytest.mark.parametrize("mix", [None, (-1, 1, 0)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mask_is_the_constraint(orc, seed, mix):
    """3 parts, K = 2, planes of 5 x 6 and 3 x 4 cells, dyadic numbers (every sum exact in float): the reference's score is the largest
    float64 re-score (dp_ref.rescore) over ALL configurations whose every part is admissible, and its own configuration is one of them
    and re-scores to that score."""
    m = _model(seed)
    resp = _resp(m, 10 + seed)
    truth = _truth(m, 0, [(2, 2), (3, 2), (3, 3)])
    overlap = 0.3
    got = _run(orc, m, resp, truth, overlap, mix=mix)
    best, nconf = None, 0
    for l, (H, W, s) in enumerate(LEVELS):
        per_part = []
        for p in range(3):
            opts = []
            for k in range(2):
                if mix is not None and mix[p] >= 0 and k != mix[p]:
                    continue
                adm = LR.admissible(m, 0, p, k, H, W, s, 0, np.float32, truth[p], overlap)
                opts += [(x, y, k) for y in range(H) for x in range(W) if adm[y, x]]
            per_part.append(opts)
        for cfg in itertools.product(*per_part):
            nconf += 1
            sc, _ = dp_ref.rescore(m, 0, resp[l], np.asarray(cfg))
            if best is None or sc > best:
                best = sc
    assert nconf > 500
    assert got["found"] == 1 and float(got["score"]) == best
    sc, _ = dp_ref.rescore(m, 0, resp[got["level"]], got["locs"])
    assert sc == best
    H, W, s = LEVELS[got["level"]]
    for p, (x, y, k) in enumerate(got["locs"]):
        assert LR.admissible(m, 0, p, int(k), H, W, s, 0, np.float32, truth[p], overlap)[y, x]
        assert mix is None or mix[p] < 0 or k == mix[p]
    # the boxes are the back-tracking's (tests/boundary_pad_ref.py states the same rule)
    want = boxes_from_locs(m, 0, got["locs"][None], s, 0)[0][:3]
    np.testing.assert_array_equal(got["boxes"], want)


def test_own_boxes_overlap_exactly_one(orc):
    """a record's own boxes as truth: overlap 1.0 at its cells, for uniform and mixed sizes, with and without padding"""
    for sizes, pad in ((None, 0), ((3, 5, 7), 0), ((3, 5, 7), 3)):
        m = _model(4, sizes)
        resp = _resp(m, 20)
        got = _run(orc, m, resp, _truth(m, 0, [(2, 2), (3, 2), (3, 3)], pad=pad), 0.2, pad=pad)
        assert got["found"] == 1
        H, W, s = LEVELS[got["level"]]
        for p, (x, y, k) in enumerate(got["locs"]):
            ov = LR.overlap_grid(*LR.window(m, 0, p, int(k), H, W, s, pad, np.float32), got["boxes"][p])
            assert ov[y, x] == 1.0
        again = _run(orc, m, resp, np.vstack([got["boxes"], np.zeros((m.max_parts - 3, 4), np.int32)]), 0.999, pad=pad)
        assert again["found"] == 1 and again["level"] == got["level"]
        np.testing.assert_array_equal(again["locs"], got["locs"])


def test_all_inadmissible_truth_finds_nothing(orc):
    m = _model(5)
    truth = np.tile(np.array([100000, 100000, 10, 10], np.int32), (m.max_parts, 1))
    got = _run(orc, m, _resp(m, 30), truth, 0.0)
    assert got["found"] == 0 and not got["admissible"].any()
    # one part without an admissible cell is enough
    truth = _truth(m, 0, [(2, 2), (3, 2), (3, 3)])
    truth[2] = (100000, 100000, 10, 10)
    got = _run(orc, m, _resp(m, 30), truth, 0.3)
    assert got["found"] == 0


def _differs(a, b):
    if a["found"] != b["found"]:
        return True
    return a["found"] == 1 and (a["level"] != b["level"] or a["score"] != b["score"] or not np.array_equal(a["locs"], b["locs"]))


def test_each_slip_changes_a_result(orc):
    # missing + 1: a 40-pixel window against itself overlaps 39^2 / (2 40^2 - 39^2) = 0.906 < 0.95 instead of 1
    m = _model(6)
    resp = _resp(m, 40)
    truth = _truth(m, 0, [(2, 2), (3, 2), (3, 3)])
    good = _run(orc, m, resp, truth, 0.95)
    assert good["found"] == 1 and _run(orc, m, resp, truth, 0.95, slip="no_plus1")["found"] == 0
    # >= for >: at overlap 0 a window that misses the box (overlap exactly 0) becomes admissible; the best pose sits there
    truth = _truth(m, 0, [(0, 0), (0, 0), (0, 0)])
    far = [r.copy() for r in resp]
    for f in range(len(m.filtersw)):
        far[0][f, 4, 5] += 64.0
    good = _run(orc, m, far, truth, 0.0)
    bad = _run(orc, m, far, truth, 0.0, slip="ge")
    assert good["found"] == 1 and tuple(good["locs"][0][:2]) != (5, 4)
    assert bad["found"] == 1 and bad["level"] == 0 and tuple(bad["locs"][0][:2]) == (5, 4) and _differs(good, bad)
    # the size of mixture 0 for every mixture: 3-row windows never cover 0.9 of a 7-row box
    ms = _model(7, sizes=(3, 7))                # filter 2 p + k: mixture 0 has 3 rows, mixture 1 has 7
    resp = _resp(ms, 41)
    truth = _truth(ms, 0, [(2, 2), (3, 2), (3, 3)], mixture=1)
    good = _run(orc, ms, resp, truth, 0.9)
    assert good["found"] == 1 and all(int(k) == 1 for k in good["locs"][:, 2])
    assert _run(orc, ms, resp, truth, 0.9, slip="size_mix0")["found"] == 0
    # org without the pad: the admissible cell moves by the padding
    truth = _truth(m, 0, [(4, 3), (4, 3), (4, 3)], pad=2)
    resp = _resp(m, 42)
    good = _run(orc, m, resp, truth, 0.9, pad=2)
    bad = _run(orc, m, resp, truth, 0.9, pad=2, slip="org_nopad")
    assert good["found"] == 1 and tuple(good["locs"][0][:2]) == (4, 3)
    assert _differs(good, bad)
