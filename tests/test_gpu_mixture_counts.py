"""The DP stages on models whose parts have different mixture counts, and on exact score ties, against the oracle bit for bit.

* Mixture counts per part (src/DynamicProgram.cpp:99-100: nmixtures of the part, pnmixtures of its parent): the fold and the
  reduce handle L != K with clamped, unpredicated copies (entries beyond K repeat mixture K - 1, columns beyond L repeat L - 1),
  so a stride or clamp that used the child's count where the parent's belongs passes every model with one count for all parts.
* Ties: Math::reduceMax takes the first maximum (strict >, K == 1 copies), argmin keeps roots strictly above the threshold
  (:208), the score-map NMS keeps a block maximum strictly above its neighbourhood (src/nms.cpp:84-129).  Quantised responses and
  flat frames (zero HOG features: equal responses over whole regions) make those rules decide."""
import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_tree_model_k
from tests import dp_ref, nms_ref
from tests.mixture_models import HET, het_model, level_responses, two_profiles
from tests.util import assert_candidates_equal, thresh_from_oracle

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _model(name, **kw):
    return two_profiles(**kw) if name == "two_profiles" else het_model(name, **kw)


def _dp_case(orc, model, w, h, seed, dtype, kind="normal", dp_mode=0, plain=False, tied=False):
    """Injected responses -> pbd_dp_min -> every Ix / Iy / Ik plane and the root tables against orc.dp_min_level, bit for bit.
    plain: also against the first-maximum statement of tests/dp_ref.py.  tied: every reduce ties, so Ik == 0 and rooti == 0."""
    hd = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, dp_mode=dp_mode)
    hd.begin_frame(w, h, 3)
    g = hd._geo
    rng = np.random.default_rng(seed)
    desc = model.to_desc()
    resp = [level_responses(rng, model, g["cell_h"][l], g["cell_w"][l], dtype, kind) for l in range(g["nlevels"])]
    for l in range(g["nlevels"]):
        for n in range(len(model.filtersw)):
            hd.set_level_response(l, n, resp[l][n])
    hd.dp_min()
    for l in range(g["nlevels"]):
        for c in range(model.ncomponents):
            Ix, Iy, Ik, rv, ri = orc.dp_min_level(desc, c, resp[l], dtype=dtype)
            grv, gri = hd.root(l, c)
            np.testing.assert_array_equal(_bits(grv), _bits(rv), err_msg=f"rootv level {l} comp {c}")
            np.testing.assert_array_equal(gri, ri, err_msg=f"rooti level {l} comp {c}")
            if plain:
                maps = dp_ref.level_maps(orc, model, c, resp[l], dtype=dtype)
                rx, ry, rk = dp_ref.pointer_planes(model, c, maps)
                np.testing.assert_array_equal(gri, maps["rooti"])
            if tied:
                assert not gri.any(), f"rooti != 0 on all-tied root mixtures, level {l} comp {c}"
            plane = 0
            for p in range(1, model.nparts(c)):
                L = len(model.filterid[c][model.parentid[c][p]])
                for pm in range(L):
                    gx, gy, gk = hd.dp_pointers(l, c, p, pm)
                    where = f"level {l} comp {c} part {p} parent mixture {pm}"
                    np.testing.assert_array_equal(gk, Ik[plane], err_msg="Ik " + where)
                    np.testing.assert_array_equal(gx, Ix[plane], err_msg="Ix " + where)
                    np.testing.assert_array_equal(gy, Iy[plane], err_msg="Iy " + where)
                    if plain:
                        np.testing.assert_array_equal(gk, rk[plane], err_msg="Ik (first maximum) " + where)
                    if tied:
                        assert not gk.any(), "Ik != 0 on all-tied mixtures, " + where
                    plane += 1
    hd.close()


# ---------------------------------------------------------------- a mixture count per part: DynamicProgram::min
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(HET) + ["two_profiles"])
def test_dp_min_mixture_count_per_part(gpu_required, orc, name, dtype):
    _dp_case(orc, _model(name), 100, 80, 11, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["foldmix5", "L6_child_K1", "two_profiles"])
def test_dp_min_mixture_count_per_part_three_kernel(gpu_required, orc, name, dtype):
    """dp_mode = 1: the x pass / y pass / k_reduce structure on the same models."""
    _dp_case(orc, _model(name), 100, 80, 12, dtype, dp_mode=1)


# ---------------------------------------------------------------- a mixture count per part: detect() end to end
def _thresh(orc, model, im, dtype, q=99.0):
    if dtype == np.float32:
        return thresh_from_oracle(orc, model, im, q)
    model.thresh = -1e30
    fr = orc.detect(model, im, capacity=1, keep=True, dtype=dtype)[4]
    v = np.concatenate([fr.root(l)[0].ravel() for l in range(fr.nlevels)])
    fr.free()
    return float(np.float32(np.percentile(v, q)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["root1_children_many", "L6_child_K1", "siblings_1_to_8", "foldmix7", "k10_among_small", "two_profiles"])
def test_detect_mixture_count_per_part_exact(gpu_required, orc, name, dtype):
    m = _model(name)
    im = make_image(4, 200, 150)
    m.thresh = _thresh(orc, m, im, dtype)
    ref = orc.detect(m, im, dtype=dtype)[:3]
    assert len(ref[0]) > 5
    hd = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype)
    assert_candidates_equal(hd.detect(im), ref)
    hd.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_detect_mixture_count_per_part_sized_bank(gpu_required, orc, dtype):
    """pbd_create_sized with filters of several sizes inside one part: a part's box is the size of the filter of the mixture
    it chose (include/Parts.hpp xsize(m)), read from a table whose entries beyond the part's K repeat its last mixture."""
    from tests.test_gpu_mixed_bank import Composed, _set_thresh
    from partsbaseddetector_amd.model import _filters
    m = make_tree_model_k([-1, 0, 1, 1, 0], [1, 4, 2, 6, 3], seed=21)
    rng = np.random.default_rng(22)
    sizes = {(0, 0): (7, 7), (1, 0): (3, 5), (1, 2): (6, 4), (1, 3): (3, 3), (3, 5): (8, 6), (3, 1): (4, 4), (4, 2): (6, 6)}
    for (p, k), (kh, kw) in sizes.items():
        m.filtersw[m.filterid[0][p][k]] = _filters(rng, 1, kh, kw, m.flen)[0]
    assert not m.is_uniform()
    im = make_image(5, 320, 240)
    comp = Composed(orc, m, im, dtype)
    _set_thresh(comp, 99.0)
    ref = comp.candidates()
    assert len(ref[0]) > 5
    h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype)
    assert h.fsize is not None
    assert_candidates_equal(h.detect(im), ref)
    h.close()


def test_detect_mixture_count_per_part_batch_graph(gpu_required, orc):
    m = two_profiles()
    frames = [make_image(20 + i, 200, 150) for i in range(3)]
    m.thresh = thresh_from_oracle(orc, m, frames[0], 99.0)
    refs = [orc.detect(m, f)[:3] for f in frames]
    h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, graph=1)
    for _ in range(3):          # capture, then replays
        for got, ref in zip(h.detect_batch(frames), refs):
            assert_candidates_equal(got, ref)
    h.close()


def test_detect_mixture_count_per_part_default_bank_classified(gpu_required, orc):
    """PBD_CONV_AUTO (the split-product bank for float handles from 16 filters on) on a two-component model with different
    count profiles: every part-location difference from the oracle is a classified near-tie, none a bug."""
    from tests.test_gpu_parity import _classified_compare
    m = two_profiles()
    assert len(m.filtersw) >= 16
    im = make_image(7, 320, 240)
    m.thresh = thresh_from_oracle(orc, m, im, 99.0)
    rh, rb, rl, _, fr = orc.detect(m, im, keep=True)
    hd = capi.Handle(m)
    got = hd.detect(im)
    n, flips, ties, bugs, worst = _classified_compare(orc, m, im, hd, got, (rh, rb, rl), fr)
    hd.close(); fr.free()
    assert len(rh) > 20 and n >= 0.9 * len(rh) and not bugs, (len(rh), n, flips, ties, bugs)


# ---------------------------------------------------------------- exact ties in the DP
TIE_CASES = {   # name: (parents, counts, dp_mode) — fold widths M = 1, 4, 6, 8, the three-kernel structure, K > 8
    "fold_M1": ([-1, 0, 1, 1, 0], [1, 1, 1, 1, 1], 0),
    "fold_M4": ([-1, 0, 1, 1, 0], [4, 2, 4, 3, 1], 0),
    "fold_M6": ([-1, 0, 1, 2, 0, 4], [6, 1, 6, 2, 5, 3], 0),
    "fold_M8": ([-1, 0, 0, 0, 0, 0, 0, 0, 0], [2, 1, 2, 3, 4, 5, 6, 7, 8], 0),
    "three_kernel": ([-1, 0, 0, 0, 0, 0, 0, 0, 0], [2, 1, 2, 3, 4, 5, 6, 7, 8], 1),
    "k10": ([-1, 0, 1, 0], [3, 10, 4, 2], 0),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(TIE_CASES))
def test_dp_min_exact_ties(gpu_required, orc, case, dtype):
    """Quantised responses (multiples of 1/4), biases and deformations: sums are exact, so weighted maps tie.
      * all tied: every mixture of a part shares its response, deformation and (constant) bias row — the first mixture is
        taken everywhere, Ik == 0 and rooti == 0;
      * partly tied: independent quantised responses — Ik is the first maximum of the weighted maps (tests/dp_ref.py)."""
    parents, Ks, dp_mode = TIE_CASES[case]
    seed = 40 + list(TIE_CASES).index(case)
    tied = make_tree_model_k(parents, Ks, seed=seed, shared=True, quantised=True)
    _dp_case(orc, tied, 90, 70, seed, dtype, kind="tied", dp_mode=dp_mode, plain=True, tied=True)
    part = make_tree_model_k(parents, Ks, seed=seed + 100, quantised=True)
    _dp_case(orc, part, 90, 70, seed + 1, dtype, kind="quant", dp_mode=dp_mode, plain=True)


# ---------------------------------------------------------------- exact ties end to end: flat and letterboxed frames
def _flat_model():
    """Quantised, two parts whose mixtures tie, every filter weight <= 0: HOG features are >= 0 and exactly 0 on flat regions,
    so the root score is largest — and one exact float value — on every root whose whole tree sits on flat content."""
    m = make_tree_model_k([-1, 0, 1, 1, 0], [2, 3, 1, 4, 2], seed=31, shared=[1, 3], quantised=True, interval=5)
    m.filtersw = [-np.abs(f) for f in m.filtersw]
    return m


def _frame(kind):
    if kind == "black":
        return np.zeros((120, 160, 3), np.uint8)
    if kind == "grey":
        return np.full((120, 160, 3), 128, np.uint8)
    if kind == "letterbox":          # 640 x 360 content, bars top and bottom
        im = np.zeros((480, 640, 3), np.uint8)
        im[60:420] = make_image(2, 640, 360)
        return im
    im = np.full((480, 640, 3), 30, np.uint8)   # pillarbox: 480 x 480 content, grey bars left and right
    im[:, 80:560] = make_image(3, 480, 480)
    return im


FRAMES = ["black", "grey", "letterbox", "pillarbox"]
CAP = 16384


def _plateau(orc, m, im, dtype):
    """(plateau value, number of roots on it, Frame with the roots) — the largest root score, which flat content attains exactly."""
    m.thresh = -1e30
    fr = orc.detect(m, im, capacity=1, keep=True, dtype=dtype)[4]
    v = np.concatenate([fr.root(l)[0].ravel() for l in range(fr.nlevels)])
    top = v.max()
    assert float(np.float32(top)) == float(top)      # Model::thresh is a float: the plateau must be one
    return float(top), int((v == top).sum()), fr


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frame", FRAMES)
def test_flat_frames_threshold_on_the_plateau(gpu_required, orc, frame, dtype):
    m, im = _flat_model(), _frame(frame)
    top, n_top, fr = _plateau(orc, m, im, dtype)
    fr.free()
    assert n_top >= 100
    # the threshold equal to an attained score: argmin keeps roots strictly above it (:208) — none here
    m.thresh = top
    ref = orc.detect(m, im, capacity=CAP, dtype=dtype)[:3]
    assert len(ref[0]) == 0
    h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, max_candidates=CAP)
    assert_candidates_equal(h.detect(im, capacity=CAP), ref)
    h.close()
    # one float below: every root on the plateau, all with one score
    m.thresh = float(np.nextafter(np.float32(top), np.float32(-np.inf)))
    ref = orc.detect(m, im, capacity=CAP, dtype=dtype)[:3]
    assert len(ref[0]) == n_top and np.all(ref[0]["score"] == np.float32(top))
    h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, max_candidates=CAP)
    assert_candidates_equal(h.detect(im, capacity=CAP), ref)
    h.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sz", [1, 2, 5])
def test_flat_frames_device_nms_on_plateaus(gpu_required, orc, sz, dtype):
    """nms_sz > 0 (k_nms_roots<T>, f64 included) on root planes with plateaus: the oracle's candidates whose root the plain
    restatement of src/nms.cpp (tests/nms_ref.py) keeps on the oracle's own root plane of the same T."""
    m = _flat_model()
    kept = 0
    for frame in ("black", "letterbox"):
        im = _frame(frame)
        top, _, fr = _plateau(orc, m, im, dtype)
        m.thresh = float(np.nextafter(np.float32(top), np.float32(-np.inf))) if frame == "black" else \
            float(np.float32(np.percentile(np.concatenate([fr.root(l)[0].ravel() for l in range(fr.nlevels)]), 90.0)))
        rh, rb, rl = orc.detect(m, im, capacity=CAP, dtype=dtype)[:3]
        masks = {(l, c): nms_ref.nms_map(fr.root(l)[0][c], sz) for l in range(fr.nlevels) for c in range(m.ncomponents)
                 if fr.root(l)[0][c].size}
        fr.free()
        keep = np.array([masks[(int(r["level"]), int(r["component"]))][int(lc[0][1]), int(lc[0][0])] != 0 for r, lc in zip(rh, rl)], bool)
        kept += int(keep.sum())
        h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, nms_sz=sz, max_candidates=CAP)
        assert_candidates_equal(h.detect(im, capacity=CAP), (rh[keep], rb[keep], rl[keep]))
        h.close()
    assert kept > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_frames_sort_and_nms_of_equal_scores(gpu_required, orc, dtype):
    """Candidate::sort and sort + nonMaximaSuppression on the device, on candidates that all have one score (black frame) or
    hundreds of equal scores among others (letterbox): the oracle's stable order and its painted-box suppression."""
    m = _flat_model()
    for frame in ("black", "letterbox"):
        im = _frame(frame)
        hgt, w = im.shape[:2]
        top, _, fr = _plateau(orc, m, im, dtype)
        m.thresh = float(np.nextafter(np.float32(top), np.float32(-np.inf))) if frame == "black" else \
            float(np.float32(np.percentile(np.concatenate([fr.root(l)[0].ravel() for l in range(fr.nlevels)]), 90.0)))
        fr.free()
        raw = orc.detect(m, im, capacity=CAP, dtype=dtype)[:3]
        assert 0 < len(raw[0]) < CAP
        for mode, ov in ((capi.PBD_CAND_SORT, 0.0), (capi.PBD_CAND_SORT_NMS, 0.0), (capi.PBD_CAND_SORT_NMS, 0.3)):
            exp = orc.candidates_sort(*raw)
            if mode == capi.PBD_CAND_SORT_NMS:
                exp = orc.candidates_nms(*exp, w, hgt, ov)
            h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, max_candidates=CAP, cand_filter=(mode, ov))
            got = h.detect(im, capacity=CAP)
            h.close()
            assert len(got[0]) == len(exp[0]), (frame, mode, ov, len(got[0]), len(exp[0]))
            assert got[0].tobytes() == np.ascontiguousarray(exp[0]).tobytes(), (frame, mode, ov)
            assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]), (frame, mode, ov)


# ---------------------------------------------------------------- pbd_nms_map against src/nms.cpp
@pytest.fixture(scope="module")
def small(gpu_required):
    h = capi.Handle(het_model("foldmix3"), conv_mode=capi.PBD_CONV_EXACT)
    yield h
    h.close()


@pytest.mark.parametrize("M,N,sz", [(1, 1, 1), (1, 40, 2), (37, 1, 3), (5, 7, 10), (3, 3, 3), (6, 6, 5), (16, 16, 1), (30, 41, 2),
                                    (29, 33, 5), (100, 130, 1)])
def test_nms_map_matches_the_plain_statement(small, M, N, sz):
    """Constant planes (0, negative, positive: with sz >= M and N the neighbourhood is empty and vnmax = 0), quantised planes
    (ties inside blocks: the first maximum in row-major order is the block's candidate), ramps, noise; 1 x N and M x 1; planes
    of fewer blocks than a workgroup's threads, and of more."""
    rng = np.random.default_rng(M * 1000 + N + sz)
    yy, xx = np.mgrid[0:M, 0:N]
    planes = [np.zeros((M, N)), np.full((M, N), -1.5), np.full((M, N), 2.0), rng.integers(0, 3, (M, N)) * 0.5,
              rng.integers(-1, 1, (M, N)) * 1.0, (xx + yy) * 0.25, -(xx * 0.5) + yy * 0.0, (yy // 2) * 0.75, rng.normal(size=(M, N))]
    for i, a in enumerate(planes):
        a = np.ascontiguousarray(a, np.float32)
        np.testing.assert_array_equal(small.nms_map(a, sz), nms_ref.nms_map(a, sz), err_msg=f"plane {i}")
