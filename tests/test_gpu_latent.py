"""Latent detection on the GPU (k_latent.hip: k_latent_mask between pdf and min, k_latent_best in front of the unchanged k_backtrack) held
bit for bit to tests/latent_ref.py: masks and flags through an integer view, the DP tables on the masked planes against the oracle's,
the returned record, the whole-path entries end to end.  No tolerance anywhere but the part-score identity (part_scores_ref.bound)."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_tree_model_k
from tests import dp_range_cases as R
from tests import latent_ref as LR
from tests.mixture_models import stack_components
from tests.part_scores_ref import bound, totals

pytestmark = pytest.mark.gpu
DTYPES = (np.float32, np.float64)
MODES = (0, 1, 2)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _tree(name, seed, **kw):
    parents, Ks = R.TREES[name]
    return make_tree_model_k(parents, Ks, seed=seed, **kw)


def _sized(m, sizes=(3, 5, 7)):
    m.filtersw = [np.zeros((sizes[i % 3], sizes[i % 3] * m.flen), np.float32) for i in range(len(m.filtersw))]
    return m


def _two():
    return stack_components(make_tree_model_k([-1, 0, 1], [1, 4, 1], seed=71), _tree("M6", 72))


# name -> (model, response kind, pad, component, forced mixtures, truth level / root cell or None for a truth nowhere near the frame)
def _cases():
    return {
        "free_M4": (_tree("M4", 61), "normal", 0, -1, None, (4, (8, 6))),
        "forced_M6": (_tree("M6", 62), "normal", 0, -1, (-1, 0, 3, 1, -1, 2), (6, (6, 5))),
        "two_all": (_two(), "normal", 0, -1, None, (3, (9, 7))),
        "two_fixed1": (_two(), "normal", 0, 1, (2, -1, -1, -1, -1, -1), (3, (9, 7))),
        "mixed_357_M4": (_sized(_tree("M4", 63)), "normal", 0, -1, None, (5, (7, 5))),
        "pad3_M1": (_tree("M1", 64), "normal", 3, -1, None, (4, (9, 8))),
        # exact ties.  Zero planes under a truth that covers the frame's left half at overlap 0: every window that touches it is
        # admissible, and the root score is one constant wherever the whole pose fits — across cells AND levels.  Twin components on
        # the same dyadic planes: every root score occurs in both.
        "tie_zero_M4": (_tree("M4", 65, quantised=True), "zero", 0, -1, None, "left"),
        "tie_twin_M4": (stack_components(_tree("M4", 66, quantised=True), _tree("M4", 66, quantised=True)), "twin", 0, -1, None, (2, (10, 8))),
        "none_M4": (_tree("M4", 67), "normal", 0, -1, None, None),
    }


CASES = _cases()
OVERLAP = {"tie_zero_M4": 0.0}


def _responses(name, model, geo, l, dtype):
    H, W = int(geo["cell_h"][l]), int(geo["cell_w"][l])
    rng = np.random.default_rng([sum(map(ord, name)), l])
    kind = CASES[name][1]
    nf = len(model.filtersw)
    if kind == "zero":
        return np.zeros((nf, H, W), dtype)
    if kind == "twin":
        return np.tile((rng.integers(-2, 3, (nf // 2, H, W)) * 0.5).astype(dtype), (2, 1, 1))
    return np.clip(rng.normal(0, 1, (nf, H, W)), -6, 6).astype(dtype)


def _truth(model, geo, pad, where):
    """the windows of mixture 0 of every part (of the largest component) one cell apart around a root cell of one level: a pose the
    model could return there.  Components with fewer parts use the first rows."""
    if where is None:
        return np.tile(np.array([50000, 50000, 20, 20], np.int32), (model.max_parts, 1))
    if where == "left":
        return np.tile(np.array([0, 0, 40, 79], np.int32), (model.max_parts, 1))
    l, (x, y) = where
    c = int(np.argmax([model.nparts(k) for k in range(model.ncomponents)]))
    cells = [(x + pad + (p % 3) - 1, y + pad + (p // 3) % 3 - 1) for p in range(model.nparts(c))]
    return LR.truth_at(model, c, geo["scales"][l], cells, pad)


_ref = {}


def _setup(orc, name, dtype, dp_mode, correct_ptr=0):
    """(handle with the case's responses resident, geometry, responses per level, truth, reference) — the reference is computed once per
    (case, type, pointer mode) and left unchanged"""
    model, _, pad, comp, mix, where = CASES[name]
    hd = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, dp_mode=dp_mode, dt_correct_ptr=correct_ptr, max_candidates=4096)
    if pad:
        hd.set_boundary_pad(pad)
    hd.begin_frame(*R.FRAME, 3)
    geo = hd._geo
    assert geo["nlevels"] == 21
    resp = [_responses(name, model, geo, l, dtype) for l in range(geo["nlevels"])]
    truth = _truth(model, geo, pad, where)
    for l, r in enumerate(resp):
        for n in range(len(model.filtersw)):
            hd.set_level_response(l, n, r[n])
    key = (name, np.dtype(dtype).name, correct_ptr)
    if key not in _ref:
        _ref[key] = LR.detect(orc, model, geo["scales"], lambda l: resp[l], truth, OVERLAP.get(name, 0.5), mix, comp, pad, dtype, correct_ptr)
    return hd, geo, resp, truth, _ref[key]


def _assert_record(got, ref, model):
    heads, boxes, locs = got
    assert len(heads) == ref["found"]
    if not ref["found"]:
        return
    P = model.nparts(ref["component"])
    assert (int(heads[0]["component"]), int(heads[0]["level"]), int(heads[0]["nparts"])) == (ref["component"], ref["level"], P)
    assert _bits(np.float32(heads[0]["score"])) == _bits(np.float32(ref["score"]))
    np.testing.assert_array_equal(locs[0][:P], ref["locs"])
    np.testing.assert_array_equal(boxes[0][:P], ref["boxes"])
    assert not boxes[0][P:].any() and not locs[0][P:].any()


@pytest.mark.parametrize("dp_mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(CASES))
def test_latent_stages_bit_exact(gpu_required, orc, name, dtype, dp_mode):
    """planes before the mask -> pbd_latent_mask -> the planes equal the reference's mask of those same planes and `admissible` its flags;
    pbd_dp_min -> rootv / rooti / Ix / Iy / Ik of every pair equal the oracle's on the masked planes; pbd_dp_argbest -> the reference's
    record (ties: the smallest level, component, y, x)."""
    model, _, pad, comp, mix, where = CASES[name]
    hd, geo, resp, truth, ref = _setup(orc, name, dtype, dp_mode)
    nf = len(model.filtersw)
    for l in (0, 7, 20):
        for n in (0, nf - 1):
            np.testing.assert_array_equal(_bits(hd.level_response(l, n)), _bits(resp[l][n]))
    adm = hd.latent_mask(truth, OVERLAP.get(name, 0.5), mix, comp)
    np.testing.assert_array_equal(adm, ref["admissible"])
    assert (where is None) == (not adm.any())
    masked_cells = 0
    for l in range(geo["nlevels"]):
        for n in range(nf):
            got = hd.level_response(l, n)
            np.testing.assert_array_equal(_bits(got), _bits(ref["masked"][l][n]), err_msg=f"masked plane level {l} filter {n}")
            masked_cells += int((got == LR.NEG).sum())
    assert masked_cells > 0
    hd.dp_min()
    for l in range(geo["nlevels"]):
        for c in range(model.ncomponents):
            Ix, Iy, Ik, rv, ri = ref["tables"][l][c]
            grv, gri = hd.root(l, c)
            np.testing.assert_array_equal(_bits(grv), _bits(rv), err_msg=f"rootv level {l} component {c}")
            np.testing.assert_array_equal(gri, ri, err_msg=f"rooti level {l} component {c}")
            if l % 4:
                continue
            plane = 0
            for p in range(1, model.nparts(c)):
                for pm in range(len(model.filterid[c][model.parentid[c][p]])):
                    gx, gy, gk = hd.dp_pointers(l, c, p, pm)
                    np.testing.assert_array_equal(gk, Ik[plane]); np.testing.assert_array_equal(gx, Ix[plane]); np.testing.assert_array_equal(gy, Iy[plane])
                    plane += 1
    _assert_record(hd.dp_argbest(), ref, model)
    if name.startswith("tie") and ref["found"]:
        v = ref["score"]
        ties = sum(int((ref["tables"][l][c][3] == v).sum()) for l in range(geo["nlevels"]) for c in range(model.ncomponents) if ref["admissible"][l, c])
        assert ties > 1, "the tie case has no tie"
    hd.close()


def test_latent_record_as_truth_and_argmin_afterwards(gpu_required, orc):
    """a record's own boxes as truth at overlap 0.999 give the record again (overlap exactly 1 at its cells); pbd_dp_argmin after
    pbd_dp_argbest thresholds the root tables again"""
    name = "free_M4"
    model = CASES[name][0]
    hd, geo, resp, truth, ref = _setup(orc, name, np.float32, 0, correct_ptr=1)   # true arg-max pointers: the pose is the unique optimum
    hd.latent_mask(truth, 0.5)
    hd.dp_min()
    first = hd.dp_argbest()
    _assert_record(first, ref, model)
    rv = np.concatenate([ref["tables"][l][0][3].ravel() for l in range(geo["nlevels"])])
    model.thresh = float(np.float32(np.sort(rv)[-10]))
    hd2 = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, max_candidates=4096, dt_correct_ptr=1)
    hd2.begin_frame(*R.FRAME, 3)
    for l, r in enumerate(resp):
        for n in range(len(model.filtersw)):
            hd2.set_level_response(l, n, r[n])
    own = np.zeros((model.max_parts, 4), np.int32)
    own[:len(ref["boxes"])] = first[1][0][:len(ref["boxes"])]
    hd2.latent_mask(own, 0.999)
    hd2.dp_min()
    again = hd2.dp_argbest()
    assert len(again[0]) == 1 and again[0][0]["level"] == first[0][0]["level"]
    np.testing.assert_array_equal(again[2], first[2])
    n_above = int((np.concatenate([hd2.root(l, 0)[0].ravel() for l in range(geo["nlevels"])]).astype(np.float64) > model.thresh).sum())
    assert len(hd2.dp_argmin(4096)[0]) == n_above
    hd.close(); hd2.close()


# ---------------------------------------------------------------- whole path
def _oracle_latent(orc, model, im, truth, overlap, mix=None, component=-1, dtype=np.float32):
    fr = orc.detect(model, im, capacity=1, keep=True, dtype=dtype)[4]
    scales = [d[4] for d in fr.dims]
    out = LR.detect(orc, model, scales, lambda l: fr.resp(l) if fr.dims[l][2] * fr.dims[l][3] else None, truth, overlap, mix, component, 0, dtype)
    fr.free()
    return out


def _frame_truth(orc, model, im, level, cell):
    g = orc.geometry(im.shape[1], im.shape[0], model.sbin, model.interval)
    x, y = cell
    return LR.truth_at(model, 0, g["scales"][level], [(x + (p % 3) - 1, y + (p // 3) % 3 - 1) for p in range(model.nparts(0))])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_detect_latent_exact_bank_end_to_end(gpu_required, orc, dtype):
    """PBD_CONV_EXACT: pbd_detect_latent_u8, the device-image entry and the batch entry (two frames, two truth sets) equal the oracle's
    pyramid, features and responses -> the reference; the model's threshold plays no part"""
    model = _tree("M4", 81)
    model.thresh = 1e30
    frames = [make_image(51, 160, 120), make_image(52, 160, 120)]
    truths = [_frame_truth(orc, model, frames[0], 5, (9, 7)), _frame_truth(orc, model, frames[1], 8, (6, 5))]
    mixes = [np.array([-1, 1, -1, 2, 0], np.int32), np.full(5, -1, np.int32)]
    refs = [_oracle_latent(orc, model, f, t, 0.4, m, dtype=dtype) for f, t, m in zip(frames, truths, mixes)]
    assert all(r["found"] for r in refs)
    hd = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype)
    for f, t, m, r in zip(frames, truths, mixes, refs):
        _assert_record(hd.detect_latent(f, t, 0.4, m), r, model)
    for got, r in zip(hd.detect_batch_latent(frames, truths, 0.4, mixes), refs):
        _assert_record(got, r, model)
    far = np.tile(np.array([50000, 50000, 9, 9], np.int32), (5, 1))
    got = hd.detect_batch_latent(frames, [far, truths[1]], 0.4, [mixes[1], mixes[1]])
    assert len(got[0][0]) == 0
    _assert_record(got[1], refs[1], model)
    if np.dtype(dtype) == np.float32:
        import torch
        t = torch.from_numpy(frames[0]).cuda()
        torch.cuda.synchronize()
        _assert_record(hd.detect_latent_dev(t.data_ptr(), 160, 120, 3, truths[0], 0.4, mixes[0]), refs[0], model)
    hd.close()


@pytest.mark.parametrize("graph", [0, 1])
def test_detect_latent_default_bank_is_the_stage_composition(gpu_required, orc, graph):
    """the default bank (PBD_CONV_AUTO: the split-product bank from 16 filters on): pbd_detect_latent_u8 equals pyramid -> pdf -> mask ->
    min -> argbest on the same handle, bit for bit; a plain detect() before and after a latent frame is unchanged (eager and replayed)"""
    model = _tree("M6", 82)
    model.thresh = 0.5
    assert len(model.filtersw) >= 16
    im = make_image(53, 160, 120)
    hd = capi.Handle(model, graph=graph, max_candidates=32768)
    assert hd.conv_mode == capi.PBD_CONV_SPLIT
    hd.pyramid(im); hd.pdf()
    truth = _frame_truth(orc, model, im, 4, (10, 8))
    hd.latent_mask(truth, 0.3)
    hd.dp_min()
    staged = hd.dp_argbest()
    assert len(staged[0]) == 1
    plain = [hd.detect(im, 32768) for _ in range(3)]
    whole = hd.detect_latent(im, truth, 0.3)
    after = [hd.detect(im, 32768) for _ in range(2)]
    for k in range(3):
        np.testing.assert_array_equal(whole[k], staged[k])
    for other in plain[1:] + after:
        for k in range(3):
            np.testing.assert_array_equal(other[k], plain[0][k])
    assert len(plain[0][0]) > 0
    hd.close()


def test_latent_part_scores_reproduce_the_score(gpu_required, orc):
    """with dt_correct_ptr = 1 the per-part scores of a latent record add up to its score within part_scores_ref.bound"""
    model = _tree("M4", 83)
    im = make_image(54, 160, 120)
    truth = _frame_truth(orc, model, im, 5, (9, 7))
    hd = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dt_correct_ptr=1)
    hd.set_part_scores(True)
    heads, boxes, locs = hd.detect_latent(im, truth, 0.4)
    assert len(heads) == 1
    ps = hd.part_scores(0)
    assert ps.shape == (1, model.max_parts, 3)
    assert (np.abs(ps[0, :, 0]) < 1e9).all(), "a part sits on a masked cell"
    err = abs(float(totals(ps)[0]) - float(heads[0]["score"]))
    b = float(bound(ps, [5], np.float32)[0]) + 2.0 ** -24 * abs(float(heads[0]["score"]))
    print(f"LATENT-PARTSCORES error {err:.3e} bound {b:.3e}")
    assert err <= b
    hd.close()


# ---------------------------------------------------------------- refusals
def _code(fn):
    with pytest.raises(capi.PbdError) as e:
        fn()
    return e.value.code


def test_latent_refusals(gpu_required):
    model = _tree("M4", 84)
    model.thresh = 1e30       # the pending plain frame below is there to be pending: it returns nothing.  Latent frames ignore thresh_
    im = make_image(55, 160, 120)
    truth = np.tile(np.array([10, 10, 30, 30], np.int32), (5, 1))
    hd = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT)
    bad = truth.copy(); bad[3, 2] = -1
    assert _code(lambda: hd.detect_latent(im, bad, 0.5)) == capi.PBD_ERR_ARG
    bad = truth.copy(); bad[0, 3] = -5
    assert _code(lambda: hd.detect_latent(im, bad, 0.5)) == capi.PBD_ERR_ARG
    for ov in (-0.1, 1.0, float("nan")):
        assert _code(lambda: hd.detect_latent(im, truth, ov)) == capi.PBD_ERR_ARG
    assert _code(lambda: hd.detect_latent(im, truth, 0.5, mix=[0, 2, 0, 0, 0])) == capi.PBD_ERR_ARG     # part 1 has two mixtures
    assert _code(lambda: hd.detect_latent(im, truth, 0.5, mix=[-2, 0, 0, 0, 0])) == capi.PBD_ERR_ARG
    for comp in (-2, 1):
        assert _code(lambda: hd.detect_latent(im, truth, 0.5, component=comp)) == capi.PBD_ERR_ARG
    hd._geo = hd.geometry(160, 120)
    hd.enqueue(np.ascontiguousarray(im))
    assert _code(lambda: hd.detect_latent(im, truth, 0.5)) == capi.PBD_ERR_STATE
    assert _code(lambda: hd.latent_mask(truth, 0.5)) == capi.PBD_ERR_STATE
    hd.collect()
    assert len(hd.detect_latent(im, truth, 0.5)[0]) == 1          # the handle is fine afterwards
    hd.close()
    st = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT)
    st.pyramid(im)
    assert _code(lambda: st.latent_mask(truth, 0.5)) == capi.PBD_ERR_STATE   # before pdf()
    st.pdf()
    assert _code(st.dp_argbest) == capi.PBD_ERR_STATE                        # before min()
    st.close()
    nms = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, nms_sz=1)
    assert _code(lambda: nms.detect_latent(im, truth, 0.5)) == capi.PBD_ERR_UNSUPPORTED
    nms.close()
    shared = _tree("M4", 85)
    shared.filterid[0][3][1] = shared.filterid[0][2][0]           # parts 2 and 3 share a response plane
    sh = capi.Handle(shared, conv_mode=capi.PBD_CONV_EXACT)
    assert _code(lambda: sh.detect_latent(im, truth, 0.5)) == capi.PBD_ERR_UNSUPPORTED
    assert "shared" in sh.L.pbd_last_error(sh.h).decode()
    sh.close()
    grp = capi.Group(model, [0], gather=capi.PBD_GATHER_HOST, conv_mode=capi.PBD_CONV_EXACT)
    member = C.c_void_p(grp.L.pbd_group_member(grp.g, 0))
    tr = np.ascontiguousarray(truth)
    rc = grp.L.pbd_latent_mask(member, tr.ctypes.data_as(C.c_void_p), None, -1, C.c_double(0.5), None)
    assert rc == capi.PBD_ERR_UNSUPPORTED
    grp.close()
