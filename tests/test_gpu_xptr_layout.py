"""The x pass's pointer planes are stored transposed ([column][row], the level's row count as pitch: k_dp.hip, read-out): everything
that dereferences them — pbd_get_dp_pointers, k_backtrack, and through the candidates the part scores and latent detection — against
the oracle on the CPU, on frames whose levels are far from square.

Frames (all tiny): 96x40 and 40x96 pixels (levels of 22x8 .. 10x3 cells and their transposes: a pitch of W where H belongs, or the
reverse, reads another cell at every level), 412x44 (rows of 101 cells, a prime: several lanes share a row in the read-out and no
sub-range count divides it), and a batch of three 96x40 frames (virtual levels: frame f's level l is plan level f * nlevels + l, each
with planes of its own, read through pbd_get_frame_dp_pointers).  A level of a frame is never one cell high or wide — the pyramid ends where the image's shorter side is
5 sbin pixels, i.e. 3 cells (HOGFeatures.cpp:99, 174-175) — so the one-cell geometries go through pbd_dt2d, which runs the same two
launches on a map of any shape and hands out the same composed pointers.

Every handle variant: the fold (dp_mode 0), the x / y / k_reduce structure (1), the compact memory plan (2), double, and the
dt_correct_ptr composition (which reads Ix at the row Iy names).  The exact filter bank throughout: its responses are the oracle's bit
for bit, so every table and every candidate must be equal, not close."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_tree_model
from tests import latent_ref as LR
from tests.part_scores_ref import part_scores_ref
from tests.util import assert_candidates_equal

pytestmark = pytest.mark.gpu

FRAMES = {"wide": (61, 96, 40), "tall": (62, 40, 96), "long": (63, 412, 44)}
BATCH = [(61, 96, 40), (64, 96, 40), (65, 96, 40)]
# (dtype, dp_mode, dt_correct_ptr)
VARIANTS = {"fold": (np.float32, 0, 0), "reduce": (np.float32, 1, 0), "compact": (np.float32, 2, 0), "f64": (np.float64, 0, 0),
            "f64_reduce": (np.float64, 1, 0), "correct_ptr": (np.float32, 0, 1)}


def _image(spec):
    return make_image(*spec)


_model, _refs = [], {}


def model_of(orc):
    """one model for every test: five parts, three mixtures each, a threshold that keeps about a tenth of the root cells of the frames"""
    if not _model:
        m = make_tree_model([-1, 0, 1, 1, 0], 3, seed=5)
        m.thresh = -1e30
        vals = []
        for spec in FRAMES.values():
            fr = orc.detect(m, _image(spec), capacity=1, keep=True)[4]
            vals += [fr.root(l)[0].ravel() for l in range(fr.nlevels)]
            fr.free()
        m.thresh = float(np.float32(np.percentile(np.concatenate(vals), 90)))
        _model.append(m)
    return _model[0]


def reference(orc, spec, dtype, correct_ptr):
    """the oracle on one frame, computed once: candidates, per level the composed (Ix, Iy, Ik) of component 0, the responses, the scales"""
    key = (spec, np.dtype(dtype).name, correct_ptr)
    if key not in _refs:
        m = model_of(orc)
        heads, boxes, locs, _, fr = orc.detect(m, _image(spec), keep=True, correct_ptr=correct_ptr, dtype=dtype)
        resp = [fr.resp(l) for l in range(fr.nlevels)]
        tabs = [orc.dp_min_level(m.to_desc(), 0, r, correct_ptr, dtype)[:3] for r in resp]
        scales = [d[4] for d in fr.dims]
        fr.free()
        for a in (heads, boxes, locs, *resp, *[t for tab in tabs for t in tab]):
            a.setflags(write=False)
        _refs[key] = dict(cands=(heads, boxes, locs), tabs=tabs, resp=resp, scales=scales)
    return _refs[key]


def handle(orc, variant, **kw):
    dtype, dp_mode, correct_ptr = VARIANTS[variant]
    return capi.Handle(model_of(orc), conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, dp_mode=dp_mode, dt_correct_ptr=correct_ptr, **kw)


def assert_tables(hd, model, ref, frame=0):
    """the (Ix, Iy, Ik) of every (part, parent mixture) of one frame of the plan equal the oracle's at every cell: frame 0 of a single-frame
    plan through pbd_get_dp_pointers, a batch's frames through pbd_get_frame_dp_pointers (the stage entry points refuse batch plans)"""
    batch = frame is not None and getattr(hd, "_nbatch", 1) > 1
    for l, (Ix, Iy, Ik) in enumerate(ref["tabs"]):
        sh = Ix.shape[1:]
        plane = 0
        for p in range(1, model.nparts(0)):
            for pm in range(len(model.filterid[0][model.parentid[0][p]])):
                gx, gy, gk = (np.full(sh, -1, np.int32) for _ in range(3))
                out = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in (gx, gy, gk)]
                if batch:
                    hd._chk(hd.L.pbd_get_frame_dp_pointers(hd.h, frame, l, 0, p, pm, *out))
                else:
                    hd._chk(hd.L.pbd_get_dp_pointers(hd.h, l, 0, p, pm, *out))
                what = f"frame {frame} level {l} ({sh[1]}x{sh[0]} cells) part {p} parent mixture {pm}"
                np.testing.assert_array_equal(gk, Ik[plane], err_msg="Ik " + what)
                np.testing.assert_array_equal(gx, Ix[plane], err_msg="Ix " + what)
                np.testing.assert_array_equal(gy, Iy[plane], err_msg="Iy " + what)
                plane += 1


@pytest.mark.parametrize("name", list(FRAMES))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tables_and_candidates_equal_the_oracle(gpu_required, orc, variant, name):
    dtype, _, correct_ptr = VARIANTS[variant]
    ref = reference(orc, FRAMES[name], dtype, correct_ptr)
    assert len(ref["cands"][0]) > 20
    assert {t[0].shape[1] > t[0].shape[2] for t in ref["tabs"]} == {name == "tall"}   # every level is wide, or every level is tall
    hd = handle(orc, variant)
    for _ in range(2):   # twice: the second frame writes over the first one's planes
        assert_candidates_equal(hd.detect(_image(FRAMES[name])), ref["cands"])   # k_backtrack
    assert_tables(hd, hd.model, ref)
    gx, gy, gk = hd.frame_dp_pointers(0, 0, 0, 1, 0, *FRAMES[name][1:])   # a single-frame plan: frame 0 is pbd_get_dp_pointers
    np.testing.assert_array_equal(gx, ref["tabs"][0][0][0]); np.testing.assert_array_equal(gy, ref["tabs"][0][1][0])
    np.testing.assert_array_equal(gk, ref["tabs"][0][2][0])
    hd.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_batch_of_three_frames(gpu_required, orc, variant):
    dtype, _, correct_ptr = VARIANTS[variant]
    refs = [reference(orc, spec, dtype, correct_ptr) for spec in BATCH]
    hd = handle(orc, variant)
    got = hd.detect_batch([_image(spec) for spec in BATCH])
    hd._nbatch = len(BATCH)
    assert len({r["cands"][0].tobytes() for r in refs}) == 3   # three different frames
    for f, ref in enumerate(refs):
        assert len(ref["cands"][0]) > 20
        assert_candidates_equal(got[f], ref["cands"])
        assert_tables(hd, hd.model, ref, f)
    with pytest.raises(capi.PbdError) as e:   # frames of the plan only
        hd.frame_dp_pointers(len(BATCH), 0, 0, 1, 0, *BATCH[0][1:])
    assert e.value.code == capi.PBD_ERR_ARG
    hd.close()


@pytest.mark.parametrize("rows,cols", [(1, 37), (37, 1), (1, 1), (1, 300), (300, 1), (2, 131), (131, 2)])
@pytest.mark.parametrize("variant", ["fold", "f64", "correct_ptr"])
def test_one_cell_high_and_one_cell_wide_maps(gpu_required, orc, variant, rows, cols):
    dtype, _, correct_ptr = VARIANTS[variant]
    hd = handle(orc, variant)
    a = np.random.default_rng(rows * 1000 + cols).normal(0, 1, (rows, cols)).astype(dtype)
    for ax, bx, ay, by, osx, osy in ((-0.05, 0.01, -0.03, -0.02, 1, -2), (-0.5, 0.0, -0.25, 0.0, 0, 0)):
        out, ix, iy = hd.dt2d(a, ax, bx, ay, by, osx, osy)
        rout, rix, riy = orc.dt2d(a, ax, bx, ay, by, osx, osy, correct_ptr=correct_ptr, dtype=dtype)
        assert out.tobytes() == np.asarray(rout, dtype).tobytes()
        np.testing.assert_array_equal(ix, rix)
        np.testing.assert_array_equal(iy, riy)
    hd.close()


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "compact"])   # the compact plan's min() overwrites the responses: part scores refuse it
def test_part_scores_of_a_wide_frame(gpu_required, orc, variant):
    dtype, _, correct_ptr = VARIANTS[variant]
    ref = reference(orc, FRAMES["wide"], dtype, correct_ptr)
    hd = handle(orc, variant)
    hd.set_part_scores(True)
    heads, boxes, locs = hd.detect(_image(FRAMES["wide"]))
    assert_candidates_equal((heads, boxes, locs), ref["cands"])
    exp = part_scores_ref(hd.model, lambda l: ref["resp"][l], ref["cands"][0], ref["cands"][2])   # the oracle's planes and locations
    got = hd.part_scores(0)
    assert got.shape == exp.shape and got.tobytes() == exp.tobytes()
    hd.close()


@pytest.mark.parametrize("name", ["wide", "tall"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_latent_detection(gpu_required, orc, variant, name):
    dtype, _, correct_ptr = VARIANTS[variant]
    ref = reference(orc, FRAMES[name], dtype, correct_ptr)
    m = model_of(orc)
    level = 3
    H, W = ref["resp"][level].shape[1:]
    cells = [(W // 2 + (p % 3) - 1, H // 2 + (p // 3) % 3 - 1) for p in range(m.nparts(0))]
    truth = LR.truth_at(m, 0, ref["scales"][level], cells)
    exp = LR.detect(orc, m, ref["scales"], lambda l: ref["resp"][l], truth, 0.4, None, -1, 0, dtype, correct_ptr)
    assert exp["found"]
    hd = handle(orc, variant)
    heads, boxes, locs = hd.detect_latent(_image(FRAMES[name]), truth, 0.4)
    P = m.nparts(0)
    assert len(heads) == 1
    assert (int(heads[0]["component"]), int(heads[0]["level"]), int(heads[0]["nparts"])) == (exp["component"], exp["level"], P)
    assert np.float32(heads[0]["score"]).tobytes() == np.float32(exp["score"]).tobytes()
    np.testing.assert_array_equal(locs[0][:P], exp["locs"])
    np.testing.assert_array_equal(boxes[0][:P], exp["boxes"])
    hd.close()
