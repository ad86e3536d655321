"""Fold plans do not store the winning child mixtures (Ik) any more: k_backtrack picks them at the cells it visits from the children's
kept scores (csrc/fold_pick.hpp), and k_ik_fill writes the planes only when somebody asks for the tables.  Everything that used to read
the planes, against the oracle bit for bit, on the 100 x 80 frame of tests/dp_range_cases.py (21 levels, 23 x 18 cells down to 4 x 3):

* detect(): candidates, locs[:, 2] (the mixtures) included — float and double, the fold and the compact plan, both pointer compositions,
  a single frame, a batch of three, a captured graph replayed twice;
* the tables after such a frame, from pbd_get_dp_pointers / pbd_get_frame_dp_pointers: twice, then another frame, then again;
* a caller's own Ik (pbd_set_dp_pointers) is what pbd_dp_argmin follows, and the three-kernel structure still writes and reads planes;
* a response plane handed in on the compact plan — it overwrites kept scores — leaves the tables and the back-tracking as they were;
* part scores and latent detection, which start from the candidates' mixtures.

Models: fold widths 1, 4, 6 and 8 with a mixture count per part (dp_range_cases.TREES), plain and quantised (exact ties: the tie
cases of tests/test_gpu_mixture_counts.py).  The exact filter bank throughout: its responses are the oracle's, so equal means equal."""
import ctypes as C

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_tree_model_k
from tests import latent_ref as LR
from tests.dp_range_cases import FRAME, LEVEL_W, TREES
from tests.part_scores_ref import part_scores_ref
from tests.test_gpu_mixture_counts import TIE_CASES
from tests.util import assert_candidates_equal

pytestmark = pytest.mark.gpu

SEEDS = (81, 82, 83)                     # the frames: SEEDS[0] alone, all three as a batch
# (dtype, dp_mode, dt_correct_ptr): dp_mode 0 the fold, 2 the fold on the compact memory plan, 1 the three-kernel structure (k_reduce)
VARIANTS = {"fold": (np.float32, 0, 0), "fold_f64": (np.float64, 0, 0), "compact": (np.float32, 2, 0), "compact_f64": (np.float64, 2, 0),
            "fold_cp": (np.float32, 0, 1), "compact_cp": (np.float32, 2, 1), "fold_f64_cp": (np.float64, 0, 1), "reduce": (np.float32, 1, 0)}
MODELS = {"M1": ("M1", False), "M4": ("M4", False), "M6": ("M6", False), "M8": ("M8", False), "M6_ties": ("M6", True), "M8_ties": ("M8", True)}

_models, _refs = {}, {}


def image(seed):
    return make_image(seed, *FRAME)


def model_of(orc, name):
    """a threshold that keeps about a twentieth of the first frame's root cells (float scores; the double handles share it)"""
    if name not in _models:
        tree, ties = MODELS[name]
        parents, Ks = TREES[tree]
        assert not ties or (parents, Ks) == TIE_CASES["fold_" + tree][:2]
        m = make_tree_model_k(parents, Ks, seed=90 + sorted(MODELS).index(name), quantised=ties)
        m.thresh = -1e30
        fr = orc.detect(m, image(SEEDS[0]), capacity=1, keep=True)[4]
        assert fr.nlevels == 21 and fr.root(0)[0].shape[-1] == LEVEL_W[0]
        vals = np.concatenate([fr.root(l)[0].ravel() for l in range(fr.nlevels)])
        fr.free()
        m.thresh = float(np.float32(np.percentile(vals, 95)))
        _models[name] = m
    return _models[name]


def reference(orc, name, seed, dtype, correct_ptr):
    """the oracle on one frame, computed once and frozen: candidates, per level (Ix, Iy, Ik) of component 0, responses, scales"""
    key = (name, seed, np.dtype(dtype).name, correct_ptr)
    if key not in _refs:
        m = model_of(orc, name)
        heads, boxes, locs, _, fr = orc.detect(m, image(seed), keep=True, correct_ptr=correct_ptr, dtype=dtype)
        resp = [fr.resp(l) for l in range(fr.nlevels)]
        tabs = [orc.dp_min_level(m.to_desc(), 0, r, correct_ptr, dtype)[:3] for r in resp]
        scales = [d[4] for d in fr.dims]
        fr.free()
        for a in (heads, boxes, locs, *resp, *[t for tab in tabs for t in tab]):
            a.setflags(write=False)
        _refs[key] = dict(cands=(heads, boxes, locs), tabs=tabs, resp=resp, scales=scales)
    return _refs[key]


def handle(orc, name, variant, **kw):
    dtype, dp_mode, correct_ptr = VARIANTS[variant]
    return capi.Handle(model_of(orc, name), conv_mode=capi.PBD_CONV_EXACT, dtype=dtype, dp_mode=dp_mode, dt_correct_ptr=correct_ptr, **kw)


def planes_of(model):
    """[(part, parent mixture)] in the oracle's plane order"""
    return [(p, pm) for p in range(1, model.nparts(0)) for pm in range(len(model.filterid[0][model.parentid[0][p]]))]


def assert_tables(hd, ref, frame=None):
    """every (Ix, Iy, Ik) of one frame of the plan: pbd_get_dp_pointers (frame None), pbd_get_frame_dp_pointers (a batch's frame)"""
    for l, (Ix, Iy, Ik) in enumerate(ref["tabs"]):
        for plane, (p, pm) in enumerate(planes_of(hd.model)):
            if frame is None:            # (arrays sized by the oracle's planes: capi.Handle.dp_pointers sizes them by a begin_frame geometry)
                gx, gy, gk = (np.full(Ik[plane].shape, -1, np.int32) for _ in range(3))
                hd._chk(hd.L.pbd_get_dp_pointers(hd.h, l, 0, p, pm, *[a.ctypes.data_as(C.POINTER(C.c_int32)) for a in (gx, gy, gk)]))
            else:
                gx, gy, gk = hd.frame_dp_pointers(frame, l, 0, p, pm, *FRAME)
            what = f"frame {frame} level {l} part {p} parent mixture {pm}"
            np.testing.assert_array_equal(gk, Ik[plane], err_msg="Ik " + what)
            np.testing.assert_array_equal(gx, Ix[plane], err_msg="Ix " + what)
            np.testing.assert_array_equal(gy, Iy[plane], err_msg="Iy " + what)


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_candidates_single_batch_and_graph(gpu_required, orc, variant, name):
    dtype, _, cp = VARIANTS[variant]
    refs = [reference(orc, name, s, dtype, cp) for s in SEEDS]
    assert len(refs[0]["cands"][0]) > 20 and len({r["cands"][0].tobytes() for r in refs}) == 3
    if MODELS[name][0] != "M1":
        assert len(np.unique(refs[0]["cands"][2][:, 1:, 2])) > 1            # the candidates do choose between mixtures
    hd = handle(orc, name, variant)
    for _ in range(2):
        assert_candidates_equal(hd.detect(image(SEEDS[0])), refs[0]["cands"])
    for got, ref in zip(hd.detect_batch([image(s) for s in SEEDS]), refs):
        assert_candidates_equal(got, ref["cands"])
    hd.close()
    hd = handle(orc, name, variant, graph=1)
    for i in range(4):                   # an eager frame, the capture, two replays
        assert_candidates_equal(hd.detect(image(SEEDS[i % 2])), refs[i % 2]["cands"])
    if name in ("M6", "M8_ties"):        # the tables behind a replay (the graph's back-tracking picks, whatever the host asked for in between), then a replay behind them
        assert_tables(hd, refs[1])
        assert_candidates_equal(hd.detect(image(SEEDS[0])), refs[0]["cands"])
        assert_tables(hd, refs[0])
    hd.close()


@pytest.mark.parametrize("name", ["M4", "M8", "M6_ties"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tables_on_request_after_a_frame(gpu_required, orc, variant, name):
    dtype, _, cp = VARIANTS[variant]
    refs = [reference(orc, name, s, dtype, cp) for s in SEEDS]
    hd = handle(orc, name, variant)
    assert_candidates_equal(hd.detect(image(SEEDS[0])), refs[0]["cands"])
    assert_tables(hd, refs[0])
    assert_tables(hd, refs[0])           # already materialised
    assert_candidates_equal(hd.dp_argmin(), refs[0]["cands"])              # back-tracking over the materialised planes
    assert_candidates_equal(hd.detect(image(SEEDS[1])), refs[1]["cands"])  # the next frame: lazy again, other values
    assert_tables(hd, refs[1])
    got = hd.detect_batch([image(s) for s in SEEDS])
    for f in (2, 0, 1):
        assert_candidates_equal(got[f], refs[f]["cands"])
        assert_tables(hd, refs[f], frame=f)
    hd.close()


def _backtrack(model, tabs, head, root_loc):
    """argmin over (Ix, Iy, Ik) planes as DynamicProgram::argmin reads them -> locs [P, 3]"""
    Ix, Iy, Ik = tabs[int(head["level"])]
    first = {}
    for plane, (p, pm) in enumerate(planes_of(model)):
        first.setdefault(p, plane)
    locs = np.zeros((model.nparts(0), 3), np.int32)
    locs[0] = root_loc
    for p in range(1, model.nparts(0)):
        px, py, pm = locs[model.parentid[0][p]]
        pl = first[p] + pm
        locs[p] = (Ix[pl][py, px], Iy[pl][py, px], Ik[pl][py, px])
    return locs


@pytest.mark.parametrize("variant", ["fold", "compact_f64", "reduce"])
def test_callers_ik_is_followed(gpu_required, orc, variant):
    """pbd_set_dp_pointers with Ik altered at the candidates' cells: pbd_dp_argmin must return the altered mixtures — and, below
    them, the children picked under the altered parent mixture — which only the planes can tell it"""
    name = "M6"
    dtype, _, cp = VARIANTS[variant]
    ref = reference(orc, name, SEEDS[0], dtype, cp)
    m = model_of(orc, name)
    hd = handle(orc, name, variant)
    heads, boxes, locs = hd.detect(image(SEEDS[0]))
    assert_candidates_equal((heads, boxes, locs), ref["cands"])
    tabs = [tuple(np.array(t) for t in tab) for tab in ref["tabs"]]
    part = 2                                                               # K = 6, parent: part 1 (K = 1), children: part 3
    assert len(m.filterid[0][part]) == 6 and m.parentid[0][3] == part
    plane = [pl for pl, (p, pm) in enumerate(planes_of(m)) if p == part][0]
    changed = 0
    for l in sorted({int(h["level"]) for h in heads}):
        Ix, Iy, Ik = tabs[l]
        for h, lc in zip(heads, locs):
            if int(h["level"]) == l:
                px, py, _ = lc[m.parentid[0][part]]
                Ik[plane][py, px] = (ref["tabs"][l][2][plane][py, px] + 1) % 6
        hd.set_dp_pointers(l, 0, part, 0, Ix[plane], Iy[plane], Ik[plane])
    got = hd.dp_argmin()
    assert len(got[0]) == len(heads) and got[0].tobytes() == heads.tobytes()
    for h, lc, glc in zip(heads, locs, got[2]):
        exp = _backtrack(m, tabs, h, lc[0])
        np.testing.assert_array_equal(glc[:m.nparts(0)], exp)
        changed += int(exp[part][2] != lc[part][2])
    assert changed == len(heads)
    hd.close()


@pytest.mark.parametrize("variant", ["compact", "compact_f64"])
def test_response_handed_in_on_the_compact_plan_keeps_the_tables(gpu_required, orc, variant):
    """the compact plan keeps a mixture's transformed scores in its own response plane: pbd_set_level_response after a frame goes over
    what Ik would be picked from, so the planes are written first"""
    name = "M4"
    dtype, _, cp = VARIANTS[variant]
    ref = reference(orc, name, SEEDS[0], dtype, cp)
    m = model_of(orc, name)
    hd = handle(orc, name, variant)
    assert_candidates_equal(hd.detect(image(SEEDS[0])), ref["cands"])
    for l in (0, 7, 20):
        for f in m.filterid[0][2]:
            hd.set_level_response(l, f, np.full(ref["resp"][l][f].shape, 1e3, dtype))
    assert_candidates_equal(hd.dp_argmin(), ref["cands"])
    assert_tables(hd, ref)
    hd.close()


@pytest.mark.parametrize("variant", ["fold", "fold_f64", "fold_cp"])       # (the compact plan's min() overwrites the responses: part scores refuse it)
def test_part_scores(gpu_required, orc, variant):
    dtype, _, cp = VARIANTS[variant]
    ref = reference(orc, "M8", SEEDS[0], dtype, cp)
    hd = handle(orc, "M8", variant)
    hd.set_part_scores(True)
    assert_candidates_equal(hd.detect(image(SEEDS[0])), ref["cands"])
    exp = part_scores_ref(hd.model, lambda l: ref["resp"][l], ref["cands"][0], ref["cands"][2])
    got = hd.part_scores(0)
    assert got.shape == exp.shape and got.tobytes() == exp.tobytes()
    hd.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_latent_detection(gpu_required, orc, variant):
    dtype, _, cp = VARIANTS[variant]
    ref = reference(orc, "M6", SEEDS[0], dtype, cp)
    m = model_of(orc, "M6")
    level = 3
    H, W = ref["resp"][level].shape[1:]
    cells = [(W // 2 + (p % 3) - 1, H // 2 + (p // 3) % 3 - 1) for p in range(m.nparts(0))]
    truth = LR.truth_at(m, 0, ref["scales"][level], cells)
    exp = LR.detect(orc, m, ref["scales"], lambda l: ref["resp"][l], truth, 0.4, None, -1, 0, dtype, cp)
    assert exp["found"]
    hd = handle(orc, "M6", variant)
    heads, boxes, locs = hd.detect_latent(image(SEEDS[0]), truth, 0.4)
    P = m.nparts(0)
    assert len(heads) == 1
    assert (int(heads[0]["component"]), int(heads[0]["level"]), int(heads[0]["nparts"])) == (exp["component"], exp["level"], P)
    assert np.float32(heads[0]["score"]).tobytes() == np.float32(exp["score"]).tobytes()
    np.testing.assert_array_equal(locs[0][:P], exp["locs"])
    np.testing.assert_array_equal(boxes[0][:P], exp["boxes"])
    hd.close()
