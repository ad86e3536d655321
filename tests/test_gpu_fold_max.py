"""The fold's value form (csrc/fold_pick.hpp: fold_max; k_dp.hip: fold_children) on the GPU, against the oracle bit for bit.

The fold takes a message as `max_k(sd[k] + bias[k])` by a maximum instruction and computes a child again with fold_pick's compare /
select chain when a lane of the wavefront meets a maximum that is a zero (tied zeros of both signs: the reference keeps the first).
Both paths must run and both must give the oracle's tables:

* models of tests/mixture_models.py's kind — a 2-part chain, a 3-part star (two children on one parent) and a two-component model made
  of the two — with (K child, L parent) mixtures in {(1,1), (1,6), (6,1), (2,3), (6,6), (8,8)}: fold widths 1, 4, 6 and 8;
* one 64 x 48 frame whose responses are handed in through pbd_set_level_response, in three kinds by level: 'zeros' (planes of -0.0 /
  +0.0, biases of both zeros: the maxima are tied zeros of both signs — the branch), 'ints' (small non-positive integers and zeros: some wavefronts
  branch, some do not) and 'clear' (integers + 1/256 under dyadic deformations and biases that are multiples of 1/4: no sum is a zero,
  no lane branches).  The host reference says at which cells the tied zeros are, and that a maximum which orders -0.0 below +0.0
  (dp_ref's "zero_order" slip) changes root scores there;
* Ix / Iy / Ik of every plane, the root scores through an integer view, rooti and the back-tracked candidates;
* the same models on a batch of two real 64 x 48 frames, and the person model (26 parts x 6 mixtures) on one 96 x 80 frame, through the
  exact filter bank (its responses are the oracle's)."""
import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_person_model, make_tree_model_k
from tests import dp_ref
from tests.mixture_models import stack_components
from tests.util import thresh_from_oracle

pytestmark = pytest.mark.gpu

FRAME = (64, 48)
KL = [(1, 1), (1, 6), (6, 1), (2, 3), (6, 6), (8, 8)]                     # (K of the children, L of their parent)
SHAPES = ["chain", "star", "two"]
KINDS = ("zeros", "ints", "clear")                                        # level l gets KINDS[l % 3]
CAP = 4096
_models, _expected, GEO = {}, {}, {}


@pytest.fixture(autouse=True)
def _geometry(orc):
    if not GEO:
        GEO.update(orc.geometry(*FRAME, 4, 10))
        assert GEO["nlevels"] >= 6 and int(GEO["cell_w"][0]) >= 12


def _signed_zero_model(parents, Ks, seed):
    """quantised deformations; biases: both zeros and -1/4, the root's -0.0; the first mixture of every part keeps
    the sign of a zero (bias(0)[m] = -0.0, linear weights >= 0) and comes first in every tie, the others may turn it (dp_range_cases, family Z)"""
    m = make_tree_model_k(parents, Ks, seed=seed, quantised=True)
    rng = np.random.default_rng(seed + 1000)
    m.defw = np.array(m.defw, np.float32)
    m.biasw = rng.choice(np.array([-0.0, 0.0, -0.25], np.float32), len(m.biasw), p=[0.45, 0.35, 0.2]).astype(np.float32)   # (none positive: zeros stay maxima)
    m.biasw[m.biasid[0][0][0]] = np.float32(-0.0)
    lin = np.abs(m.defw[:, [1, 3]])
    lin[rng.random(lin.shape) < 0.3] *= np.float32(-1.0)
    m.defw[:, [1, 3]] = lin
    for p in range(1, m.nparts(0)):
        L = len(m.filterid[0][parents[p]])
        m.biasw[m.biasid[0][p][0]:m.biasid[0][p][0] + L] = np.float32(-0.0)
        m.defw[m.defid[0][p][0], [1, 3]] = np.abs(m.defw[m.defid[0][p][0], [1, 3]])
    return m


def model_of(shape, K, L):
    key = (shape, K, L)
    if key not in _models:
        seed = 300 + 10 * KL.index((K, L))
        chain = _signed_zero_model([-1, 0], [L, K], seed)
        star = _signed_zero_model([-1, 0, 0], [L, K, K], seed + 1)
        _models[key] = {"chain": chain, "star": star}[shape] if shape != "two" else stack_components(chain, star)
    return _models[key]


def responses(model, level, kind, seed):
    rng = np.random.default_rng(seed * 100 + level)
    shape = (len(model.filtersw), int(GEO["cell_h"][level]), int(GEO["cell_w"][level]))
    if kind == "zeros":
        return np.array([-0.0, 0.0], np.float32)[rng.choice(2, shape, p=[0.8, 0.2])]
    if kind == "ints":
        return np.array([-0.0, 0.0, -3.0, -2.0, -1.0], np.float32)[rng.choice(5, shape, p=[0.3, 0.15, 0.2, 0.2, 0.15])]   # (none positive: a zero stays its cell's maximum)
    return (rng.integers(-3, 4, shape) + 1.0 / 256).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tied_zero_cells(model, comp, maps):
    """cells of a level at which a message's maximum is a zero held by entries of both signs, and cells at which any message is a zero"""
    fid, bid, par = model.filterid[comp], model.biasid[comp], model.parentid[comp]
    tied = anyzero = 0
    for p in range(1, model.nparts(comp)):
        for m in range(len(fid[par[p]])):
            w = np.stack([(maps["sdt"][p][k] + np.float32(model.biasw[bid[p][k] + m])).astype(np.float32) for k in range(len(fid[p]))])
            top = w.max(axis=0)
            attn = (w == top[None]) & (top[None] == 0)
            tied += int((attn & np.signbit(w)).any(axis=0)[(attn & ~np.signbit(w)).any(axis=0)].sum())
            anyzero += int((top == 0).sum())
    return tied, anyzero


def expected(orc, shape, K, L):
    """per level: responses, per component the oracle's tables; the candidates; how many tied-zero cells each kind of level holds and whether
    the zero_order slip shows in the root scores — computed once, left unchanged"""
    key = (shape, K, L)
    if key not in _expected:
        m = model_of(shape, K, L)
        desc = m.to_desc()
        levels, tied, anyzero, slip_shows = [], dict.fromkeys(KINDS, 0), dict.fromkeys(KINDS, 0), False
        for l in range(GEO["nlevels"]):
            kind = KINDS[l % 3]
            resp = responses(m, l, kind, 7 + KL.index((K, L)))
            tabs = [orc.dp_min_level(desc, c, resp) for c in range(m.ncomponents)]
            for c in range(m.ncomponents):
                t, z = tied_zero_cells(m, c, dp_ref.level_maps(orc, m, c, resp))
                tied[kind] += t
                anyzero[kind] += z
                if kind == "zeros" and K > 1 and not slip_shows:
                    slip_shows = not np.array_equal(_bits(dp_ref.plain_level(m, c, resp, orc=orc, slip="zero_order")[3]), _bits(tabs[c][3]))
            levels.append((resp, tabs))
        vals = np.sort(np.concatenate([t[3].ravel() for _, tabs in levels for t in tabs]))
        m.thresh = float(np.nextafter(np.float32(vals[-min(40, len(vals) // 4)]), np.float32(-np.inf)))
        desc = m.to_desc()                        # (the threshold travels in the descriptor)
        cands = [orc.dp_argmin_level(desc, c, l, GEO["scales"][l], t[3], t[4], t[0], t[1], t[2], capacity=CAP)
                 for l, (_, tabs) in enumerate(levels) for c, t in enumerate(tabs)]
        cands = tuple(np.concatenate([c[i] for c in cands]) for i in range(3))
        for a in [*cands] + [x for r, tabs in levels for x in (r, *[y for t in tabs for y in t])]:
            a.setflags(write=False)
        _expected[key] = dict(levels=levels, cands=cands, tied=tied, anyzero=anyzero, slip_shows=slip_shows, thresh=m.thresh)
    return _expected[key]


def canon(c):
    """candidates ordered by (level, component, root row, root column): the comparison is of the set, bit for bit"""
    heads, boxes, locs = c
    o = np.lexsort((locs[:, 0, 0], locs[:, 0, 1], heads["component"], heads["level"]))
    return heads[o], boxes[o], locs[o]


def assert_same_candidates(got, want):
    (ha, ba, la), (hb, bb, lb) = canon(got), canon(want)
    assert len(ha) == len(hb), (len(ha), len(hb))
    assert ha.tobytes() == hb.tobytes()
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(ba, bb)


@pytest.mark.parametrize("K,L", KL, ids=[f"K{k}L{l}" for k, l in KL])
@pytest.mark.parametrize("shape", SHAPES)
def test_tables_roots_and_candidates_on_tied_zeros(gpu_required, orc, shape, K, L):
    m = model_of(shape, K, L)
    exp = expected(orc, shape, K, L)
    m.thresh = exp["thresh"]
    # the inputs do what they are for: tied zeros of both signs where K > 1 (one weighted map cannot tie), zero maxima on the integer
    # levels, none at all on the clear ones — there no lane leaves the fast path
    print(f"FOLDMAX {shape} K{K} L{L}: tied-zero cells {exp['tied']}, zero maxima {exp['anyzero']}, zero_order slip shows {exp['slip_shows']}")
    assert exp["anyzero"]["zeros"] > 0 and exp["anyzero"]["ints"] > 0 and exp["anyzero"]["clear"] == 0
    if K > 1:
        assert exp["tied"]["zeros"] > 0 and exp["slip_shows"]
    assert 10 <= len(exp["cands"][0]) < CAP
    hd = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, max_candidates=CAP)
    hd.begin_frame(*FRAME, 3)
    assert np.array_equal(hd._geo["cell_w"], GEO["cell_w"]) and np.array_equal(hd._geo["cell_h"], GEO["cell_h"])
    for l, (resp, _) in enumerate(exp["levels"]):
        for n in range(len(m.filtersw)):
            hd.set_level_response(l, n, resp[n])
    hd.dp_min()
    for l, (_, tabs) in enumerate(exp["levels"]):
        for c, (Ix, Iy, Ik, rv, ri) in enumerate(tabs):
            grv, gri = hd.root(l, c)
            np.testing.assert_array_equal(_bits(grv), _bits(rv), err_msg=f"rootv level {l} ({KINDS[l % 3]}) component {c}")
            np.testing.assert_array_equal(gri, ri, err_msg=f"rooti level {l} component {c}")
            plane = 0
            for p in range(1, m.nparts(c)):
                for pm in range(len(m.filterid[c][m.parentid[c][p]])):
                    gx, gy, gk = hd.dp_pointers(l, c, p, pm)
                    where = f"level {l} ({KINDS[l % 3]}) component {c} part {p} parent mixture {pm}"
                    np.testing.assert_array_equal(gk, Ik[plane], err_msg="Ik " + where)
                    np.testing.assert_array_equal(gx, Ix[plane], err_msg="Ix " + where)
                    np.testing.assert_array_equal(gy, Iy[plane], err_msg="Iy " + where)
                    plane += 1
    assert_same_candidates(hd.dp_argmin(CAP), exp["cands"])
    hd.close()


@pytest.mark.parametrize("K,L", KL, ids=[f"K{k}L{l}" for k, l in KL])
def test_batch_of_two_frames(gpu_required, orc, K, L):
    """detect_batch of two real frames on the exact bank: the oracle's candidates, and frame 1's tables of the star component"""
    m = model_of("two", K, L)
    frames = [make_image(60 + i, *FRAME) for i in range(2)]
    m.thresh = thresh_from_oracle(orc, m, frames[0], 97.0)
    refs = [orc.detect(m, f, keep=True) for f in frames]
    assert sum(len(r[0]) for r in refs) > 10
    hd = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT)
    for got, ref in zip(hd.detect_batch(frames), refs):
        assert_same_candidates(got, ref[:3])
    fr = refs[1][4]
    desc = m.to_desc()
    for l in (0, fr.nlevels // 2, fr.nlevels - 1):
        Ix, Iy, Ik = orc.dp_min_level(desc, 1, fr.resp(l))[:3]
        plane = 0
        for p in range(1, m.nparts(1)):
            for pm in range(len(m.filterid[1][m.parentid[1][p]])):
                gx, gy, gk = hd.frame_dp_pointers(1, l, 1, p, pm, *FRAME)
                np.testing.assert_array_equal(gk, Ik[plane])
                np.testing.assert_array_equal(gx, Ix[plane])
                np.testing.assert_array_equal(gy, Iy[plane])
                plane += 1
    for r in refs:
        r[4].free()
    hd.close()


def test_person_model_on_one_frame(gpu_required, orc):
    m = make_person_model()
    im = make_image(77, 96, 80)
    m.thresh = thresh_from_oracle(orc, m, im, 98.0)
    heads, boxes, locs, _, fr = orc.detect(m, im, keep=True)
    assert len(heads) > 10
    hd = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT)
    hd.begin_frame(96, 80, 3)                     # (plans the frame: Handle.root sizes its arrays by the plan's geometry)
    assert_same_candidates(hd.detect(im), (heads, boxes, locs))
    for l in (0, fr.nlevels - 1):
        grv, gri = hd.root(l, 0)
        rv, ri = fr.root(l)
        np.testing.assert_array_equal(_bits(grv), _bits(rv[0] if rv.ndim == 3 else rv))
        np.testing.assert_array_equal(gri, ri[0] if ri.ndim == 3 else ri)
    fr.free()
    hd.close()
