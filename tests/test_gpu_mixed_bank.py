"""Filter banks with a size per filter (pbd_create_sized): parity with the oracle's stage functions composed per size group.

The oracle's detect() and to_desc() are uniform-only, so the expected results are built from its stage functions:
features from a uniform stand-in model (same tree, defs, biases and filter ids, dummy 5 x 5 filters: HOG does not
depend on the filters), responses from orc.pdf_level once per size group, the DP from orc.dp_min_level (which reads
responses by filter id only) and the back-tracking from orc.dp_argmin_level run once per distinct filter row count —
a part's box is taken from the run whose kh is the rows of the filter of the mixture the part chose."""
import copy
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_mixed_person_model, make_person_model, make_voc_like_model
from tests.util import assert_candidates_equal, thresh_from_oracle

pytestmark = pytest.mark.gpu


def _standin(model, kh, kw):
    m = copy.copy(model)
    m.filtersw = [np.zeros((kh, kw * model.flen), np.float32) for _ in model.filtersw]
    m._keep = []
    return m


def _standin_desc(model, kh, kw):
    """(desc, owner): the descriptor points into arrays the stand-in model keeps alive — hold `owner` while the desc is used."""
    st = _standin(model, kh, kw)
    return st.to_desc(), st


def _groups(model):
    g = {}
    for n, (kh, kw) in enumerate(model.filter_sizes().tolist()):
        g.setdefault((kh, kw), []).append(n)
    return g


def _oracle_responses(orc, model, feat, dtype):
    H, W, _ = feat.shape
    resp = np.zeros((len(model.filtersw), H, W), dtype)
    for idx in _groups(model).values():
        resp[idx] = orc.pdf_level(feat, [model.filtersw[i] for i in idx], dtype)
    return resp


class Composed:
    """The oracle's pipeline for a mixed bank: features (stand-in detect), responses per size group, DP, back-tracking."""

    def __init__(self, orc, model, im, dtype=np.float32):
        self.orc, self.model, self.dtype = orc, model, np.dtype(dtype)
        st = _standin(model, 5, 5)
        st.thresh = -1e30
        _, _, _, _, fr = orc.detect(st, im, capacity=1, keep=True, dtype=dtype)
        self.dims = fr.dims
        self.feat = [fr.feat(l) for l in range(fr.nlevels)]
        fr.free()
        self.resp = [_oracle_responses(orc, model, f, dtype) if f.size else None for f in self.feat]

    def root_values(self, resp=None):
        resp = resp or self.resp
        desc, owner = _standin_desc(self.model, 5, 5)
        return np.concatenate([self.orc.dp_min_level(desc, c, r, dtype=self.dtype)[3].ravel()
                               for r in resp if r is not None for c in range(self.model.ncomponents)])

    def candidates(self, resp=None):
        """(heads, boxes, locs) in the library's order: level, component, row-major root location."""
        orc, m, dt = self.orc, self.model, self.dtype
        resp = resp or self.resp
        rows = sorted({kh for kh, _ in m.filter_sizes().tolist()})
        dmin, owner = _standin_desc(m, 5, 5)
        descs = {kh: _standin_desc(m, kh, kh) for kh in rows}
        fsz = m.filter_sizes()
        H, B, L = [], [], []
        for l, r in enumerate(resp):
            if r is None:
                continue
            for c in range(m.ncomponents):
                Ix, Iy, Ik, rv, ri = orc.dp_min_level(dmin, c, r, dtype=dt)
                runs = {kh: orc.dp_argmin_level(d, c, l, self.dims[l][4], rv, ri, Ix, Iy, Ik, dtype=dt) for kh, (d, _) in descs.items()}
                h0, b0, l0 = runs[rows[0]]
                b = b0.copy()
                for i in range(len(h0)):
                    for p in range(m.nparts(c)):
                        kh = int(fsz[m.filterid[c][p][l0[i, p, 2]]][0])
                        b[i, p] = runs[kh][1][i, p]
                H.append(h0); B.append(b); L.append(l0)
        mp = m.max_parts
        if not H:
            return (np.zeros(0, capi.HEAD_DTYPE), np.zeros((0, mp, 4), np.int32), np.zeros((0, mp, 3), np.int32))
        return np.concatenate(H), np.concatenate(B), np.concatenate(L)


def _set_thresh(comp, q=99.7):
    comp.model.thresh = float(np.float32(np.percentile(comp.root_values(), q)))


def _model(kind):
    if kind == "voc":
        return make_voc_like_model(seed=11)
    return make_mixed_person_model(seed=5, K=2)


def _gpu_responses(h, comp):
    return [None if f.size == 0 else np.stack([h.level_response(l, n) for n in range(len(comp.model.filtersw))])
            for l, f in enumerate(comp.feat)]


CASES = [("voc", 640, 480, 3), ("voc", 320, 240, 1), ("person", 320, 240, 3), ("person", 320, 240, 1)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,w,hgt,cn", CASES)
def test_mixed_bank_exact_bit_identical(gpu_required, orc, kind, w, hgt, cn, dtype):
    m = _model(kind)
    assert not m.is_uniform()
    im = make_image(3, w, hgt, cn)
    comp = Composed(orc, m, im, dtype)
    _set_thresh(comp)
    ref = comp.candidates()
    assert len(ref[0]) > 0
    h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype)
    assert [h.filter_size(n) for n in range(len(m.filtersw))] == [tuple(s) for s in m.filter_sizes().tolist()]
    assert_candidates_equal(h.detect(im), ref)
    h.pyramid(im)
    h.pdf()
    for l, r in enumerate(comp.resp):
        if r is not None:
            for n in range(len(m.filtersw)):
                np.testing.assert_array_equal(h.level_response(l, n), r[n], err_msg=f"level {l} filter {n}")
    h.close()


@pytest.mark.parametrize("kind", ["voc", "person"])
@pytest.mark.parametrize("mode,dtype", [(capi.PBD_CONV_AUTO, np.float32), (capi.PBD_CONV_MFMA, np.float32),
                                        (capi.PBD_CONV_MFMA, np.float64), (capi.PBD_CONV_SPLIT_F16, np.float32)])
def test_mixed_bank_fast_modes(gpu_required, orc, kind, mode, dtype):
    m = _model(kind)
    im = make_image(4, 320, 240, 3)
    comp = Composed(orc, m, im, dtype)
    _set_thresh(comp)
    h = capi.Handle(m, conv_mode=mode, dtype=dtype)
    if mode == capi.PBD_CONV_AUTO:
        assert h.conv_mode == capi.PBD_CONV_SPLIT   # >= 16 filters, float handle
    got = h.detect(im)
    h.pyramid(im)
    h.pdf()
    gresp = _gpu_responses(h, comp)
    worst = max(float(np.abs(g - r).max()) for g, r in zip(gresp, comp.resp) if r is not None)
    assert worst < 2e-5, worst
    # the DP and the back-tracking on the GPU's own responses: bit-identical
    assert_candidates_equal(got, comp.candidates(gresp))
    # against the fully composed oracle: the same roots up to threshold ties, scores within 1e-4
    ref = comp.candidates()
    key = lambda hd, lc: {(int(a["level"]), int(a["component"]), int(b[0, 0]), int(b[0, 1])): float(a["score"]) for a, b in zip(hd, lc)}
    kg, kr = key(got[0], got[2]), key(ref[0], ref[2])
    common = set(kg) & set(kr)
    assert len(common) >= max(len(kr) - max(2, len(kr) // 10), 1)
    assert max(abs(kg[k] - kr[k]) for k in common) < 1e-4
    h.close()


def test_uniform_sized_bank_is_the_uniform_handle(gpu_required, orc):
    """pbd_create_sized with every filter 5 x 5 gives the bytes of pbd_create: single frames, batches, graph replay."""
    m = make_person_model(seed=9, K=2)
    frames = [make_image(s, 320, 240, 3) for s in range(3)]
    m.thresh = thresh_from_oracle(orc, m, frames[0], 99.9)
    a = capi.Handle(m, graph=1, max_candidates=32768)
    b = capi.Handle(m, graph=1, sized=True, max_candidates=32768)
    assert b.fsize is not None and a.conv_mode == b.conv_mode
    for _ in range(2):   # the second pass replays the captured graphs
        for x, y in zip(a.detect_batch(frames, capacity=32768), b.detect_batch(frames, capacity=32768)):
            assert_candidates_equal(x, y)
            assert len(x[0]) > 0
    assert_candidates_equal(a.detect(frames[0], capacity=32768), b.detect(frames[0], capacity=32768))
    a.close(); b.close()


def test_mixed_bank_other_entry_points(gpu_required, orc, tmp_path):
    """Batches with graph replay, a two-member pbd_group on one GPU and the C++ demo on the reference's XML format give the
    candidates of single-frame pbd_detect_u8."""
    m = make_voc_like_model(seed=12)
    frames = [make_image(s, 320, 240, 3) for s in (5, 6)]
    comp = Composed(orc, m, frames[0])
    _set_thresh(comp)
    h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT)
    single = [h.detect(f) for f in frames]
    assert_candidates_equal(single[0], comp.candidates())
    hg = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, graph=1)
    for _ in range(2):
        for x, y in zip(hg.detect_batch(frames), single):
            assert_candidates_equal(x, y)
    g = capi.Group(m, [0, 0], gather=capi.PBD_GATHER_HOST, conv_mode=capi.PBD_CONV_EXACT)
    for x, y in zip(g.detect_batch(frames), single):
        assert_candidates_equal(x, y)
    g.close(); hg.close(); h.close()
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "host", "pbd_demo")
    m.save_filestorage(str(tmp_path / "model.xml"))
    frames[0].tofile(str(tmp_path / "im.raw"))
    heads, boxes, _ = orc.candidates_sort(*single[0])
    out = subprocess.run([exe, str(tmp_path / "model.xml"), str(tmp_path / "im.raw"), "320", "240", "3"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == f"Number of candidates: {len(heads)}" and len(heads) > 0
    for ln, hd, b in zip(lines[1:], heads, boxes):
        tok = ln.split()
        assert np.float32(float(tok[0])) == hd["score"] and int(tok[2]) == hd["level"]
        got = np.array([[int(v) for v in t.split(",")] for t in tok[3:]])
        np.testing.assert_array_equal(got, b[: len(got)])


def test_mixed_bank_boxes_use_rows_on_both_axes(gpu_required, orc):
    """include/Parts.hpp:185-187: xsize() and ysize() both return the filter's rows — a 6 x 4 or 5 x 8 root gets square boxes."""
    m = make_voc_like_model(seed=11)
    im = make_image(3, 320, 240, 3)
    _set_thresh(Composed(orc, m, im), 99.5)
    h = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT)
    heads, boxes, locs = h.detect(im)
    assert len(heads) > 0
    scales = h.geometry(320, 240)["scales"]
    fs = m.filter_sizes()
    seen_nonsquare = False
    for hd, b, lc in zip(heads, boxes, locs):
        c = int(hd["component"])
        for p in range(m.nparts(c)):
            kh, kw = fs[m.filterid[c][p][lc[p, 2]]]
            assert b[p, 2] == b[p, 3], (b[p], kh, kw)
            seen_nonsquare |= kh != kw
            assert b[p, 2] == int(np.rint(np.float32(kh) * np.float32(scales[hd["level"]]))) - 1
    assert seen_nonsquare
    h.close()
