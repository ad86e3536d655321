"""Width of the distance transform's pointer planes on the device: bytes while every line of the plan has byte links (a stride <= 256, at
most 254 elements: k_dt_pass's own index type), int16 as soon as one line is longer — one width for the whole plan, the public entries
keep int32 either way.  Both sides of the boundary, against the oracle bit for bit:

* pbd_dt2d on maps whose lines have 253, 254 (the last byte plan) and 255 elements (the first 16-bit plan: its short lines keep 16 bits
  too), in each direction and in both, under a quadratic weak enough (a = -0.006) that a peak at the far end of a line is every output's
  pointer: the largest index a plane can hold is stored, 253 in a byte, 254 in 16 bits;
* a detector frame whose first level is 253, 254 and 255 cells wide — and high —: Ix / Iy / Ik from pbd_get_dp_pointers and
  pbd_get_frame_dp_pointers, the back-tracked part locations, and the round trip pbd_get_dp_pointers -> pbd_set_dp_pointers ->
  pbd_dp_argmin, which must give the same candidates again."""
import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_tree_model_k

pytestmark = pytest.mark.gpu

LENS = (253, 254, 255)
SHORT = 12
A, CAP = -0.006, 4096


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _map(rng, rows, cols, far):
    """small integers; `far`: a peak at the far end of every line of both passes (the last column, the last row), else at the near end"""
    a = rng.integers(-4, 5, (rows, cols)).astype(np.float32)
    if far:
        a[:, -1] += 1000.0
        a[-1, :] += 1000.0
    else:
        a[:, 0] += 1000.0
        a[0, :] += 1000.0
    return a


@pytest.fixture(scope="module")
def dt_handle(gpu_required):
    hd = capi.Handle(make_tree_model_k([-1, 0], [1, 1], seed=5), conv_mode=capi.PBD_CONV_EXACT)
    yield hd
    hd.close()


@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("shape", ["long_rows", "long_columns", "both"])
def test_dt2d_across_the_width_boundary(dt_handle, orc, shape, n):
    rows, cols = {"long_rows": (SHORT, n), "long_columns": (n, SHORT), "both": (n, n)}[shape]
    rng = np.random.default_rng(1000 + n)
    for far, (osx, osy) in ((True, (0, 0)), (False, (0, 0)), (True, (3, -2)), (None, (-1, 2))):
        a = rng.integers(-4, 5, (rows, cols)).astype(np.float32) if far is None else _map(rng, rows, cols, far)
        want = orc.dt2d(a, A, 0.0, A, 0.0, osx, osy)
        got = dt_handle.dt2d(a, A, 0.0, A, 0.0, osx, osy)
        what = f"{rows} x {cols}, far {far}, offsets {(osx, osy)}"
        np.testing.assert_array_equal(got[1], want[1], err_msg="Ix " + what)
        np.testing.assert_array_equal(got[2], want[2], err_msg="Iy " + what)
        np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg="scores " + what)
        if far and (osx, osy) == (0, 0):          # the pointers do reach the last element of the long lines
            assert want[1].max() == cols - 1 and want[2].max() == rows - 1
            assert (want[1][:, 0] == cols - 1).all() and (want[2][0, :] == rows - 1).all()


def _model():
    """a 3-part star, 2 / 3 / 2 mixtures, every deformation the weak quadratic (no linear term), interval 2: a 1024 x 48 frame has 3 levels"""
    m = make_tree_model_k([-1, 0, 0], [2, 3, 2], seed=41, interval=2, quantised=True)
    m.defw = np.array(m.defw, np.float32)
    m.defw[:, [0, 2]] = np.float32(-A)
    m.defw[:, [1, 3]] = np.float32(0.0)
    return m


@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "tall"])
def test_frame_tables_backtracking_and_round_trip(gpu_required, orc, wide, n):
    m = _model()
    desc = m.to_desc()
    w, h = ((n + 2) * 4, 48) if wide else (48, (n + 2) * 4)
    geo = orc.geometry(w, h, 4, 2)
    assert (int(geo["cell_w"][0]) if wide else int(geo["cell_h"][0])) == n and geo["nlevels"] == 3
    rng = np.random.default_rng(50 + n)
    levels = []
    for l in range(geo["nlevels"]):
        H, W = int(geo["cell_h"][l]), int(geo["cell_w"][l])
        resp = rng.integers(-4, 5, (len(m.filtersw), H, W)).astype(np.float32)
        for p in (1, 2):                          # the children's planes peak at the far end of the long lines: their pointers go there
            for f in m.filterid[0][p]:
                if wide:
                    resp[f][:, -1] += 500.0
                else:
                    resp[f][-1, :] += 500.0
        levels.append((resp, orc.dp_min_level(desc, 0, resp)))
    Ix0, Iy0 = levels[0][1][0], levels[0][1][1]
    assert (Ix0.max() if wide else Iy0.max()) == n - 1
    vals = np.sort(np.concatenate([t[3].ravel() for _, t in levels]))
    m.thresh = float(np.nextafter(np.float32(vals[-60]), np.float32(-np.inf)))
    desc = m.to_desc()                            # (the threshold travels in the descriptor)
    want = [orc.dp_argmin_level(desc, 0, l, geo["scales"][l], t[3], t[4], t[0], t[1], t[2], capacity=CAP) for l, (_, t) in enumerate(levels)]
    want = tuple(np.concatenate([c[i] for c in want]) for i in range(3))
    assert 60 <= len(want[0]) < CAP, len(want[0])
    hd = capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT, max_candidates=CAP)
    hd.begin_frame(w, h, 3)
    assert np.array_equal(hd._geo["cell_w"], geo["cell_w"]) and np.array_equal(hd._geo["cell_h"], geo["cell_h"])
    for l, (resp, _) in enumerate(levels):
        for f in range(len(m.filtersw)):
            hd.set_level_response(l, f, resp[f])
    hd.dp_min()
    planes = [(p, pm) for p in range(1, m.nparts(0)) for pm in range(len(m.filterid[0][m.parentid[0][p]]))]
    got_tabs = []
    for l, (_, (Ix, Iy, Ik, rv, ri)) in enumerate(levels):
        grv, gri = hd.root(l, 0)
        np.testing.assert_array_equal(_bits(grv), _bits(rv), err_msg=f"rootv level {l}")
        np.testing.assert_array_equal(gri, ri, err_msg=f"rooti level {l}")
        for plane, (p, pm) in enumerate(planes):
            g1 = hd.dp_pointers(l, 0, p, pm)
            g2 = hd.frame_dp_pointers(0, l, 0, p, pm, w, h)
            for g in (g1, g2):
                np.testing.assert_array_equal(g[0], Ix[plane], err_msg=f"Ix level {l} part {p} parent mixture {pm}")
                np.testing.assert_array_equal(g[1], Iy[plane], err_msg=f"Iy level {l} part {p} parent mixture {pm}")
                np.testing.assert_array_equal(g[2], Ik[plane], err_msg=f"Ik level {l} part {p} parent mixture {pm}")
            got_tabs.append((l, p, pm, g1))
    first = hd.dp_argmin(CAP)

    def same(a, b):
        oa, ob = (np.lexsort((c[2][:, 0, 0], c[2][:, 0, 1], c[0]["level"])) for c in (a, b))
        assert len(a[0]) == len(b[0]) and a[0][oa].tobytes() == b[0][ob].tobytes()
        np.testing.assert_array_equal(a[2][oa], b[2][ob])         # the back-tracked part locations and mixtures
        np.testing.assert_array_equal(a[1][oa], b[1][ob])
    same(first, want)
    far = first[2][:, 1:3, 0 if wide else 1]
    assert far.max() == n - 1                                     # candidates whose parts sit on the last cell of the long lines
    for l, p, pm, g in got_tabs:                                  # the round trip: the tables read back are handed in again
        hd.set_dp_pointers(l, 0, p, pm, *g)
    same(hd.dp_argmin(CAP), want)
    hd.close()
