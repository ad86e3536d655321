"""Virtual positives without a GPU (include/pbd_c.h "virtual positives"): pbd_rotate_geometry, pbd_map_rotate_points, pbd_flip_points and
pbd_augment_host_u8 against tests/augment_ref.py, the numpy restatement of the definition and of matlab/learning/map_rotate_points.m,
in bits; image and keypoints against each other, independently of the restatement; every refusal; and the Python helpers
augment_positives and train_model(mirror=, degrees=) with their device routes injected."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import partsbaseddetector_amd as pkg
from partsbaseddetector_amd import capi
from partsbaseddetector_amd.augment import augment_positives
from partsbaseddetector_amd.train import train_model
from tests import augment_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbd_rotate_geometry", "pbd_map_rotate_points", "pbd_flip_points", "pbd_augment_host_u8", "pbd_augment_u8", "pbd_augment_dev_u8",
         "pbd_augment_last_error", "pbd_qp_write_warped_dev_u8")


# ---- symbols ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(tmp_path):
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"\b(pbd_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in capi.EXPORTS and hasattr(L, name), name
    assert L.pbd_abi_version() == 5 == capi.PBD_ABI_VERSION and "#define PBD_ABI_VERSION 5" in header
    for name in ("rotate_geometry", "map_rotate_points", "flip_points", "augment_host", "augment", "augment_dev", "DeviceFrame", "pbd_augment_op"):
        assert hasattr(capi, name), name
    assert hasattr(capi.QpCache, "write_warped_dev") and pkg.augment_positives is augment_positives
    for text, value in (("PBD_ROT_ORI2NEW 0", capi.PBD_ROT_ORI2NEW), ("PBD_ROT_NEW2ORI 1", capi.PBD_ROT_NEW2ORI), ("PBD_ROT_NEAREST 0", capi.PBD_ROT_NEAREST),
                        ("PBD_ROT_BILINEAR 1", capi.PBD_ROT_BILINEAR), ("PBD_AUGMENT_MAX_OPS 64", capi.PBD_AUGMENT_MAX_OPS),
                        ("PBD_AUGMENT_MAX_SIDE 16384", capi.PBD_AUGMENT_MAX_SIDE)):
        assert f"#define {text}" in header and int(text.split()[1]) == value
    # the op struct's layout: the binding's against the compiler's
    op = capi.pbd_augment_op
    assert C.sizeof(op) == 24 and (op.flip.offset, op.method.offset, op.deg.offset, op.rotate.offset, op.reserved.offset) == (0, 4, 8, 16, 20)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbd_c.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(pbd_augment_op), '
                   'offsetof(pbd_augment_op, method), offsetof(pbd_augment_op, deg), offsetof(pbd_augment_op, rotate), offsetof(pbd_augment_op, reserved)); return 0;}\n')
    import subprocess
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)]).split() == [b"24", b"4", b"8", b"16", b"20"]


# ---- geometry --------------------------------------------------------------------------------------------------------------------------
def test_geometry_equals_the_restatement_in_bits():
    for w, hgt in ref.SIZES:
        for deg in ref.ANGLES:
            g = capi.rotate_geometry(w, hgt, deg)
            rows, cols, m = ref.geometry(w, hgt, deg)
            assert (g["h"], g["w"]) == (rows, cols), (w, hgt, deg)
            assert g["m"].tobytes() == np.array(m, np.float64).tobytes(), (w, hgt, deg)


@pytest.mark.parametrize("w, hgt, deg, canvas", [(640, 480, 15.0, (633, 745)), (640, 480, 0.0, (481, 641)), (37, 29, 7.5, (37, 41)), (37, 29, 0.0, (29, 37))])
def test_pinned_canvases(w, hgt, deg, canvas):
    g = capi.rotate_geometry(w, hgt, deg)
    assert (g["h"], g["w"]) == canvas
    assert g["h"] % 2 == 1 and g["w"] % 2 == 1        # 2 * hiB + 1


def test_the_files_quirks_are_kept():
    # hiB is hiA rounded up to an even number.  At 0 degrees an even side n has hiA = (n - 1) / 2 off the grid: the canvas is larger
    # (40 -> 2 * 20 + 1, 30 -> 2 * 16 + 1) and the image sits a fraction of a pixel off it; an odd side keeps its size only where
    # (n - 1) / 2 is even (37 and 29 do, 31 does not)
    g = capi.rotate_geometry(40, 30, 0.0)
    assert (g["h"], g["w"]) == (33, 41) and g["m"][2:].tolist() == [14.5, 19.5, 16.0, 20.0]
    assert capi.map_rotate_points([[0.0, 0.0]], 40, 30, 0.0).tolist() == [[0.5, 1.5]]
    g = capi.rotate_geometry(41, 31, 0.0)
    assert (g["h"], g["w"]) == (33, 41)
    # at +-90, 180 and 360 degrees cos and sin are not exactly 0 / +-1: the extent is hiA (14 or 18, both even) give or take an ulp,
    # so hiB is hiA or the next even number: a side of the turned frame, or four more; never less
    for deg, (sw, sh) in ((90.0, (29, 37)), (-90.0, (29, 37)), (180.0, (37, 29)), (360.0, (37, 29))):
        g = capi.rotate_geometry(37, 29, deg)
        assert g["w"] - sw in (0, 4) and g["h"] - sh in (0, 4), (deg, g)
    # the documented case, 37 x 29 at 90 degrees: cos(pi / 2) in double is 6.1e-17 and sin is 1.  Columns: |14 + 18 cos| = 14 + 1.1e-15
    # rounds to one ulp (1.8e-15) above 14, so hiB_c = ceil(7.000...1) * 2 = 16 and the canvas has 33 columns, not 29.  Rows: 18 -+ 14 cos
    # moves 18 by 8.6e-16, below half its ulp (3.6e-15): exactly 18, 37 rows
    g = capi.rotate_geometry(37, 29, 90.0)
    assert (g["h"], g["w"]) == (37, 33) and g["m"][4:].tolist() == [18.0, 16.0]


# ---- point maps ------------------------------------------------------------------------------------------------------------------------
def _points(w, hgt, n=40, seed=1):
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-3, w + 3, n), rng.uniform(-3, hgt + 3, n)], axis=1)
    p[:4] = [[0, 0], [w - 1, 0], [0, hgt - 1], [(w - 1) / 2.0, (hgt - 1) / 2.0]]
    return p


def test_points_equal_the_restatement_in_bits():
    for w, hgt in ref.SIZES:
        pts = _points(w, hgt)
        for deg in ref.ANGLES:
            for d in (capi.PBD_ROT_ORI2NEW, capi.PBD_ROT_NEW2ORI):
                got = capi.map_rotate_points(pts, w, hgt, deg, d)
                assert got.tobytes() == ref.map_points(pts, w, hgt, deg, d).tobytes(), (w, hgt, deg, d)
    # a point at hiA maps to hiB: the frame in which pixel index k sits at coordinate k
    g = capi.rotate_geometry(37, 29, 15.0)
    assert capi.map_rotate_points([[18.0, 14.0]], 37, 29, 15.0).tolist() == [[g["m"][5], g["m"][4]]]


def test_new2ori_inverts_ori2new():
    """about ten operations at 2^-53 * 2^15 each stay below 1e-10: the bound 1e-9 holds for coordinates up to 16384"""
    worst = 0.0
    for w, hgt in ((640, 480), (11000, 11000), (11500, 4000), (37, 29)):      # canvases of up to about 15 300 a side
        pts = _points(w, hgt, 200, seed=w)
        for deg in (7.5, -15.0, 33.0):
            back = capi.map_rotate_points(capi.map_rotate_points(pts, w, hgt, deg), w, hgt, deg, capi.PBD_ROT_NEW2ORI)
            err = float(np.abs(back - pts).max())
            worst = max(worst, err)
            assert err < 1e-9, (w, hgt, deg, err)
    print("worst round trip", worst)


def test_flip_points():
    """twice with an involutive mirror is the identity in bits on keypoints of the pixel grid and its eighths, where w - 1 - x is exact
    (an arbitrary double below w - 1 loses its low bits in the first subtraction: no definition of the mirror could return them)"""
    pts = np.round(_points(37, 29, 6) * 8.0) / 8.0
    mirror = [1, 0, 2, 5, 4, 3]                       # an involution
    once = capi.flip_points(pts, 37, mirror)
    assert once.tobytes() == ref.flip_points(pts, 37, mirror).tobytes()
    assert capi.flip_points(once, 37, mirror).tobytes() == pts.tobytes()
    assert capi.flip_points(pts, 37).tobytes() == ref.flip_points(pts, 37).tobytes()
    ints = np.array([[3.0, 4.0], [5.0, 6.0]])
    assert capi.flip_points(ints, 37, [1, 0]).tolist() == [[31.0, 6.0], [33.0, 4.0]]
    for bad in ([0, 0, 2, 3, 4, 5], [0, 1, 2, 3, 4, 6], [-1, 1, 2, 3, 4, 5]):
        with pytest.raises(capi.PbdError) as e:
            capi.flip_points(pts, 37, bad)
        assert e.value.code == capi.PBD_ERR_ARG and "permutation" in str(e.value)


# ---- the host image against the restatement ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_grid():
    """{(w, hgt, cn): (frame, specs, [the host function's canvases])}: computed once, through padded input and output strides"""
    out = {}
    for w, hgt, cn in ref.FRAMES:
        im = ref.padded(ref.frame(w, hgt, cn))
        assert not im.flags["C_CONTIGUOUS"] and im.strides[0] == w * cn + 5
        specs = ref.grid_specs()
        ops = capi.augment_ops(specs)
        canv = [capi.augment_canvas(w, hgt, ops[i]) for i in range(len(specs))]
        bufs = [np.full((r, c * cn + 7), 0x5A, np.uint8) for r, c in canv]
        got = capi.augment_host(im, specs, outs=bufs)
        out[w, hgt, cn] = (im, specs, got, bufs, canv)
    return out


def test_host_image_equals_the_restatement_in_bytes(host_grid):
    for (w, hgt, cn), (im, specs, got, bufs, canv) in host_grid.items():
        for (flip, deg, method), g, b, (r, c) in zip(specs, got, bufs, canv):
            want = ref.augment(im, flip, deg, method)
            assert g.shape == want.shape and np.array_equal(g, want), ((w, hgt, cn), (flip, deg, method), np.argwhere(g != want)[:3])
            assert (b[:, c * cn:] == 0x5A).all(), "bytes behind a canvas row were written"
        assert (np.asarray(im).base[:, w * cn:] == 0xA5).all()


def test_zero_degrees_on_the_odd_frame_returns_the_source(host_grid):
    """37 x 29: (n - 1) / 2 is even on both axes, so the 0-degree canvas is the frame's and every source coordinate is an integer"""
    im, specs, got, _, _ = host_grid[37, 29, 3]
    zero = [g for (flip, deg, _), g in zip(specs, got) if deg == 0.0 and not flip]
    assert len(zero) == 2 and all(np.array_equal(g, im) for g in zero)      # nearest and bilinear
    assert np.array_equal(got[0], np.asarray(im)[:, ::-1])                 # the mirror alone


def test_one_call_equals_one_call_per_op(host_grid):
    im, specs, got, _, _ = host_grid[40, 30, 1]
    for sp, g in list(zip(specs, got))[::5]:
        assert np.array_equal(capi.augment_host(np.ascontiguousarray(im), [sp])[0], g), sp


# ---- image and points agree (independent of the restatement) -----------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [15.0, -15.0, 90.0])
def test_a_bright_block_lands_where_its_keypoint_is_mapped(deg):
    """nearest sampling moves a pixel centre by at most half a pixel per axis, and a 3 x 3 block cannot be missed: the centroid of the
    bright output pixels lies within one pixel per axis of the mapped keypoint"""
    w, hgt = 41, 31
    for kx, ky in ((10, 8), (30, 20), (20, 15), (5, 25)):
        im = np.zeros((hgt, w), np.uint8)
        im[ky - 1:ky + 2, kx - 1:kx + 2] = 255
        out = capi.augment_host(im, [(False, deg, "nearest")])[0]
        ys, xs = np.nonzero(out)
        assert len(ys) >= 4
        px, py = capi.map_rotate_points([[kx, ky]], w, hgt, deg)[0]
        assert abs(xs.mean() - px) <= 1.0 and abs(ys.mean() - py) <= 1.0, (deg, (kx, ky), (xs.mean(), ys.mean()), (px, py))


def test_a_bright_block_lands_where_its_keypoint_is_mirrored():
    w, hgt = 41, 31
    pts = np.array([[10.0, 8.0], [30.0, 20.0]])
    im = np.zeros((hgt, w), np.uint8)
    im[7:10, 9:12] = 255                                   # the block of keypoint 0
    out = capi.augment_host(im, [(True, None)])[0]
    ys, xs = np.nonzero(out)
    fx, fy = capi.flip_points(pts, w, [1, 0])[1]           # the mirrored frame's part 1 is the original's part 0
    assert len(ys) == 9 and abs(xs.mean() - fx) <= 1.0 and abs(ys.mean() - fy) <= 1.0
    # and the mirror followed by a rotation: the mirrored keypoint carried through the map
    out = capi.augment_host(im, [(True, 15.0, "nearest")])[0]
    ys, xs = np.nonzero(out)
    px, py = capi.map_rotate_points([[fx, fy]], w, hgt, 15.0)[0]
    assert abs(xs.mean() - px) <= 1.0 and abs(ys.mean() - py) <= 1.0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _raw(fn, lead, im, w, hgt, cn, stride, ops, nops, bufs, strides):
    ptrs = (C.c_void_p * max(len(bufs), 1))(*[b.ctypes.data for b in bufs]) if bufs is not None else None
    st = None if strides is None else np.ascontiguousarray(strides, np.int32)
    return fn(*lead, None if im is None else capi._vp(im), w, hgt, cn, stride, ops, nops, ptrs, None if st is None else capi._vp(st))


def _refusal_cases():
    """(name, code, text, overrides of the valid call)"""
    A, U = capi.PBD_ERR_ARG, capi.PBD_ERR_UNSUPPORTED
    nan_op, inf_op = capi.augment_ops([(False, float("nan"))]), capi.augment_ops([(False, float("inf"))])
    bad_method = capi.augment_ops([(False, 15.0, 2)])
    return [("null im", A, "NULL", dict(im=None)), ("null ops", A, "NULL", dict(ops=None)), ("null outs", A, "NULL", dict(bufs=None)),
            ("null strides", A, "NULL", dict(strides=None)), ("cn 2", A, "cn", dict(cn=2)), ("cn 4", A, "cn", dict(cn=4)),
            ("w 0", A, "w / hgt", dict(w=0)), ("hgt 0", A, "w / hgt", dict(hgt=0)), ("stride", A, "stride below", dict(stride=36)),
            ("nan", A, "not finite", dict(ops=nan_op)), ("inf", A, "not finite", dict(ops=inf_op)), ("method", A, "unknown method", dict(ops=bad_method)),
            ("nops 0", A, "nops", dict(nops=0)), ("nops 65", A, "nops", dict(nops=65)), ("out stride", A, "out_strides[0]", dict(strides=[40])),
            ("canvas", U, "16384", dict(w=16000, hgt=9000, stride=16000, ops=capi.augment_ops([(False, 45.0)])))]


def _refusals(fn, lead):
    im = ref.frame(37, 29, 1)
    for name, code, text, over in _refusal_cases():
        out = np.full((64, 64), 0x5A, np.uint8)
        kw = dict(im=im, w=37, hgt=29, cn=1, stride=37, ops=capi.augment_ops([(False, 15.0)]), nops=1, bufs=[out], strides=[64])
        kw.update(over)
        assert _raw(fn, lead, **kw) == code, name
        assert text in capi.lib().pbd_augment_last_error().decode(), (name, capi.lib().pbd_augment_last_error())
        assert (out == 0x5A).all(), name
    out = np.full((64, 64), 0x5A, np.uint8)       # a NULL output pointer among the ops
    ptrs = (C.c_void_p * 2)(out.ctypes.data, None)
    st = np.array([64, 64], np.int32)
    assert fn(*lead, capi._vp(im), 37, 29, 1, 37, capi.augment_ops([(True, None), (True, None)]), 2, ptrs, capi._vp(st)) == capi.PBD_ERR_ARG
    assert (out == 0x5A).all()


def test_host_refusals_leave_the_outputs_untouched():
    _refusals(capi.lib().pbd_augment_host_u8, ())


def test_device_entries_refuse_before_they_need_a_gpu():
    """the refusals come first, as pbd_cluster_parts': without a GPU a valid call answers PBD_ERR_HIP, with one it runs"""
    L = capi.lib()
    _refusals(L.pbd_augment_u8, (0,))
    _refusals(L.pbd_augment_dev_u8, (0,))
    import torch
    if not torch.cuda.is_available():
        im, out = ref.frame(37, 29, 1), np.full((29, 40), 0x5A, np.uint8)
        assert _raw(L.pbd_augment_u8, (0,), im, 37, 29, 1, 37, capi.augment_ops([(True, None)]), 1, [out], [40]) == capi.PBD_ERR_HIP
        assert (out == 0x5A).all()
        with pytest.raises(capi.PbdError) as e:
            capi.augment(im, [(True, None)])
        assert e.value.code == capi.PBD_ERR_HIP
    assert L.pbd_qp_write_warped_dev_u8(None, None, 1, 1, 1, 1, None, None, 0, 0, 0, 0.0, None, None) == capi.PBD_ERR_ARG


def test_point_and_geometry_refusals():
    A, U = capi.PBD_ERR_ARG, capi.PBD_ERR_UNSUPPORTED
    for call, code in ((lambda: capi.rotate_geometry(0, 5, 1.0), A), (lambda: capi.rotate_geometry(5, 0, 1.0), A),
                       (lambda: capi.rotate_geometry(5, 5, float("nan")), A), (lambda: capi.rotate_geometry(16000, 9000, 45.0), U),
                       (lambda: capi.rotate_geometry(5, 5, 1e308), U),
                       (lambda: capi.map_rotate_points([[1, 1]], 5, 5, 1.0, 2), A), (lambda: capi.map_rotate_points([[1, 1]], 5, 5, float("inf")), A),
                       (lambda: capi.flip_points([[1, 1]], 0), A)):
        with pytest.raises(capi.PbdError) as e:
            call()
        assert e.value.code == code
    L = capi.lib()
    out = np.full(2, 7.0)
    assert L.pbd_map_rotate_points(None, 1, 5, 5, 1.0, 0, capi._vp(out)) == A and L.pbd_flip_points(None, 1, 5, None, capi._vp(out)) == A
    assert out.tolist() == [7.0, 7.0]
    assert L.pbd_rotate_geometry(5, 5, 1.0, None, None, None) == capi.PBD_OK       # every output may be NULL


# ---- the Python helpers --------------------------------------------------------------------------------------------------------------------
def _positives(n=3, P=4, w=41, hgt=31):
    rng = np.random.default_rng(5)
    return [(ref.frame(w, hgt, 3, seed=i), np.stack([rng.uniform(1, w, P), rng.uniform(1, hgt, P)], axis=1)) for i in range(n)]


def test_augment_positives_order_counts_and_one_based_points():
    pos = _positives()
    mirror, degrees = [1, 0, 3, 2], (7.5, -15.0)
    routed = []

    def route(im, specs):
        routed.append(list(specs))
        return capi.augment_host(im, specs)

    out = augment_positives(pos, mirror=mirror, degrees=degrees, method="nearest", _route=route)
    n = len(pos)
    assert len(out) == n * 2 * 3 and len(routed) == n                  # one call per annotated image
    assert all(a is b for a, b in zip(out[:n], pos))                    # the originals, first and untouched
    w, hgt = 41, 31
    for i, (im, pts) in enumerate(pos):
        p0 = pts - 1.0
        fim, fpts = out[n + i]
        assert np.array_equal(fim, im[:, ::-1]) and fpts.tobytes() == (ref.flip_points(p0, w, mirror) + 1.0).tobytes()
        for a, deg in enumerate(degrees):
            for f, (src_im, src_p0) in enumerate(((im, p0), (im[:, ::-1], fpts - 1.0))):
                rim, rpts = out[2 * n + a * 2 * n + f * n + i]
                assert np.array_equal(rim, ref.augment(src_im, False, deg, ref.NEAREST)), (i, deg, f)
                assert rpts.tobytes() == (ref.map_points(src_p0, w, hgt, deg, ref.ORI2NEW) + 1.0).tobytes(), (i, deg, f)
    # a mirrored 1-based keypoint: x -> w + 1 - x
    assert np.allclose(out[n][1][:, 0], w + 1 - pos[0][1][mirror, 0], atol=1e-12)
    # the pieces alone, and nothing asked for: the very list
    assert len(augment_positives(pos, mirror=mirror, _route=route)) == 2 * n and len(augment_positives(pos, degrees=(5,), _route=route)) == 2 * n
    same = augment_positives(pos, _route=route)
    assert len(same) == n and all(a is b for a, b in zip(same, pos))


def _train_model_run(pos, **kw):
    got = {}

    def fake_cluster(deffeat, pa, k):
        got["def"] = np.asarray(deffeat).shape
        return dict(idx=np.zeros((len(pa), np.asarray(deffeat).shape[1]), np.int32))

    def fake_train(model, positives, negs, warp, **opts):
        got.setdefault("calls", []).append((positives, warp))
        return model, []

    def fake_augment(positives, **opts):
        got["augment"] = opts
        return augment_positives(positives, mirror=opts["mirror"], degrees=opts["degrees"], method=opts["method"], _route=capi.augment_host)

    train_model(pos, ["neg"], 1, [-1, 0, 0, 1], 4, tsize=(5, 5), _train=fake_train, _cluster=fake_cluster, _augment=fake_augment, **kw)
    return got


def test_train_model_hands_the_augmented_list_on():
    pos = _positives(n=3)
    mirror = [0, 2, 1, 3]
    got = _train_model_run(pos, mirror=mirror, degrees=(10.0,), augment_method="nearest")
    assert got["augment"] == dict(mirror=mirror, degrees=(10.0,), method="nearest", device=0, keep_on_device=True)
    want = augment_positives(pos, mirror=mirror, degrees=(10.0,), method="nearest", _route=capi.augment_host)
    assert got["def"] == (4, 12, 2)                                     # the clusters run over the augmented keypoints
    final = got["calls"][-1][0]
    assert len(final) == 12 and all(np.array_equal(f[0], w[0]) for f, w in zip(final, want))
    assert final[0][0] is pos[0][0]
    part0 = got["calls"][0][0]                                          # K = 1: every positive of the longer list trains part 0
    assert len(part0) == 12 and part0[5][0].shape == want[5][0].shape


def test_train_model_with_the_defaults_hands_on_the_list_it_got():
    pos = _positives(n=3)
    got = _train_model_run(pos)
    assert "augment" not in got and got["def"] == (4, 3, 2)
    assert all(len(c[0]) == 3 and all(it[0] is p[0] for it, p in zip(c[0], pos)) for c in got["calls"])


# ---- the C++ layer -------------------------------------------------------------------------------------------------------------------------
def test_cpp_layer_host_route(tmp_path):
    """pbd::augment(host = true), pbd::mapRotatePoints and pbd::flipPoints (tests/tools/augment_check.cpp) give the host functions' bytes
    and points and throw the header's refusal; ExampleCache::writeWarped from a pbd::DeviceFrame compiles"""
    im, lines = ref.cpp_check(tmp_path, os.path.dirname(capi.LIB_PATH), "host")
    ref.cpp_expect(im, lines, capi.augment_host, capi.map_rotate_points, capi.flip_points)
