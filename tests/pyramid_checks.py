"""The assertions of the definition tests, shared by the CPU file (oracle) and the GPU file (kernels): `got` is whatever is under test,
everything it is compared with comes from tests/hog_ref.py and tests/pyramid_ref.py.  Each check prints the figure it asserts on."""
import numpy as np

from tests.hog_ref import excused_cells, float_bound, hog_def
from tests.pyramid_ref import pyrdown_def, pyrdown_float_bound, resize_def, resize_float_bound, resize_u8_bound

F64_TOL = 1e-12        # double against double: only the order of the additions differs.  A cell's bin sums <= 4 sbin^2 = 256 votes of
                       # magnitude <= 65535 sqrt(2) * 2 (16-bit), relative error <= 256 * 2^-53 = 3e-14 of a value that the normalisation
                       # brings to <= 0.4 (<= 0.85 for the texture sums): <= 3e-14 absolute, 30 times below the tolerance
EXCUSED_CAP = 0.001    # T = float on wide depths: at most 0.1 % of a frame's cells may be touched by excused pixels


def check_hog(got, im, sbin, label="", ref=None, **wrong):
    """`got` [ch, cw, 32] of dtype float64 (T = double: <= 1e-12, nothing excluded) or float32 (T = float: hog_ref.float_bound; nothing
    excluded for 8-bit images, cells excused by hog_ref.excused_cells for the other depths, at most EXCUSED_CAP of them)."""
    ref3 = hog_def(im, sbin, details=True, **wrong) if ref is None else ref
    feat, margin, det = ref3
    assert got.shape == feat.shape, (label, got.shape, feat.shape)
    if feat.size == 0:
        return 0.0
    d = np.abs(got.astype(np.float64) - feat)
    if got.dtype == np.float64:
        worst = float(d.max())
        print(f"[hog f64] {label}: worst |got - def| = {worst:.3e} (tol {F64_TOL:.0e})")
        assert worst <= F64_TOL, (label, worst)
        return worst
    b_hist, b_tex = float_bound(sbin)
    mask = np.zeros(feat.shape[:2], bool)
    if np.asarray(im).dtype == np.uint8:
        # exact dots are integer multiples of 1e-4 (uu, vv have four decimals, dx, dy are integers): two different ones are >= 1e-4 apart
        nz = margin[margin > 1e-9]
        assert nz.size == 0 or nz.min() >= 1e-4 - 1e-9, (label, nz.min())
    else:
        mask, nbad = excused_cells(margin, det, feat.shape[:2])
        frac = mask.mean()
        print(f"[hog f32] {label}: {nbad} near-tie pixels excuse {int(mask.sum())} of {mask.size} cells ({100 * frac:.3f} %)")
        assert frac <= EXCUSED_CAP, (label, frac)
    keep = ~mask
    w_hist = float(d[..., :27][keep].max()) if keep.any() else 0.0
    w_tex = float(d[..., 27:][keep].max()) if keep.any() else 0.0
    print(f"[hog f32] {label}: worst |got - def| = {w_hist:.3e} (bound {b_hist:.2e}) features 0..26, {w_tex:.3e} (bound {b_tex:.2e}) texture")
    assert w_hist <= b_hist and w_tex <= b_tex, (label, w_hist, b_hist, w_tex, b_tex)
    return max(w_hist, w_tex)


def _range(im):
    return float(np.abs(np.asarray(im).astype(np.float64)).max())


def check_pyrdown(got, im, label="", **wrong):
    """8/16-bit: got == floor(def + 0.5) on every pixel ((sum + 128) >> 8 IS that, in integers).  float / double: within
    pyrdown_float_bound of the definition."""
    im = np.asarray(im)
    d = pyrdown_def(im, **wrong)
    assert got.shape == d.shape and got.dtype == im.dtype, (label, got.shape, d.shape, got.dtype)
    if im.dtype.kind == "u":
        want = np.floor(d + 0.5).astype(im.dtype)
        nbad = int((got != want).sum())
        print(f"[pyrDown {im.dtype}] {label}: {nbad} pixels differ from floor(def + 0.5)")
        assert nbad == 0, (label, nbad)
        return 0.0
    b = pyrdown_float_bound(_range(im), im.dtype == np.float64)
    worst = float(np.abs(got.astype(np.float64) - d).max())
    print(f"[pyrDown {im.dtype}] {label}: worst |got - def| = {worst:.3e} (bound {b:.2e})")
    assert worst <= b, (label, worst, b)
    return worst


def check_resize(got, im, label="", **wrong):
    """8-bit: within resize_u8_bound (< 1 grey level) of the exact bilinear value.  16-bit: the float path's bound plus the 0.5 of the final
    cvRound.  float / double: resize_float_bound."""
    im = np.asarray(im)
    oh, ow = got.shape[:2]
    h, w = im.shape[:2]
    d = resize_def(im, ow, oh, **wrong)
    assert got.shape == d.shape and got.dtype == im.dtype, (label, got.shape, d.shape, got.dtype)
    if im.dtype == np.uint8:
        b = resize_u8_bound(max(w, h, ow, oh))
        assert b < 1.0, b
    else:
        b = resize_float_bound(_range(im), ow, oh, w, h, im.dtype == np.float64) + (0.5 if im.dtype == np.uint16 else 0.0)
    worst = float(np.abs(got.astype(np.float64) - d).max())
    print(f"[resize {im.dtype}] {label} {w}x{h} -> {ow}x{oh}: worst |got - def| = {worst:.4g} (bound {b:.4g})")
    assert worst <= b, (label, worst, b)
    return worst


def check_geometry(got, want, label=""):
    assert got["nlevels"] == want["nlevels"], (label, got["nlevels"], want["nlevels"])
    for k in ("img_w", "img_h", "cell_w", "cell_h", "scales"):
        assert np.array_equal(np.asarray(got[k]), want[k]), (label, k, got[k], want[k])
