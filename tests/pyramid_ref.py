"""cv::resize(INTER_LINEAR), cv::pyrDown and the pyramid geometry of HOGFeatures<T>::pyramid (src/HOGFeatures.cpp:94-127) as
DEFINITIONS in float64 numpy: the published OpenCV 2.4 operations in exact arithmetic, with none of OpenCV's (or oracle/'s)
fixed-point or float intermediate formats.  The tests hold the oracle and the kernels to these within bounds DERIVED from
those formats (the *_bound functions below); nothing in a bound comes from what the code under test produced.

  resize   dst(d) = bilinear sample of src at (d + 0.5) * (n_src / n_dst) - 0.5 per axis, coordinates clamped to the image
           (samples left of pixel 0 / right of pixel n-1 are that pixel)
  pyrDown  dst(y, x) = sum_ij w_i w_j src(2y + i - 2, 2x + j - 2) / 256, w = [1 4 6 4 1], BORDER_REFLECT_101 (the border pixel
           is not repeated: -1 -> 1, n -> n - 2), size ((w + 1) / 2, (h + 1) / 2)
  geometry levels 0 .. interval-1: resize of the frame to cvRound(size * (float)(1 / sfactor^i)), sfactor = 2^(1/interval) in
           float; level j >= interval: pyrDown of level j - interval; nscales = 1 + floor(log(min(w, h) / (5 sbin)) / log(sfactor))
           in float; scales[i] = sfactor^i * sbin, scales[j] = 2 scales[j - interval]; cells = round(size / sbin) - 2

Each function has a deliberately WRONG switch (half_pixel=False, reflect101=False) for the power checks of the tests.
"""
import numpy as np

from tests.hog_ref import cells_of

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def _axis(n_src, n_dst, half_pixel=True):
    d = np.arange(n_dst, dtype=np.float64)
    f = (d + 0.5) * (n_src / n_dst) - 0.5 if half_pixel else d * (n_src / n_dst)
    f = np.clip(f, 0.0, n_src - 1.0)
    i0 = np.minimum(np.floor(f).astype(int), n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, f - i0


def resize_def(im, ow, oh, half_pixel=True):
    """exact bilinear resize -> float64 [oh, ow(, cn)] (NOT rounded to the pixel type)"""
    a = np.asarray(im).astype(np.float64)
    h, w = a.shape[:2]
    x0, x1, fx = _axis(w, ow, half_pixel)
    y0, y1, fy = _axis(h, oh, half_pixel)
    sh = (slice(None),) * 2 + (None,) * (a.ndim - 2)
    fxb, fyb = fx[None, :][sh], fy[:, None][sh]
    rows0 = a[y0][:, x0] * (1 - fxb) + a[y0][:, x1] * fxb
    rows1 = a[y1][:, x0] * (1 - fxb) + a[y1][:, x1] * fxb
    return rows0 * (1 - fyb) + rows1 * fyb


def _border(p, n, reflect101=True):
    p = np.asarray(p).copy()
    if n == 1:
        return np.zeros_like(p)
    for _ in range(8):                      # windows reach 2 pixels outside; tiny images need the reflection more than once
        if reflect101:
            p = np.where(p < 0, -p, p)
            p = np.where(p >= n, 2 * n - 2 - p, p)
        else:                               # BORDER_REFLECT: the border pixel IS repeated (-1 -> 0, n -> n - 1)
            p = np.where(p < 0, -p - 1, p)
            p = np.where(p >= n, 2 * n - 1 - p, p)
    assert ((p >= 0) & (p < n)).all()
    return p


def pyrdown_def(im, reflect101=True):
    """exact 5 x 5 Gaussian pyrDown -> float64 [(h + 1) // 2, (w + 1) // 2(, cn)] (NOT rounded to the pixel type)"""
    a = np.asarray(im).astype(np.float64)
    h, w = a.shape[:2]
    wt = (1.0, 4.0, 6.0, 4.0, 1.0)
    ys, xs = 2 * np.arange((h + 1) // 2), 2 * np.arange((w + 1) // 2)
    hor = sum(wt[j] * a[:, _border(xs + j - 2, w, reflect101)] for j in range(5))
    return sum(wt[i] * hor[_border(ys + i - 2, h, reflect101)] for i in range(5)) / 256.0


def geometry_def(w, h, sbin, interval):
    """dict like orc.geometry / Handle.geometry, or None where the frame is refused (fewer levels than `interval`: the reference
    would index scales_[j - interval] below zero).  float32 wherever the C++ computes in float."""
    f32 = np.float32
    sf = f32(np.power(2.0, np.float64(f32(1.0) / f32(interval))))            # pow(2.0f, 1.0f / (float)interval_) -> float
    mn = f32(min(w, h))
    r = f32(np.log(np.float64(mn / (f32(5.0) * f32(sbin))))) / f32(np.log(np.float64(sf)))   # float log / float log, in float
    n = int(f32(1.0) + np.floor(r))
    if n < interval:
        return None
    iw, ih, sc = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    for i in range(min(interval, n)):
        f = f32(f32(1.0) / np.power(np.float64(sf), i))                      # (float)(1.0f / pow(sfactor_, (int)i)): pow in double
        iw[i], ih[i] = int(np.rint(f32(w) * f)), int(np.rint(f32(h) * f))    # Size_<float> -> Size: cvRound (halves to even)
        sc[i] = f32(np.power(np.float64(sf), i) * sbin)
        for j in range(i + interval, n, interval):
            iw[j], ih[j] = (iw[j - interval] + 1) // 2, (ih[j - interval] + 1) // 2
            sc[j] = f32(2.0) * sc[j - interval]
    cw, ch = zip(*[cells_of(a, b, sbin) for a, b in zip(iw, ih)])
    return dict(nlevels=n, img_w=iw, img_h=ih, cell_w=np.array(cw, np.int32), cell_h=np.array(ch, np.int32), scales=sc)


# --------------------------------------------------------------------------------------------------------------------
# bounds, derived from the number formats of OpenCV 2.4's implementations (imgwarp.cpp, pyramids.cpp)
# --------------------------------------------------------------------------------------------------------------------
def resize_u8_bound(max_coord=2048):
    """|resize_8u - resize_def| in grey levels, derived from the FORMAT of OpenCV's 8-bit fixed-point path (no resize is run here):
         R_k = S a0 + S' a1            horizontal, 11-bit coefficient pair (a0, a1) = (round((1 - fx) 2048), round(fx 2048)), a0 + a1 = 2048
         out = (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2      vertical pair (b0, b1), b0 + b1 = 2048
      (a) the shifts.  Let T_k = R_k >> 4 and b_k T_k = 65536 m_k + r_k, 0 <= r_k < 65536.  Then q = m0 + m1 and the value the
          coefficients define is z = (b0 T0 + b1 T1) / 2^18 = q / 4 + (r0 + r1) / 2^18, the last term in [0, 0.5).  `(q + 2) >> 2` is
          q / 4 rounded to the nearest integer, halves up: out - q / 4 is 0, -1/4, +1/2 or +1/4.  So out - z lies in (-0.75, +0.5].
      (b) `>> 4` drops < 16 of R_k: < 16 (b0 + b1) / 2^22 = 0.0079 grey levels, downwards.
      (c) coefficients.  a1 = 2048 fx + d with |d| <= 0.5 and a0 = 2048 - a1, so the horizontal value is off by d (S' - S) / 2048:
          <= 0.5 * 255 / 2048 = 0.0623; the same for the vertical pair: 0.1245 for both axes.  (The pair sums to 2048 for every fx
          whose products do not fall within 2^-14 of a half: cvRound(x) + cvRound(2048 - x) = 2048 also at exact halves, halves go to even.)
      (d) coordinates.  fx = (float)((d + .5) scale - .5) is off by <= 2^-24 * max_coord, `fx -= sx` is exact; a fraction error e moves
          the sample by e * 255: 2^-24 * max_coord * 255 per axis (0.031 for coordinates below 2048).
    Worst case, all at one pixel and all downwards: 0.75 + 0.0079 + 0.1245 + 2 * 0.031 = 0.945 < 1.0, so a result that is one grey level
    off where the exact value is representable is seen.  (Upwards the bound would be 0.5 + 0.1245 + 0.062 = 0.69; one number is used.)"""
    return 0.75 + 16 * 2048 / 2.0 ** 22 + 2 * 0.5 * 255 / 2048 + 2 * U32 * max_coord * 255


def resize_float_bound(rng, ow, oh, sw, sh, f64=False):
    """|resize_32f/64f - resize_def| for images of value range `rng` (max |pixel|): OpenCV keeps the coordinates and the coefficients
    in FLOAT for every depth.  fx = (float)(coordinate) has error u * |coordinate| <= u * max(sw, sh), and fx -= sx is exact, so each
    fraction is off by <= u * max(sw, sh) (u = 2^-24); a fraction error e moves the sample by e * |S - S'| <= e * 2 rng; two axes.
    Arithmetic: 1 - fx (u), two products and an add per axis in float (3u each on values <= rng) — in double for CV_64F, negligible.
        2 * (u * max(sw, sh) * 2 rng) + (f64 ? 0 : 8 u rng)"""
    m = float(max(sw, sh, ow, oh))
    return 2.0 * (U32 * m * 2.0 * rng) + (16 * U64 * rng if f64 else 8.0 * U32 * rng)


def pyrdown_float_bound(rng, f64=False):
    """|pyrDown_32f/64f - pyrdown_def|: per pass 5 taps = 3 multiplies and 4 adds, two passes and the final * (1/256) (exact): fewer than
    10 multiply-adds on partial sums <= 16 rng resp. 256 rng before the scale, each rounding u relative: <= 10 u rng."""
    return 10.0 * (U64 if f64 else U32) * rng
