"""HOG as a definition: what HOGFeatures<T>::features (src/HOGFeatures.cpp:168-341) computes, stated once in float64 numpy.

This is NOT the oracle restated: no loop nest of oracle/*.inc is reused, every step is a whole-array expression, and the
accumulation is numpy's (np.bincount), whose order is neither the C++'s nor features.cc's.  It is held to the compiled
MATLAB ancestor (oracle/ref_features, tests/golden/ref_hog_v1.npz) within 1e-12 by tests/test_pyramid_definition_cpu.py.

The definition, for an image of `cn` in {1, 3} channels, w x h pixels, bin size s:
  blocks  bw = round(w / s), bh = round(h / s) (halves away from zero); output (bh - 2) x (bw - 2) cells, never negative
  pixels  every (x, y) with 1 <= x <= bw*s - 2, 1 <= y <= bh*s - 2, READ at (min(x, w - 2), min(y, h - 2)): when
          round() went up, bw*s > w and the last columns are the clamped column again
  gradient central differences; colour: the channel with the largest dx^2 + dy^2, where interleaved channel 2 is the
          incumbent and channel 1, then channel 0, replace it only when STRICTLY greater
  bin     of the 18 values (+dot_0, -dot_0, +dot_1, -dot_1, ...), dot_o = uu[o] dx + vv[o] dy, the largest, the first
          one in that order on a tie; all <= 0 (no gradient): bin 0
  vote    |gradient| spread bilinearly over the four cells around ((x + .5)/s - .5, (y + .5)/s - .5); cells outside are dropped
  energy  E(cell) = sum_o (hist[o] + hist[o + 9])^2;  N(y, x) = E(y, x) + E(y, x+1) + E(y+1, x) + E(y+1, x+1)
  feature for output cell (y, x), c = hist(y + 1, x + 1), n1..n4 = 1 / sqrt(N + 1e-4) at (y+1, x+1), (y, x+1), (y+1, x), (y, x):
          0..17  0.5 * sum_k min(c[o] n_k, 0.2);  18..26  the same for c[o] + c[o + 9];
          27..30 0.2357 * sum_o min(c[o] n_k, 0.2) for k = 1..4;  31  zero

One quirk of the C++ that a "mathematical" reading misses and that this file therefore states: the pixel difference
`*(s + stride) - *(s - stride)` is evaluated in the PIXEL type's arithmetic before it becomes a T.  For 8- and 16-bit
pixels that is exact; for CV_32F images it is one IEEE float32 subtraction (rounded), also when T = double.
"""
import numpy as np

UU = np.array([1.0000, 0.9397, 0.7660, 0.5000, 0.1736, -0.1736, -0.5000, -0.7660, -0.9397])
VV = np.array([0.0000, 0.3420, 0.6428, 0.8660, 0.9848, 0.9848, 0.8660, 0.6428, 0.3420])
U32 = 2.0 ** -24          # unit roundoff of float32 (round to nearest)


def blocks_of(n, sbin):
    """round(n / sbin), halves away from zero, in integers"""
    return (2 * int(n) + int(sbin)) // (2 * int(sbin))


def cells_of(w, h, sbin):
    return max(blocks_of(w, sbin) - 2, 0), max(blocks_of(h, sbin) - 2, 0)


def _diff(a, b):
    """pixel difference in the pixel type's own arithmetic (module docstring), widened to float64"""
    if a.dtype == np.float32:
        return (a - b).astype(np.float64)              # one float32 subtraction
    return a.astype(np.float64) - b.astype(np.float64)  # exact for 8/16-bit, the double subtraction for CV_64F


def hog_def(im, sbin, swap_n2_n3=False, details=False):
    """features [ch, cw, 32] float64 and the per-pixel orientation margin [bh*s - 2, bw*s - 2] (winner's dot minus the
    runner-up's among the 18 signed dots; 0 where the pixel has no gradient).  details=True adds a dict with `absdot`
    (|uu dx| + |vv dy| summed at the winner's magnitude scale: |dx| + |dy| of the chosen channel), the four hist cells
    of every pixel (`iy`, `ix`) and the block counts.
    swap_n2_n3: the deliberately WRONG variant the power check of the tests uses (n2 and n3 exchanged)."""
    im = np.asarray(im)
    if im.dtype not in (np.uint8, np.uint16, np.float32, np.float64):
        im = im.astype(np.uint8)
    if im.ndim == 2:
        im = im[:, :, None]
    h, w, cn = im.shape
    assert cn in (1, 3)
    s = int(sbin)
    bw, bh = blocks_of(w, s), blocks_of(h, s)
    ow, oh = max(bw - 2, 0), max(bh - 2, 0)
    feat = np.zeros((oh, ow, 32))
    xs, ys = np.arange(1, bw * s - 1), np.arange(1, bh * s - 1)
    if ow == 0 or oh == 0 or len(xs) == 0 or len(ys) == 0:
        margin = np.zeros((max(len(ys), 0), max(len(xs), 0)))
        return (feat, margin, dict(absdot=margin.copy(), iy=ys, ix=xs, bw=bw, bh=bh)) if details else (feat, margin)
    assert w >= 3 and h >= 3, "the reference reads outside the image below 3 pixels"
    sx, sy = np.minimum(xs, w - 2), np.minimum(ys, h - 2)
    dx = _diff(im[np.ix_(sy, sx + 1)], im[np.ix_(sy, sx - 1)])          # [Y, X, cn]
    dy = _diff(im[np.ix_(sy + 1, sx)], im[np.ix_(sy - 1, sx)])
    v = dx * dx + dy * dy
    if cn == 3:
        pick = np.full(v.shape[:2], 2)
        best = v[..., 2].copy()
        for c in (1, 0):                                               # strictly greater replaces the incumbent
            m = v[..., c] > best
            pick[m] = c
            best[m] = v[..., c][m]
        gx = np.take_along_axis(dx, pick[..., None], 2)[..., 0]
        gy = np.take_along_axis(dy, pick[..., None], 2)[..., 0]
    else:
        gx, gy, best = dx[..., 0], dy[..., 0], v[..., 0]
    dots = gx[..., None] * UU + gy[..., None] * VV                      # [Y, X, 9]
    signed = np.stack([dots, -dots], axis=-1).reshape(dots.shape[:2] + (18,))   # visiting order +0, -0, +1, -1, ...
    k = np.argmax(signed, axis=-1)                                      # first maximum wins
    top2 = np.partition(signed, 16, axis=-1)[..., 16:]
    margin = top2[..., 1] - top2[..., 0]
    nograd = signed.max(axis=-1) <= 0
    bin_ = np.where(nograd, 0, k // 2 + 9 * (k % 2))
    margin = np.where(nograd, 0.0, margin)
    mag = np.sqrt(best)

    xp, yp = (xs + 0.5) / s - 0.5, (ys + 0.5) / s - 0.5
    ixp, iyp = np.floor(xp).astype(int), np.floor(yp).astype(int)
    vx0, vy0 = xp - ixp, yp - iyp
    hist = np.zeros(bh * bw * 18)
    for oy, wy in ((0, 1.0 - vy0), (1, vy0)):
        for ox, wx in ((0, 1.0 - vx0), (1, vx0)):
            cy, cx = iyp + oy, ixp + ox
            ok = ((cy >= 0) & (cy < bh))[:, None] & ((cx >= 0) & (cx < bw))[None, :]
            idx = (cy[:, None] * bw + cx[None, :]) * 18 + bin_
            wgt = wy[:, None] * wx[None, :] * mag
            hist += np.bincount(idx[ok], weights=wgt[ok], minlength=hist.size)
    hist = hist.reshape(bh, bw, 18)
    t = hist[..., :9] + hist[..., 9:]
    E = (t * t).sum(axis=-1)
    N = E[:-1, :-1] + E[:-1, 1:] + E[1:, :-1] + E[1:, 1:]               # N[y, x]: the 2 x 2 blocks whose top-left is (y, x)
    inv = 1.0 / np.sqrt(N + 0.0001)
    n1, n2, n3, n4 = inv[1:, 1:], inv[:-1, 1:], inv[1:, :-1], inv[:-1, :-1]
    if swap_n2_n3:
        n2, n3 = n3, n2
    c, tc = hist[1:-1, 1:-1], t[1:-1, 1:-1]
    tex = []
    for n in (n1, n2, n3, n4):
        hk = np.minimum(c * n[..., None], 0.2)
        feat[..., :18] += hk
        feat[..., 18:27] += np.minimum(tc * n[..., None], 0.2)
        tex.append(hk.sum(axis=-1))
    feat[..., :27] *= 0.5
    feat[..., 27:31] = 0.2357 * np.stack(tex, axis=-1)
    if details:
        return feat, margin, dict(absdot=np.abs(gx) + np.abs(gy), iy=iyp, ix=ixp, bw=bw, bh=bh)
    return feat, margin


def float_bound(sbin):
    """Worst-case |feature_float - feature_exact| for T = float, given the SAME orientation bin per pixel, derived from the float
    evaluation alone (u = 2^-24, first order; nothing here comes from measured kernel output).  Returns (bound for features 0..26,
    bound for the texture features 27..30).

      * sbin is a power of two, so (x + .5)/sbin - .5, the four bilinear weights and their products are exact floats.
      * pixel: dx, dy exact (8/16-bit), the same rounded float in both (CV_32F) or narrowed once (CV_64F: u, so u on the magnitude);
        dx^2 + dy^2: 2u, sqrt halves it and rounds: 2u; times the weight: 4u per vote.  All votes are >= 0, so errors stay RELATIVE
        to the sum.
      * a bin of a cell receives at most n = (2 sbin)^2 = 4 sbin^2 votes, added one by one: (n - 1)u.  hist: eh = (n + 4)u.
      * energy: (a + b)^2 summed over 9: 2 eh + 12u; four of them added in T: + 3u; + eps, sqrt in double (halves), 1/x, narrowing:
        n_k: en <= eh + 10u.
      * c[o] * n_k: eh + en + u; min with (float)0.2 (|0.2f - 0.2| < 0.2u): value <= 0.2, error 0.2 (eh + en + 2u).
      * features 0..17: three float adds (3u) and the narrowing of 0.5 * sum (u), value <= 0.4:  0.4 (2 eh + 16u); 18..26 add one u for
        c[o] + c[o + 9]:  0.4 (2 eh + 17u) = 0.4 (2n + 25) u — used for all of 0..26.
      * texture: 18 float adds (18u) of values <= 0.2, times 0.2357 in double and narrowed (u), value <= 0.2357 * 3.6:
        0.8486 (2 eh + 31u) = 0.8486 (2n + 39) u.
    sbin 4: 3.6e-6 and 8.4e-6; sbin 8: 1.3e-5 and 2.8e-5.  (No factor is gained from the bilinear weights summing to sbin^2 per cell: the error of a running sum is u times the sum of its
    PARTIAL sums, which the number of additions bounds, not the size of the terms; every pixel's weight is non-zero, so n adds stand.)
    This is the rigorous worst case (every one of the n votes in one bin, every
    rounding in one direction); the measured figures are ~100 times smaller (test docstrings).  It is still far below the smallest
    mistake it exists for: the power checks of tests/test_pyramid_definition_cpu.py fail against it."""
    s = int(sbin)
    assert s & (s - 1) == 0, "the derivation assumes a power-of-two bin size (exact bilinear weights)"
    n = 4 * s * s
    return 0.4 * (2 * n + 25) * U32, 0.8486 * (2 * n + 39) * U32


def float_dot_error(absdot):
    """bound of |dot_float - dot_exact| for dot = uu dx + vv dy in float: the two coefficients narrowed (u each), two products (u each),
    one add (u), and for CV_64F images dx, dy narrowed (u): <= 4u (|uu dx| + |vv dy|) <= 4u (|dx| + |dy|).  Two dots are compared, so a float evaluation can only pick another
    orientation than the exact one where the exact margin is <= 2 * this."""
    return 4.0 * U32 * np.asarray(absdot, np.float64)


def excused_cells(margin, det, out_shape):
    """T = float on 16-bit / float / double images: output cells that may legitimately differ, i.e. those touched by a pixel whose exact
    orientation margin is within the float error of the comparison (float_dot_error, twice).  A pixel votes into hist cells
    (iy..iy+1, ix..ix+1); hist cell (cy, cx) enters output cells (cy-2..cy, cx-2..cx) (its own features and the 2 x 2 energies around)."""
    oh, ow = out_shape
    bad = (margin > 0) & (margin <= 2.0 * float_dot_error(det["absdot"]))
    mask = np.zeros((oh, ow), bool)
    for py, px in zip(*np.nonzero(bad)):
        cy, cx = det["iy"][py], det["ix"][px]
        mask[max(cy - 2, 0):min(cy + 2, oh), max(cx - 2, 0):min(cx + 2, ow)] = True   # rows cy-2 .. cy+1 (hist rows cy, cy+1)
    return mask, int(bad.sum())
