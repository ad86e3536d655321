"""Test helper: nonMaximaSuppression(src, sz, dst) of src/nms.cpp:84-129 restated line by line in numpy, without a mask.

Blocks of (sz+1) x (sz+1) from the origin; the block's maximum by minMaxLoc (the first maximum in row-major order); the
neighbourhood of (2 sz + 1)^2 around it clipped to the map, minus the window of (sz+1)^2 starting at the block's origin; a
point is kept when the block maximum is strictly greater than the neighbourhood's maximum, which is 0 when the
neighbourhood is empty (minMaxLoc over an all-zero mask leaves maxVal = 0).  Values compare as doubles (minMaxLoc's output)."""
import numpy as np


def nms_map(src, sz):
    src = np.asarray(src)
    M, N = src.shape
    dst = np.zeros((M, N), np.uint8)
    block = np.full((2 * sz + 1, 2 * sz + 1), 255, np.uint8)
    for m in range(0, M, sz + 1):
        for n in range(0, N, sz + 1):
            ic = (m, min(m + sz + 1, M))
            jc = (n, min(n + sz + 1, N))
            blk = src[ic[0]:ic[1], jc[0]:jc[1]].astype(np.float64)
            i, j = np.unravel_index(int(np.argmax(blk)), blk.shape)
            vcmax = float(blk[i, j])
            cy, cx = ic[0] + int(i), jc[0] + int(j)
            in_ = (max(cy - sz, 0), min(cy + sz + 1, M))
            jn = (max(cx - sz, 0), min(cx + sz + 1, N))
            blockmask = block[: in_[1] - in_[0], : jn[1] - jn[0]].copy()
            iis = (ic[0] - in_[0], min(ic[0] - in_[0] + sz + 1, in_[1] - in_[0]))
            jis = (jc[0] - jn[0], min(jc[0] - jn[0] + sz + 1, jn[1] - jn[0]))
            blockmask[iis[0]:iis[1], jis[0]:jis[1]] = 0
            nb = src[in_[0]:in_[1], jn[0]:jn[1]].astype(np.float64)[blockmask != 0]
            vnmax = float(nb.max()) if nb.size else 0.0
            if vcmax > vnmax:
                dst[cy, cx] = 255
    return dst
