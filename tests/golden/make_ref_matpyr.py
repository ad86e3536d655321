"""Writes tests/golden/ref_matpyr_v1.npz: the outputs of the COMPILED reference pyramid stages — matlab/mex/resize.cc and
matlab/mex/reduce.cc, read in place from the reference checkout — on the cases of tests/matlab_pyramid_ref.py.

Only outputs are stored (float64); the inputs are regenerated from seeds by the tests.  The two reference files are compiled, each
with tests/golden/ref_matpyr_driver.cpp (the accessor bodies of oracle/ref_features/mex.h and one extern "C" call, no arithmetic),
into a temporary directory outside the tree: nothing compiled is kept.  -ffp-contract=off: no product is fused into a sum.

    PBD_REFERENCE=<reference checkout> python tests/golden/make_ref_matpyr.py
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import matlab_pyramid_ref as mp  # noqa: E402
from tests.pyramid_cases import noise  # noqa: E402


def build(ref, tmp, which):
    so = os.path.join(tmp, f"libref_{which}.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w", f"-DREF_{which.upper()}",
                           "-I", os.path.join(ROOT, "oracle", "ref_features"), os.path.join(HERE, "ref_matpyr_driver.cpp"),
                           os.path.join(ref, "matlab", "mex", f"{which}.cc"), "-o", so])
    fn = C.CDLL(so).ref_matpyr
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return fn


def call(fn, im, scale, oh, ow):
    """im [h, w, cn] -> [oh, ow, cn]: to the reference's planar column-major layout and back (copies only)"""
    im = np.asarray(im, np.float64)
    if im.ndim == 2:
        im = im[:, :, None]
    h, w, cn = im.shape
    src = np.ascontiguousarray(im.transpose(2, 1, 0))
    out = np.zeros((cn, ow, oh), np.float64)
    r, c = C.c_int(0), C.c_int(0)
    assert fn(src.ctypes.data, h, w, cn, scale, None, C.byref(r), C.byref(c)) == 0 and (r.value, c.value) == (oh, ow), (r.value, c.value, oh, ow)
    assert fn(src.ctypes.data, h, w, cn, scale, out.ctypes.data, C.byref(r), C.byref(c)) == 0
    return np.ascontiguousarray(out.transpose(2, 1, 0))


if __name__ == "__main__":
    ref = os.environ.get("PBD_REFERENCE")
    if not ref or not os.path.isfile(os.path.join(ref, "matlab", "mex", "resize.cc")):
        sys.exit("set PBD_REFERENCE to the reference checkout (matlab/mex/resize.cc, matlab/mex/reduce.cc)")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        resize, reduce_ = build(ref, tmp, "resize"), build(ref, tmp, "reduce")
        for name, im, s in mp.resize_cases():
            h, w = im.shape[:2]
            out[name] = call(resize, im, s, mp.c_round(h * s), mp.c_round(w * s))
        for name, im in mp.reduce_cases():
            h, w = im.shape[:2]
            out[name] = call(reduce_, im, 0.0, mp.c_round(h * .5), mp.c_round(w * .5))
        im = noise(*mp.PYRAMID_FRAME)
        for interval in mp.PYRAMID_INTERVALS:
            g = mp.geometry_matlab(im.shape[1], im.shape[0], mp.PYRAMID_SBIN, interval)
            sc = 2.0 ** (1.0 / interval)
            lv = [None] * g["nlevels"]
            for i in range(interval):
                lv[i] = call(resize, im, 1.0 / sc ** i, int(g["img_h"][i]), int(g["img_w"][i]))
                for j in range(i + interval, g["nlevels"], interval):
                    lv[j] = call(reduce_, lv[j - interval], 0.0, int(g["img_h"][j]), int(g["img_w"][j]))
            for l, a in enumerate(lv):
                out[f"pyr_i{interval}_l{l}"] = a
    path = os.path.join(HERE, "ref_matpyr_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")
