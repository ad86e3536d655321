"""ctypes binding of oracle/_ref/libref_features.so: the reference's matlab/mex/features.cc, compiled in place from its
checkout by `make -C oracle ref_features` (see README.md here).  TEST INFRASTRUCTURE, like the rest of oracle/."""
import ctypes as C
import os

import numpy as np

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "_ref", "libref_features.so")
_lib = None


def available() -> bool:
    return os.path.exists(LIB)


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(LIB)
        _lib.ref_features.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def features(im, sbin):
    """im: H x W (grey) or H x W x 3 (interleaved, the C++ reference's channel order) of any dtype -> [cells_h, cells_w, 32] float64.

    features.cc wants a planar column-major double colour image.  Its tie rule is "the first plane wins, a later one must be
    strictly greater"; the C++ port starts from interleaved channel 2 and lets channel 1, then channel 0 replace it only when
    strictly greater, so the planes are handed over in the order (2, 1, 0).  A grey image is replicated into three planes:
    equal gradients, the strict `>` keeps the first, which is the path of the C++'s grey branch."""
    im = np.asarray(im)
    if im.ndim == 2:
        im = np.repeat(im[:, :, None], 3, axis=2)
    h, w = im.shape[:2]
    planar = np.ascontiguousarray(im[:, :, ::-1].astype(np.float64).transpose(2, 1, 0))   # [c][x][y] in C order == MATLAB (y, x, c)
    L = _load()
    a, b = C.c_int(0), C.c_int(0)
    if L.ref_features(planar.ctypes.data, h, w, int(sbin), None, C.byref(a), C.byref(b)):
        raise ValueError("features.cc refused the input")
    out = np.zeros((32, b.value, a.value), np.float64)
    rc = L.ref_features(planar.ctypes.data, h, w, int(sbin), out.ctypes.data, C.byref(a), C.byref(b))
    assert rc == 0
    return np.ascontiguousarray(out.transpose(2, 1, 0))
