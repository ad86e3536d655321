"""ctypes binding of oracle/_ref/libref_dt.so: the reference's include/DistanceTransform.hpp (DistanceTransform<T>::compute with
Quadratic penalties), compiled in place from its checkout by `make -C oracle ref_dt` (see README.md here).
TEST INFRASTRUCTURE, like the rest of oracle/."""
import ctypes as C
import os

import numpy as np

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "_ref", "libref_dt.so")
_lib = None


def available() -> bool:
    return os.path.exists(LIB)


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(LIB)
        for fn in (_lib.ref_dt2d, _lib.ref_dt2d_f64):
            fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                           C.c_void_p, C.c_void_p, C.c_void_p]
            fn.restype = None
    return _lib


def dt2d(a, ax, bx, ay, by, osx, osy, dtype=np.float32):
    """[rows, cols] scores -> (out, ix, iy) of DistanceTransform<dtype>::compute(a, Quadratic(ax, bx), Quadratic(ay, by),
    Point(osx, osy)): the signature of oracle.orc.dt2d."""
    a = np.ascontiguousarray(a, dtype)
    assert a.ndim == 2 and a.dtype in (np.float32, np.float64)
    out = np.zeros_like(a)
    ix, iy = np.zeros(a.shape, np.int32), np.zeros(a.shape, np.int32)
    fn = _load().ref_dt2d_f64 if a.dtype == np.float64 else _load().ref_dt2d
    fn(a.ctypes.data, a.shape[0], a.shape[1], float(ax), float(bx), float(ay), float(by), int(osx), int(osy),
       out.ctypes.data, ix.ctypes.data, iy.ctypes.data)
    return out, ix, iy
