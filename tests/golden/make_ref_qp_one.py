"""Writes tests/golden/ref_qp_one_v1.npz and ref_qp_one_v2.npz: the outputs of the COMPILED reference coordinate-descent pass —
matlab/mex/qp_one_sparse.cc, read in place from the reference checkout — over consecutive passes of the cases of
tests/qp_solve_cases.py: v1 holds CASES (free, binding), v2 holds LARGE_CASES (manyblock, manyids), every pass of both in full.

Only outputs are stored, per case and pass: loss, a, w, sv, l.  The inputs are regenerated from seeds by the tests; the order of pass p
is qp_solve_cases.next_order of the sv the compiled file left.  The file is compiled with tests/golden/ref_qp_one_driver.cpp (the
accessor bodies of tests/golden/ref_qp_one_shim/mex.h and one extern "C" call, no arithmetic) into a temporary directory outside the
tree: nothing compiled is kept.  -ffp-contract=off: no product is fused into a sum.

    PBD_REFERENCE=<reference checkout> python tests/golden/make_ref_qp_one.py [v1 | v2]      (neither: both files)
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

from tests import qp_solve_cases  # noqa: E402
from tests.qp_cases import LEN  # noqa: E402


def build(ref, tmp):
    so = os.path.join(tmp, "libref_qp_one.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-I", os.path.join(HERE, "ref_qp_one_shim"),
                           os.path.join(HERE, "ref_qp_one_driver.cpp"), os.path.join(ref, "matlab", "mex", "qp_one_sparse.cc"), "-o", so])
    fn = C.CDLL(so).ref_qp_one
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double,
                                                                        C.c_void_p, C.c_int, C.c_void_p]
    return fn


def run_case(fn, c):
    x = np.ascontiguousarray(c["x"], np.float32)              # [n, k] row-major = k x n column-major
    ids, b, d = (np.ascontiguousarray(c[k_]) for k_ in ("ids", "b", "d"))
    a, w = c["a"].copy(), c["w"].copy()
    noneg1 = (c["noneg"] + 1).astype(np.uint32)               # MATLAB's 1-based indices
    sv = np.ones(len(x), np.bool_)
    l = np.array([c["l"]], np.float64)
    out = {}
    for p in range(c["passes"]):
        order = qp_solve_cases.next_order(c, p, sv)
        o1 = np.ascontiguousarray(order.astype(np.float64) + 1.0)
        loss = np.zeros(1)
        assert fn(x.ctypes.data, x.shape[1], x.shape[0], ids.ctypes.data, b.ctypes.data, d.ctypes.data, a.ctypes.data, w.ctypes.data,
                  LEN, noneg1.ctypes.data, len(noneg1), sv.ctypes.data, l.ctypes.data, 1.0, o1.ctypes.data, len(o1),
                  loss.ctypes.data) == 0
        out[p] = dict(loss=loss.copy(), a=a.copy(), w=w.copy(), sv=sv.astype(np.uint8), l=l.copy())
    return out


if __name__ == "__main__":
    ref = os.environ.get("PBD_REFERENCE")
    if not ref or not os.path.isfile(os.path.join(ref, "matlab", "mex", "qp_one_sparse.cc")):
        sys.exit("set PBD_REFERENCE to the reference checkout (matlab/mex/qp_one_sparse.cc)")
    files = {"v1": qp_solve_cases.CASES, "v2": qp_solve_cases.LARGE_CASES}
    with tempfile.TemporaryDirectory() as tmp:
        fn = build(ref, tmp)
        for version in sys.argv[1:] or sorted(files):
            out = {}
            for name, make in files[version].items():
                for p, r in run_case(fn, make()).items():
                    for key, v in r.items():
                        out[f"{name}_{p}_{key}"] = v
            path = os.path.join(HERE, f"ref_qp_one_{version}.npz")
            np.savez_compressed(path, **out)
            print(path, os.path.getsize(path), "bytes;", len(out), "arrays")
