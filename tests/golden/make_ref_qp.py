"""Writes tests/golden/ref_qp_v1.npz: the outputs of the COMPILED reference sweeps of the QP's example cache — matlab/mex/score.cc and
matlab/mex/lincomb.cc, read in place from the reference checkout — on the cases of tests/qp_cases.py.

Only outputs are stored (float64); the inputs are regenerated from seeds by the tests.  The two reference files are compiled, each
with tests/golden/ref_qp_driver.cpp (the accessor bodies of tests/golden/ref_qp_shim/mex.h and one extern "C" call, no arithmetic),
into a temporary directory outside the tree: nothing compiled is kept.  -ffp-contract=off: no product is fused into a sum.

    PBD_REFERENCE=<reference checkout> python tests/golden/make_ref_qp.py
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

from tests import qp_cases  # noqa: E402


def build(ref, tmp, which):
    so = os.path.join(tmp, f"libref_{which}.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w", f"-DREF_{which.upper()}",
                           "-I", os.path.join(HERE, "ref_qp_shim"), os.path.join(HERE, "ref_qp_driver.cpp"),
                           os.path.join(ref, "matlab", "mex", f"{which}.cc"), "-o", so])
    fn = C.CDLL(so).ref_qp
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return fn


def call(fn, x, v, vlen, inds, nout):
    x = np.ascontiguousarray(x, np.float32)                 # [ncols, k] row-major = k x ncols column-major
    v = np.ascontiguousarray(v, np.float64)
    i1 = np.ascontiguousarray(np.asarray(inds, np.float64) + 1.0)   # MATLAB's 1-based indices, as doubles
    out = np.zeros(max(nout, 1), np.float64)
    assert fn(x.ctypes.data, x.shape[1], x.shape[0], v.ctypes.data, vlen, i1.ctypes.data, len(i1), out.ctypes.data) == 0
    return out[:nout]


if __name__ == "__main__":
    ref = os.environ.get("PBD_REFERENCE")
    if not ref or not os.path.isfile(os.path.join(ref, "matlab", "mex", "score.cc")):
        sys.exit("set PBD_REFERENCE to the reference checkout (matlab/mex/score.cc, matlab/mex/lincomb.cc)")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        score, lincomb = build(ref, tmp, "score"), build(ref, tmp, "lincomb")
        for name, make in qp_cases.CASES.items():
            c = make()
            for iname, inds in c["inds"].items():
                out[f"{name}_score_{iname}"] = call(score, c["x"], c["w"], qp_cases.LEN, inds, len(inds))
                out[f"{name}_lincomb_{iname}"] = call(lincomb, c["x"], c["a"], qp_cases.LEN, inds, qp_cases.LEN)
    path = os.path.join(HERE, "ref_qp_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")
