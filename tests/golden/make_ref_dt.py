"""Writes tests/golden/ref_dt_v1.npz: the outputs of the COMPILED reference distance transform (the reference's
include/DistanceTransform.hpp, built by `make -C oracle ref_dt` into oracle/_ref/libref_dt.so) on tests/dt_path_cases.RECORDED_CASES.

Only outputs are stored — scores in the case's own type, pointers as int16 —; the inputs are regenerated from seeds by the tests.
Nothing of this repository's arithmetic is between the map and the stored numbers: oracle/ref_dt hands the map over and reads the
result back.

    python tests/golden/make_ref_dt.py        (needs the reference checkout, see oracle/ref_dt/README.md)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_dt  # noqa: E402
from tests import dt_path_cases as dc  # noqa: E402

if __name__ == "__main__":
    if not ref_dt.available():
        sys.exit("oracle/_ref/libref_dt.so is missing: run `make -C oracle ref_dt` with PBD_REFERENCE set")
    out = {}
    for c in dc.RECORDED_CASES:
        o, ix, iy = ref_dt.dt2d(c["make"](), *c["q"], dtype=c["dtype"])
        assert o.dtype == c["dtype"] and 0 <= ix.min() and ix.max() < 32768 and 0 <= iy.min() and iy.max() < 32768
        out[c["name"] + "_out"], out[c["name"] + "_ix"], out[c["name"] + "_iy"] = o, ix.astype(np.int16), iy.astype(np.int16)
    np.savez_compressed(dc.REF_DT_FIXTURE, **out)
    print(dc.REF_DT_FIXTURE, os.path.getsize(dc.REF_DT_FIXTURE), "bytes;", len(dc.RECORDED_CASES), "cases")
