"""Writes tests/golden/ref_hog_v1.npz: the outputs of the COMPILED reference HOG (the reference's matlab/mex/features.cc, built by
`make -C oracle ref_features` into oracle/_ref/libref_features.so) on the frames of tests/pyramid_cases.fixture_frames().

Only outputs are stored (float64); the inputs are regenerated from seeds by the tests.  Nothing of this repository's arithmetic is
between the image and the stored numbers: oracle/ref_features hands the image over as planar doubles and reads the result back.

    python tests/golden/make_ref_hog.py        (needs the reference checkout, see oracle/ref_features/README.md)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_features  # noqa: E402
from tests.pyramid_cases import fixture_frames  # noqa: E402

if __name__ == "__main__":
    if not ref_features.available():
        sys.exit("oracle/_ref/libref_features.so is missing: run `make -C oracle ref_features` with PBD_REFERENCE set")
    out = {name: ref_features.features(im, sbin) for name, im, sbin in fixture_frames()}
    path = os.path.join(HERE, "ref_hog_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})
