"""Cost of a mixed filter bank (pbd_create_sized) against its size groups run as uniform banks of their own.

The person model (26 parts x 6 mixtures) with its 6 root filters 7 x 7 and the other 150 filters 5 x 5, at 640 x 480: the pdf stage
(pbd_get_stage_ms) of the mixed handle, of one uniform handle per size group (same frame geometry), and of the bank padded to the
largest size (every filter 7 x 7 with zero taps: what the mixed bank avoids).  Median of `--reps` frames after warm-up; one JSON line.
    python tests/tools_mixed_bank_probe.py [--reps 30] [--mode split|exact|mfma]   (split: what AUTO runs for the mixed bank)"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from partsbaseddetector_amd import capi  # noqa: E402
from partsbaseddetector_amd.model import make_image, make_mixed_person_model  # noqa: E402


def pdf_ms(model, im, mode, reps):
    h = capi.Handle(model, conv_mode=mode)
    h.set_profiling(True)
    for _ in range(5):
        h.detect(im)
    v = []
    for _ in range(reps):
        h.detect(im)
        v.append(h.stage_ms()["pdf"])
    h.close()
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--mode", default="split", choices=["split", "exact", "mfma"])
    a = ap.parse_args()
    mode = dict(split=capi.PBD_CONV_SPLIT, exact=capi.PBD_CONV_EXACT, mfma=capi.PBD_CONV_MFMA)[a.mode]
    m = make_mixed_person_model(seed=1234, K=6, root=(7, 7), odd_sizes=())
    m.thresh = 1e30   # the bank's cost only: no candidates
    im = make_image(0, 640, 480, 3)
    out = dict(mode=a.mode, nfilters=len(m.filtersw), mixed_ms=pdf_ms(m, im, mode, a.reps), groups={})
    sizes = m.filter_sizes()
    for kh, kw in sorted({tuple(s) for s in sizes.tolist()}):
        idx = [n for n in range(len(m.filtersw)) if tuple(sizes[n]) == (kh, kw)]
        g = type(m)(**{**m.__dict__, "filtersw": [m.filtersw[i] for i in idx],
                       "filterid": [[[0] * len(k) for k in comp] for comp in m.filterid], "_keep": []})
        # a uniform handle of the group's filters on the same frame geometry (its DP is the model's shape with filter 0 everywhere)
        out["groups"][f"{kh}x{kw}"] = dict(n=len(idx), pdf_ms=pdf_ms(g, im, mode, a.reps))
    pad = type(m)(**{**m.__dict__, "_keep": [], "filtersw": [np.pad(f.reshape(f.shape[0], -1, m.flen),
                     ((0, 7 - f.shape[0]), (0, 7 - f.shape[1] // m.flen), (0, 0))).reshape(7, 7 * m.flen) for f in m.filtersw]})
    out["padded_7x7_ms"] = pdf_ms(pad, im, mode, a.reps)
    out["sum_groups_ms"] = sum(g["pdf_ms"] for g in out["groups"].values())
    out["mixed_over_sum"] = out["mixed_ms"] / out["sum_groups_ms"]
    out["mixed_over_padded"] = out["mixed_ms"] / out["padded_7x7_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
