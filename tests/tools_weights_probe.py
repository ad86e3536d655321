"""What a weight update costs: pbd_set_weights plus the first detect after it, beside the only route there was before —
pbd_destroy + pbd_create + the first detect of the new handle —, and pbd_qp_apply_weights alone.  Person model, one make_image frame,
float handle; host clock with a device synchronisation on both sides of every figure; --reps runs each, the median (and the runs).
One JSON line.
    python tests/tools_weights_probe.py [--size 640x480] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from partsbaseddetector_amd import capi  # noqa: E402
from partsbaseddetector_amd.model import make_image, make_person_model  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def root_percentile(model, im, q=99.9):
    model.thresh = 3.0e38
    h = capi.Handle(model)
    h.detect(im)
    h._geo = h.geometry(im.shape[1], im.shape[0])
    vals = np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])])
    h.close()
    return float(np.float32(np.percentile(vals, q)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    w, hgt = (int(v) for v in a.size.split("x"))
    im = make_image(0, w, hgt)
    ma = make_person_model(seed=1234)
    wv = [ma.weight_vector(), make_person_model(seed=99).weight_vector()]
    models = [ma, ma.with_weight_vector(wv[1])]
    t = max(root_percentile(m, im) for m in models)   # bench.py's workload: about 140 candidates per frame
    for m in models:
        m.thresh = t
    runs = dict(set_weights_detect=[], set_weights=[], destroy_create_detect=[], apply_weights=[], steady_detect=[])
    h = capi.Handle(models[0])
    for _ in range(3):
        h.detect(im)
    q = capi.QpCache(h, 16)
    q.apply_weights()                      # (the solver state exists from here on)
    h.set_weights(wv[0])
    h.detect(im)
    for r in range(a.reps):
        v = wv[(r + 1) % 2]
        runs["set_weights"].append(timed(lambda: h.L.pbd_set_weights(h.h, v.ctypes.data, v.size)))
        h.detect(im)
        v = wv[r % 2]
        runs["set_weights_detect"].append(timed(lambda: (h.L.pbd_set_weights(h.h, v.ctypes.data, v.size), h.detect(im))))
        h.detect(im)
        runs["steady_detect"].append(timed(lambda: h.detect(im)))
        runs["apply_weights"].append(timed(lambda: h.L.pbd_qp_apply_weights(q.q)))
        h.set_weights(wv[0])
        h.detect(im)
    q.close()
    for r in range(a.reps):
        def fresh():
            nonlocal h
            h.close()
            h = capi.Handle(models[(r + 1) % 2])
            h.detect(im)
        runs["destroy_create_detect"].append(timed(fresh))
        h.detect(im)
    h.close()
    out = dict(size=a.size, len=int(wv[0].size), reps=a.reps, thresh=t)
    for k, v in runs.items():
        out[k + "_ms"] = dict(median=round(statistics.median(v), 3), runs=[round(x, 3) for x in v])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
