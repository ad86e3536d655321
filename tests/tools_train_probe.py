"""What the seams of one training round cost ("One training round").

1. Mining one 640x480 negative at interval 2 against the model's own interval, on the same handle (pbd_set_interval between the two): the
   person model (26 parts x 6 mixtures), thresh = -1 raised, if need be, to the score of the --records-th best root of the interval-10
   pyramid; one cache, cleared before every call (pbd_qp_clear).  The first call after a change of interval plans the frame again and is
   timed on its own (`replan_ms`); then --reps timed calls of each interval in turn.
2. pbd_qp_positive_threshold at m = --m positives against the host route it replaces: pbd_qp_get of the ids, w + w0 .* wreg on the
   host, pbd_qp_score of the positives, / cpos, the sort.  The columns are mined records relabelled +1 through pbd_qp_get / pbd_qp_put.
Host clock around each synchronous call, warm-up calls first; one JSON line: median [first quartile, third quartile] in ms.
    python tests/tools_train_probe.py [--size 640x480] [--reps 20] [--records 20000] [--m 2000]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from partsbaseddetector_amd import capi  # noqa: E402
from partsbaseddetector_amd.model import Model, make_image, make_person_model  # noqa: E402

CAP = 65536


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--records", type=int, default=20000)
    ap.add_argument("--m", type=int, default=2000)
    a = ap.parse_args()
    w, hgt = (int(v) for v in a.size.split("x"))
    im = make_image(0, w, hgt)
    model = make_person_model()
    model.thresh = 3.0e38
    h = capi.Handle(model, max_candidates=CAP)
    h.detect(im)
    h._geo = h.geometry(w, hgt)
    vals = np.sort(np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])]))[::-1]
    h.set_threshold(max(-1.0, float(vals[min(a.records, len(vals) - 1)])))
    out = dict(size=a.size, thresh=h.threshold, reps=a.reps)
    # ---- 1. mining at interval 2 against the model's interval ----
    q = capi.QpCache(h, CAP, 0.004, 0.002)
    for iv in (model.interval, 2):
        h.set_interval(iv)
        q.clear()
        t0 = time.perf_counter()
        rec = q.mine(im, 0)[0]
        replan = (time.perf_counter() - t0) * 1e3
        ms = []
        for r in range(a.warmup + a.reps):
            q.clear()
            t0 = time.perf_counter()
            got = q.mine(im, 0)[0]
            t1 = time.perf_counter()
            assert got == rec
            if r >= a.warmup:
                ms.append((t1 - t0) * 1e3)
        out[f"mine_interval_{iv}"] = dict(levels=h.geometry(w, hgt)["nlevels"], records=rec, mine_ms=stats(ms), replan_ms=round(replan, 4))
    # ---- 2. the positives' threshold at m positives ----
    h.set_interval(model.interval)
    q.clear()
    q.mine(im, 0)
    n = min(q.dims()[3], 2 * a.m)
    x, ids, b, d = q.get(0, n)
    q.close()
    ids[::2, 0] = 1                                        # every other example a positive
    length = model.feature_layout()["size"]
    rng = np.random.default_rng(0)
    wreg, w0 = 0.5 + rng.random(length), 0.01 * rng.standard_normal(length)
    p = capi.QpCache(h, n, 0.004, 0.002, wreg, w0)
    p.put(x, ids, b, d)
    p.set_state(a=rng.random(n) * 1e-3, sv=np.ones(n, np.uint8))
    p.refresh()
    dev, host, same = [], [], True
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        thr, m = p.positive_threshold(.05)
        t1 = time.perf_counter()
        I2 = np.flatnonzero(p_ids(p, n)[:, 0] == 1).astype(np.int32)    # pbd_qp_get of the ids alone
        wv = p.state()[2]
        want = Model.positive_threshold(p.score(wv + w0 * wreg, I2) / 0.004, .05)
        t3 = time.perf_counter()
        same = same and np.float64(thr).tobytes() == np.float64(want).tobytes() and m == len(I2)
        if r >= a.warmup:
            dev.append((t1 - t0) * 1e3); host.append((t3 - t1) * 1e3)
    out["positive_threshold"] = dict(m=int(m), n=int(n), k=p.dims()[1], device_ms=stats(dev), host_route_ms=stats(host), same_bits=bool(same),
                                     pcie_bytes_device=16, pcie_bytes_host_route=int(20 * n + 8 * length * 2 + 12 * m))
    p.close()
    h.close()
    print(json.dumps(out))


def p_ids(p, n):
    ids = np.zeros((n, 5), np.int32)
    p.handle._chk(p.L.pbd_qp_get(p.q, 0, n, None, ids.ctypes.data, None, None))
    return ids


if __name__ == "__main__":
    main()
