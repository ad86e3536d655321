"""What one coordinate-descent pass on the device (pbd_qp_pass, k_qp_pass: one workgroup) costs, beside what a host solver pays today
just to see the columns (pbd_qp_get of the same cache).

The person model (26 parts x 6 mixtures): one detect at a threshold that leaves --records roots, the frame's records written into a
cache of --examples examples (repeated until full; labels alternate; every example keeps its own id, so the per-id pair branch does
not run: the timed step is score + decisions + axpy + clamp), then
  pass   pbd_qp_pass over all examples in a shuffled order, host clock around the synchronous call: --reps passes in a row (the
         state moves on, as in qp_opt), median [quartiles] in ms and microseconds per step;
  one    pbd_qp_one (pass + refresh + bounds) likewise;
  get    pbd_qp_get of the whole cache, host clock.
One JSON line.
    python tests/tools_qp_solve_probe.py [--size 320x240] [--reps 10] [--examples 1024] [--records 2000]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from partsbaseddetector_amd import capi  # noqa: E402
from partsbaseddetector_amd.model import make_image, make_person_model  # noqa: E402

CAP = 65536


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="320x240")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--examples", type=int, default=1024)
    ap.add_argument("--records", type=int, default=2000)
    a = ap.parse_args()
    w, hgt = (int(v) for v in a.size.split("x"))
    im = make_image(0, w, hgt)
    model = make_person_model()
    model.thresh = 3.0e38
    h = capi.Handle(model)
    h.detect(im)
    g = h.geometry(w, hgt)
    h._geo = g
    vals = np.sort(np.concatenate([h.root(l, 0)[0].ravel() for l in range(g["nlevels"])]))[::-1]
    h.close()
    model.thresh = float(vals[min(a.records, len(vals) - 1)])
    h = capi.Handle(model, max_candidates=CAP)
    heads, _, locs = h.detect(im, CAP)
    N = a.examples
    q = capi.QpCache(h, N, 0.002, 0.002)
    length, k, _, _ = q.dims()
    at, group = 0, 0
    while q.dims()[3] < N:                           # labels alternate by groups of four
        sel = np.arange(at, at + 4) % len(heads)
        q.write(heads[sel], locs[sel], 1 if group % 2 else -1, group)
        at, group = at + 4, group + 1
    q.noneg(model.qp_vectors()[3])
    x = q.get(0, 1)[0]
    out = dict(size=a.size, records=len(heads), cache=dict(examples=N, k=k, len=length, blocks=int(x[0, 0]), column_bytes=4 * k * N))
    rng = np.random.default_rng(0)

    def timed(fn):
        ms = []
        for r in range(a.warmup + a.reps):
            order = rng.permutation(N).astype(np.int32)
            t0 = time.perf_counter()
            fn(order)
            if r >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms
    ms = timed(q.solve_pass)
    out["pass_ms"] = stats(ms)
    out["pass_us_per_step"] = round(statistics.median(ms) * 1e3 / N, 2)
    out["one_ms"] = stats(timed(q.one))
    a_, sv, _, st = q.state()
    out["after"] = dict(support_vectors=int(sv.sum()), nonzero_a=int((a_ > 0).sum()), lb=st[1], ub=st[3])
    ms = []
    for r in range(max(a.reps // 3, 3)):
        t0 = time.perf_counter()
        q.get()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["get_ms"] = stats(ms)
    q.close()
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
