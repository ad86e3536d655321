"""What the best pose per ground-truth box on the device (pbd_detect_gtbox_u8) costs beside the call shape it replaces.

The person model (26 parts x 6 mixtures) at 640x480, one gt box (the top record's centre box grown by 10 pixels), overlap 0.3, at two
thresholds: bench.py's (99.9th percentile of the seed frame's root scores) and one low enough for at least 20 000 records.  Per frame,
host clock around synchronous calls, the three variants alternating in one loop after a warm-up of each:
  gtbox       pbd_detect_gtbox_u8: the selection behind the back-tracking, one record comes home;
  plain       pbd_detect_u8 (eager launches, as gt-box frames run) then the host pbd_candidates_best_overlap on everything it returned;
  plain_graph the same on a handle that replays its captured graph (pbd_options.graph = 1).
One JSON line per threshold: records per frame, median / quartiles / minimum in ms of each variant, and whether the winners agree.
    python tests/tools_gtbox_probe.py [--size 640x480] [--reps 60] [--records 20000]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from partsbaseddetector_amd import capi  # noqa: E402
from partsbaseddetector_amd.model import make_image, make_person_model  # noqa: E402

OVERLAP = 0.3
CAP = 65536


def root_scores(model, w, hgt):
    model.thresh = 3.0e38
    h = capi.Handle(model)
    h.detect(make_image(0, w, hgt))
    h._geo = h.geometry(w, hgt)
    vals = np.concatenate([h.root(l, c)[0].ravel() for l in range(h._geo["nlevels"]) for c in range(model.ncomponents)])
    first = np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])])
    h.close()
    return vals, first


class Plain:
    """pbd_detect_u8 into arrays allocated once, then the host selection"""
    def __init__(self, model, graph):
        self.h = capi.Handle(model, graph=graph, max_candidates=CAP)
        self.heads, self.boxes, self.locs = self.h._bufs(CAP)
        self.cnt = C.c_int(0)

    def run(self, im, gt):
        h = self.h
        hgt, w = im.shape[:2]
        h._chk(h.L.pbd_detect_u8(h.h, capi._p(im, C.c_uint8), w, hgt, 3, w * 3, self.heads.ctypes.data_as(C.c_void_p),
                                 capi._p(self.boxes, C.c_int32), capi._p(self.locs, C.c_int32), CAP, C.byref(self.cnt)))
        n = self.cnt.value
        best, o = capi.candidates_best_overlap(self.heads[:n], self.boxes[:n], gt, OVERLAP)
        return n, (self.heads[best[0]].copy() if best[0] >= 0 else None), o[0]


class GtBox:
    def __init__(self, model):
        self.h = capi.Handle(model, max_candidates=CAP)

    def run(self, im, gt):
        heads, boxes, locs, found, o = self.h.detect_gtbox(im, gt, OVERLAP)
        return self.h.gt_records, (heads[0].copy() if found[0] else None), o[0]


def stats(t):
    q = statistics.quantiles(t, n=4)
    return {"median": round(statistics.median(t) * 1e3, 3), "q1": round(q[0] * 1e3, 3), "q3": round(q[2] * 1e3, 3),
            "min": round(min(t) * 1e3, 3)}


def measure(model, im, reps, label):
    probe = capi.Handle(model, max_candidates=CAP)
    raw = probe.detect(im, CAP)
    probe.close()
    top = int(np.argmax(raw[0]["score"]))
    b = raw[1][top][:int(raw[0]["nparts"][top])].astype(np.float64)
    cx, cy = b[:, 0] + .5 * (b[:, 2] - 1), b[:, 1] + .5 * (b[:, 3] - 1)
    gt = np.array([[cx.min() - 10, cy.min() - 10, cx.max() + 10, cy.max() + 10]])
    variants = {"gtbox": GtBox(model), "plain": Plain(model, 0), "plain_graph": Plain(model, 1)}
    res = {}
    for _ in range(8):                                  # warm-up: plans, the graph's capture, the first-copy sizing
        for k, v in variants.items():
            res[k] = v.run(im, gt)
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, v in variants.items():
            t0 = time.perf_counter()
            v.run(im, gt)
            times[k].append(time.perf_counter() - t0)
    for v in variants.values():
        v.h.close()
    same = all(r[1] is not None and r[1].tobytes() == res["gtbox"][1].tobytes() and r[2] == res["gtbox"][2] for r in res.values())
    print(json.dumps({"threshold": label, "records": res["gtbox"][0], "reps": reps, "winners_agree": bool(same),
                      "ms": {k: stats(t) for k, t in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--records", type=int, default=20000)
    a = ap.parse_args()
    w, hgt = map(int, a.size.split("x"))
    model = make_person_model()
    vals, first = root_scores(model, w, hgt)
    im = make_image(0, w, hgt)
    model.thresh = float(np.float32(np.percentile(first, 99.9)))
    measure(model, im, a.reps, "bench")
    srt = np.sort(vals)[::-1]
    model.thresh = float(np.float32(srt[min(len(srt) - 1, int(a.records * 1.05))]))   # a little below the records-th best root score
    measure(model, im, a.reps, f">={a.records} records")


if __name__ == "__main__":
    main()
