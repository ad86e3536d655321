"""What hard-negative mining on the device (pbd_qp_mine_u8) costs beside the route it replaces.

The person model (26 parts x 6 mixtures) on one 640x480 frame, thresh = -1 raised, if need be, to the score of the --records-th best
root (a frame this size has more roots above -1 than max_candidates), once RAW and once with sort + nms.m's part-wise NMS
(overlap 0.3, the 1000 best).  Per mode, in one process, on one handle and one cache emptied before every call (keep of nothing):
  mine        QpCache.mine(im, 0);
  host route  Handle.detect(im) — every record collected into host arrays — then QpCache.write(all records, -1, 0).
Host clock around each synchronous call, warm-up calls first, then --reps timed calls of each route, alternating; one JSON line: median
[first quartile, third quartile] in ms, the records, and the bytes each route moves over PCIe beside the image (records x record size,
out and back in, against 28 bytes a frame), and whether the two routes left the same columns.
    python tests/tools_mine_probe.py [--size 640x480] [--reps 20] [--records 20000]"""
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
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--records", type=int, default=20000)
    a = ap.parse_args()
    w, hgt = (int(v) for v in a.size.split("x"))
    im = make_image(0, w, hgt)
    model = make_person_model()
    model.thresh = 3.0e38
    h = capi.Handle(model)
    h.detect(im)
    h._geo = h.geometry(w, hgt)
    vals = np.sort(np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])]))[::-1]
    h.close()
    model.thresh = max(-1.0, float(vals[min(a.records, len(vals) - 1)]))
    out = dict(size=a.size, thresh=model.thresh, reps=a.reps, record_bytes=16 + 28 * model.max_parts, image_bytes=w * hgt * 3)
    for name, kw in (("raw", {}), ("nms_parts", dict(cand_filter=(capi.PBD_CAND_SORT_NMS, 0.3), cand_nms=(capi.PBD_NMS_PARTS, 1000)))):
        h = capi.Handle(model, max_candidates=CAP, **kw)
        n = len(h.detect(im, CAP)[0])
        q = capi.QpCache(h, max(n, 1), 0.002, 0.002)
        mine, host, cols = [], [], []
        for r in range(a.warmup + a.reps):
            q.keep(np.zeros(0, np.int32))
            t0 = time.perf_counter()
            rec, wr, _ = q.mine(im, 0)
            t1 = time.perf_counter()
            if r == 0:
                cols.append([v.tobytes() for i0 in (0, max(n - 256, 0)) for v in q.get(i0, min(n, 256))])   # (the first and the last 256 columns)
            q.keep(np.zeros(0, np.int32))
            t2 = time.perf_counter()
            heads, _, locs = h.detect(im, CAP)
            wrote = q.write(heads, locs, -1, 0)
            t3 = time.perf_counter()
            if r == 0:
                cols.append([v.tobytes() for i0 in (0, max(n - 256, 0)) for v in q.get(i0, min(n, 256))])   # (the first and the last 256 columns)
            assert (rec, wr) == (n, n) == (len(heads), wrote)
            if r >= a.warmup:
                mine.append((t1 - t0) * 1e3); host.append((t3 - t2) * 1e3)
        out[name] = dict(records=n, k=q.dims()[1], mine_ms=stats(mine), host_route_ms=stats(host), same_columns=cols[0] == cols[1],
                         pcie_bytes_mine=28, pcie_bytes_host_route=2 * n * out["record_bytes"])
        q.close()
        h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
