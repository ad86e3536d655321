"""What the warped positives cost on the device (pbd_qp_write_warped_u8: k_warp_first + k_warp_second, k_hog over the windows,
k_qp_poswrite), beside the host route that existed before it (numpy windows and features, columns loaded with pbd_qp_put).

--boxes boxes (seeded: sides 24 .. 300 pixels, some across the border) of one make_image frame at the person model's root filter:
  device  pbd_qp_write_warped_u8 into an empty cache with profiling on: the three launch groups between events (pbd_debug_warp_ms)
          and the host clock around the synchronous call (upload of the frame and of the tap tables included); --reps calls,
          median [quartiles] in ms;
  host    tests/warp_ref.window + tests/hog_ref.hog_def + tests/warp_ref.column_ref of --host-boxes of the boxes, then pbd_qp_put:
          seconds per stage, scaled to --boxes.
One JSON line.
    python tests/tools_warp_probe.py [--size 640x480] [--boxes 256] [--reps 10] [--host-boxes 32]"""
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
from tests import warp_ref as wr  # noqa: E402
from tests.hog_ref import hog_def  # noqa: E402


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--boxes", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-boxes", type=int, default=32)
    a = ap.parse_args()
    w, hgt = (int(v) for v in a.size.split("x"))
    im = make_image(0, w, hgt)
    model = make_person_model()
    h = capi.Handle(model)
    rng = np.random.default_rng(0)
    bw, bh = rng.integers(24, 301, a.boxes), rng.integers(24, 301, a.boxes)
    x1, y1 = rng.integers(-20, w - 20, a.boxes), rng.integers(-20, hgt - 20, a.boxes)
    boxes = np.stack([x1, y1, x1 + bw - 1, y1 + bh - 1], axis=1).astype(np.float64)
    filter, bias = model.filterid[0][0][0], model.biasid[0][0][0]
    kh, kw = h.filter_size(filter)
    geo = [wr.geometry(b, kh, kw, model.sbin) for b in boxes]
    out = dict(size=a.size, boxes=a.boxes, filter=[kh, kw, model.sbin],
               taps=int(sum(g["oh"] * g["py"] + g["ow"] * g["px"] for g in geo)),
               intermediate_mb=round(sum((g["oh"] * g["cw"] if g["rows_first"] else g["ch"] * g["ow"]) * 24 for g in geo) / 2 ** 20, 2))
    h.set_profiling(True)
    wall, ev = [], []
    for r in range(a.warmup + a.reps):
        q = capi.QpCache(h, a.boxes, 0.002, 0.002)
        t0 = time.perf_counter()
        written, _ = q.write_warped(im, boxes, filter, bias)
        t1 = time.perf_counter()
        assert written == a.boxes
        if r >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            ev.append(h.warp_ms())
        if r + 1 < a.warmup + a.reps:
            q.close()
    out["device"] = dict(call_ms=stats(wall), resample_ms=stats([e[0] for e in ev]), hog_ms=stats([e[1] for e in ev]),
                         write_ms=stats([e[2] for e in ev]))
    q.close()
    # the host route
    nh = min(a.host_boxes, a.boxes)
    _, wreg, w0, _ = model.qp_vectors()
    q = capi.QpCache(h, nh, 0.002, 0.002)
    k = q.dims()[1]
    t0 = time.perf_counter()
    wins = [wr.window(im, b, kh, kw, model.sbin) for b in boxes[:nh]]
    t1 = time.perf_counter()
    feats = [hog_def(x, model.sbin)[0] for x in wins]
    t2 = time.perf_counter()
    cols = [wr.column_ref(model, f, filter, bias, i, 0.002, wreg, w0, k) for i, f in enumerate(feats)]
    t3 = time.perf_counter()
    q.put(np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols]), np.array([c[2] for c in cols], np.float32),
          np.array([c[3] for c in cols]))
    t4 = time.perf_counter()
    s = a.boxes / nh
    out["host_s_scaled"] = dict(windows=round((t1 - t0) * s, 3), features=round((t2 - t1) * s, 3), columns=round((t3 - t2) * s, 3),
                                put=round((t4 - t3) * s, 3), total=round((t4 - t0) * s, 3), measured_boxes=nh)
    # (the two routes' columns are not compared here: the host route's features are float64 and windows that cross the right border
    #  hold exact orientation ties that either evaluation may break the other way — tests/warp_cases.py; tests/test_gpu_warp.py is the check)
    q.close()
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
