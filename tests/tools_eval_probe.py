"""What an APK evaluation batch on the device (pbd_eval_apk_frame_batch_u8) costs beside the route it replaces.

The person model (26 parts x 6 mixtures) on a batch of 640x480 frames (four: from five on the plan is the compact one, which evaluation
frames refuse like mining frames), the threshold at the score of the --records-th best root of the
first frame, sort + nms.m's part-wise NMS (overlap 0.3, the 1000 best: testmodel.m), four persons per frame off its own detections.  In
one process, on one handle, alternating:
  ledger      Eval.reset(); Eval.apk_batch(frames, persons)  — the records stay on the device;
  host route  Handle.detect_batch(frames) — every record collected into host arrays — then pbd_eval_apk_match_host per frame.
Then the result over --batches batches in the ledger: Eval.apk() beside pbd_eval_ap_host on the same rows.  Host clock around each
synchronous call, warm-up calls first, then --reps timed calls of each route; one JSON line: median [first quartile, third quartile]
in ms, the records, and whether both routes gave the same rows and the same apk.
    python tests/tools_eval_probe.py [--size 640x480] [--batch 4] [--reps 20] [--records 2000] [--batches 8]"""
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

CAP = 65536     # device list of a batch, in front of the filter
KEPT = 1024     # host arrays per frame: nms.m keeps at most the 1000 best


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(ms), 4))


def persons_of(rec, P):
    """four persons off a frame's records: the part centres of its records of rank 0, 1, 2 and 3, shifted by a pixel"""
    heads, boxes = rec[0], rec[1]
    n = min(4, len(heads))
    b = boxes[:n, :P].astype(np.float64)
    pts = np.stack([b[..., 0] + .5 * (b[..., 2] - 1) + 1.0, b[..., 1] + .5 * (b[..., 3] - 1) - 1.0], -1)
    return pts, np.full(n, 20.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--batches", type=int, default=8)
    a = ap.parse_args()
    w, hgt = (int(v) for v in a.size.split("x"))
    frames = [make_image(f, w, hgt) for f in range(a.batch)]
    model = make_person_model()
    P = model.nparts(0)
    model.thresh = 3.0e38
    h = capi.Handle(model)
    h.detect(frames[0])
    h._geo = h.geometry(w, hgt)
    vals = np.sort(np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])]))[::-1]
    h.close()
    model.thresh = float(vals[min(a.records, len(vals) - 1)])
    h = capi.Handle(model, max_candidates=CAP, cand_filter=(capi.PBD_CAND_SORT_NMS, 0.3), cand_nms=(capi.PBD_NMS_PARTS, 1000))
    recs = h.detect_batch(frames, KEPT)
    persons = [persons_of(r, P) for r in recs]
    m = sum(len(r[0]) for r in recs)
    ev = capi.Eval(h, P, 64 * a.batch, max(m * a.batches, 1))
    ledger, host, rows = [], [], []
    for r in range(a.warmup + a.reps):
        ev.reset()
        t0 = time.perf_counter()
        n = ev.apk_batch(frames, persons)
        t1 = time.perf_counter()
        got = h.detect_batch(frames, KEPT)
        tp = [capi.eval_apk_match_host(g[0], g[1], p[0], p[1], P) for g, p in zip(got, persons)]
        t2 = time.perf_counter()
        assert int(n.sum()) == m == sum(len(g[0]) for g in got)
        if r == 0:
            led = ev.get()
            rows = [led["tp"].tobytes() == np.concatenate(tp).tobytes(), led["score"].tobytes() == np.concatenate([g[0]["score"] for g in got]).tobytes()]
        if r >= a.warmup:
            ledger.append((t1 - t0) * 1e3); host.append((t2 - t1) * 1e3)
    for _ in range(a.batches - 1):
        ev.apk_batch(frames, persons)
    led = ev.get()
    npos = ev.dims()[3]
    dev_ms, host_ms = [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        apk = ev.apk()
        t1 = time.perf_counter()
        e_apk = capi.eval_ap_host(led["score"], led["tp"], npos)
        t2 = time.perf_counter()
        if r >= a.warmup:
            dev_ms.append((t1 - t0) * 1e3); host_ms.append((t2 - t1) * 1e3)
    print(json.dumps(dict(size=a.size, batch=a.batch, thresh=model.thresh, reps=a.reps, records_per_batch=m, keypoints=P,
                          record_bytes=16 + 28 * model.max_parts, ledger_batch_ms=stats(ledger), host_route_batch_ms=stats(host),
                          same_rows=all(rows), result_detections=ev.dims()[2], apk_ms=stats(dev_ms), ap_host_ms=stats(host_ms),
                          same_apk=apk.tobytes() == e_apk.tobytes(), apk_mean=float(np.nanmean(apk)))))
    ev.close()
    h.close()


if __name__ == "__main__":
    main()
