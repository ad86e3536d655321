"""What the device candidate filter (pbd_set_candidate_filter) costs, against the host post-step it replaces.

The person model (26 parts x 6 mixtures) with bench.py's threshold (99.9th percentile of the seed frame's root scores):
  throughput — the benched call shape: batches of 16 resident frames, 3 handles in flight, graph replay; frames/s of
               (a) the filter off, (b) device sort + NMS 0.1, (c) the filter off plus pbd_candidates_sort + pbd_candidates_nms(0.1)
               per frame on the collecting thread;
  latency    — one pbd_detect_u8 at a time, median ms, filter off and on (sort + NMS 0.1);
  host step  — median ms per frame of the two host functions alone.
One JSON line per size.  --only-filter runs nothing but filtered batches (for a rocprofv3 --kernel-trace --stats run).
    python tests/tools_candidate_filter_probe.py [--sizes 640x480,1920x1080] [--steps 40] [--only-filter]"""
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

B, INFLIGHT = 16, 3


def threshold(model, w, hgt):
    model.thresh = 3.0e38
    h = capi.Handle(model)
    h.detect(make_image(0, w, hgt))
    h._geo = h.geometry(w, hgt)
    vals = np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])])
    h.close()
    return float(np.float32(np.percentile(vals, 99.9)))


class Out:
    def __init__(self, mp, cap):
        self.cap = cap
        self.heads = np.zeros(B * cap, capi.HEAD_DTYPE)
        self.boxes = np.zeros((B * cap, mp, 4), np.int32)
        self.locs = np.zeros((B * cap, mp, 3), np.int32)
        self.counts = np.zeros(B, np.int32)

    def collect(self, h):
        h._chk(h.L.pbd_detect_batch_collect(h.h, self.heads.ctypes.data_as(C.c_void_p), capi._p(self.boxes, C.c_int32),
                                            capi._p(self.locs, C.c_int32), self.cap, capi._p(self.counts, C.c_int32)))


def host_step(out, mp, w, hgt):
    L = capi.lib()
    kept = C.c_int(0)
    for f in range(B):
        o = f * out.cap
        hp = out.heads[o:].ctypes.data_as(C.c_void_p)
        bp, lp = capi._p(out.boxes[o:], C.c_int32), capi._p(out.locs[o:], C.c_int32)
        L.pbd_candidates_sort(hp, bp, lp, int(out.counts[f]), mp)
        L.pbd_candidates_nms(hp, bp, lp, int(out.counts[f]), mp, w, hgt, C.c_float(0.1), C.byref(kept))


def throughput(model, d_frames, w, hgt, mode, steps, host=False):
    maxc = (4096 if w * hgt <= 640 * 480 else 32768) * B   # bench.py's device list for a batch
    print(f"# {w}x{hgt} throughput mode {mode}{' + host step' if host else ''}", file=sys.stderr, flush=True)
    hs = [capi.Handle(model, graph=1, max_candidates=maxc, cand_filter=(mode, 0.1)) for _ in range(INFLIGHT)]
    outs = [Out(hs[0].max_parts, 4096 if w * hgt <= 640 * 480 else 32768) for _ in hs]
    kept = 0

    def run(n):
        nonlocal kept
        for i in range(n + INFLIGHT):
            k = i % INFLIGHT
            if i >= INFLIGHT:
                outs[k].collect(hs[k])
                if host:
                    host_step(outs[k], hs[k].max_parts, w, hgt)
                kept = int(outs[k].counts.sum())
            if i < n:
                hs[k].enqueue_batch_dev(d_frames.data_ptr(), B, w, hgt, 3)
    try:
        run(3 * INFLIGHT)
    except capi.PbdError:
        print(f"# counts {[o.counts.tolist() for o in outs]}", file=sys.stderr, flush=True)
        raise
    t0 = time.perf_counter()
    run(steps)
    dt = time.perf_counter() - t0
    for h in hs:
        h.close()
    return steps * B / dt, kept


def latency(model, im, mode, reps=30):
    h = capi.Handle(model, graph=1, cand_filter=(mode, 0.1))
    t = []
    for i in range(reps + 5):
        t0 = time.perf_counter()
        h.detect(im)
        t.append(time.perf_counter() - t0)
    h.close()
    return statistics.median(t[5:]) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1920x1080")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--only-filter", action="store_true")
    a = ap.parse_args()
    import torch
    for sz in a.sizes.split(","):
        w, hgt = map(int, sz.split("x"))
        model = make_person_model()
        model.thresh = threshold(model, w, hgt)
        d_frames = torch.from_numpy(np.stack([make_image(i % 8, w, hgt) for i in range(B)])).cuda()
        if a.only_filter:
            fps, _ = throughput(model, d_frames, w, hgt, capi.PBD_CAND_SORT_NMS, a.steps)
            print(json.dumps({"size": sz, "filtered_fps": round(fps, 1)}), flush=True)
            continue
        off, n_raw = throughput(model, d_frames, w, hgt, capi.PBD_CAND_RAW, a.steps)
        dev, n_kept = throughput(model, d_frames, w, hgt, capi.PBD_CAND_SORT_NMS, a.steps)
        hst, _ = throughput(model, d_frames, w, hgt, capi.PBD_CAND_RAW, a.steps, host=True)
        im = make_image(0, w, hgt)
        lat_off = latency(model, im, capi.PBD_CAND_RAW)
        lat_on = latency(model, im, capi.PBD_CAND_SORT_NMS)
        h = capi.Handle(model)
        raw = h.detect(im, capacity=32768)
        h.close()
        t = []
        for _ in range(20):
            t0 = time.perf_counter()
            capi.candidates_nms(*capi.candidates_sort(*raw), w, hgt, 0.1)
            t.append(time.perf_counter() - t0)
        print(json.dumps({"size": sz, "batch": B, "inflight": INFLIGHT, "candidates_per_batch_raw": n_raw, "kept_per_batch": n_kept,
                          "fps_off": round(off, 1), "fps_device_nms": round(dev, 1), "fps_host_nms": round(hst, 1),
                          "latency_ms_off": round(lat_off, 3), "latency_ms_device_nms": round(lat_on, 3),
                          "host_step_ms_per_frame": round(statistics.median(t) * 1e3, 3), "seed_frame_candidates": len(raw[0])}),
              flush=True)


if __name__ == "__main__":
    main()
