"""What the part-wise NMS on the device (pbd_set_candidate_nms PBD_NMS_PARTS) costs, beside the painted NMS and the filter off.

The person model (26 parts x 6 mixtures) with bench.py's threshold (99.9th percentile of the seed frame's root scores); overlap 0.3,
top 1000 (testmodel.m's nms(box, 0.3)):
  throughput — the benched call shape: batches of 16 resident frames, 3 handles in flight, graph replay; frames/s with the filter
               off, with sort + painted NMS, and with sort + parts NMS; raw and kept records per batch;
  latency    — one pbd_detect_u8 at a time, median ms, for the same three;
  host step  — median ms of pbd_candidates_sort + pbd_candidates_nms_parts on the seed frame.
One JSON line per size.  --only-parts runs nothing but parts-NMS batches (for a kernel-trace run of its own: k_cand_parts).
    python tests/tools_nms_parts_probe.py [--sizes 640x480,1920x1080] [--steps 40] [--only-parts]"""
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
OVERLAP, TOP = 0.3, 1000
OFF = (capi.PBD_CAND_RAW, capi.PBD_NMS_PAINTED)
PAINTED = (capi.PBD_CAND_SORT_NMS, capi.PBD_NMS_PAINTED)
PARTS = (capi.PBD_CAND_SORT_NMS, capi.PBD_NMS_PARTS)


def threshold(model, w, hgt):
    model.thresh = 3.0e38
    h = capi.Handle(model)
    h.detect(make_image(0, w, hgt))
    h._geo = h.geometry(w, hgt)
    vals = np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])])
    h.close()
    return float(np.float32(np.percentile(vals, 99.9)))


def handle(model, cfg, **kw):
    return capi.Handle(model, graph=1, cand_filter=(cfg[0], OVERLAP), cand_nms=(cfg[1], TOP), **kw)


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


def throughput(model, d_frames, w, hgt, cfg, steps):
    large = w * hgt > 640 * 480
    print(f"# {w}x{hgt} throughput {cfg}", file=sys.stderr, flush=True)
    hs = [handle(model, cfg, max_candidates=(32768 if large else 4096) * B) for _ in range(INFLIGHT)]   # bench.py's device list for a batch
    outs = [Out(hs[0].max_parts, 32768 if large else 4096) for _ in hs]
    count = 0

    def run(n):
        nonlocal count
        for i in range(n + INFLIGHT):
            k = i % INFLIGHT
            if i >= INFLIGHT:
                outs[k].collect(hs[k])
                count = int(outs[k].counts.sum())
            if i < n:
                hs[k].enqueue_batch_dev(d_frames.data_ptr(), B, w, hgt, 3)
    run(3 * INFLIGHT)
    t0 = time.perf_counter()
    run(steps)
    dt = time.perf_counter() - t0
    for h in hs:
        h.close()
    return steps * B / dt, count


def latency(model, im, cfg, reps=30):
    h = handle(model, cfg)
    t = []
    for _ in range(reps + 5):
        t0 = time.perf_counter()
        h.detect(im)
        t.append(time.perf_counter() - t0)
    h.close()
    return statistics.median(t[5:]) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1920x1080")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--only-parts", action="store_true")
    a = ap.parse_args()
    import torch
    for sz in a.sizes.split(","):
        w, hgt = map(int, sz.split("x"))
        model = make_person_model()
        model.thresh = threshold(model, w, hgt)
        d_frames = torch.from_numpy(np.stack([make_image(i % 8, w, hgt) for i in range(B)])).cuda()
        if a.only_parts:
            fps, _ = throughput(model, d_frames, w, hgt, PARTS, a.steps)
            print(json.dumps({"size": sz, "parts_fps": round(fps, 1)}), flush=True)
            continue
        off, n_raw = throughput(model, d_frames, w, hgt, OFF, a.steps)
        painted, n_painted = throughput(model, d_frames, w, hgt, PAINTED, a.steps)
        parts, n_parts = throughput(model, d_frames, w, hgt, PARTS, a.steps)
        im = make_image(0, w, hgt)
        lat = [latency(model, im, cfg) for cfg in (OFF, PAINTED, PARTS)]
        h = capi.Handle(model)
        raw = h.detect(im, capacity=32768)
        h.close()
        t = []
        for _ in range(20):
            t0 = time.perf_counter()
            kept = capi.candidates_nms_parts(*capi.candidates_sort(*raw), OVERLAP, TOP)
            t.append(time.perf_counter() - t0)
        print(json.dumps({"size": sz, "batch": B, "inflight": INFLIGHT, "overlap": OVERLAP, "top": TOP, "raw_per_batch": n_raw,
                          "kept_per_batch_painted": n_painted, "kept_per_batch_parts": n_parts, "fps_off": round(off, 1),
                          "fps_painted": round(painted, 1), "fps_parts": round(parts, 1), "latency_ms_off": round(lat[0], 3),
                          "latency_ms_painted": round(lat[1], 3), "latency_ms_parts": round(lat[2], 3),
                          "host_step_ms_seed_frame": round(statistics.median(t) * 1e3, 3), "seed_frame_raw": len(raw[0]),
                          "seed_frame_kept": len(kept[0])}), flush=True)


if __name__ == "__main__":
    main()
