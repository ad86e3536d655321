"""What depth-consistency pruning (pbd_set_depth_filter, k_zfilter.hip) costs, against the host restatement it replaces.

The person model (26 parts x 6 mixtures) with bench.py's threshold (99.9th percentile of the seed frame's root scores) and a
fixed synthetic depth scene (three planes, 1 cm noise, 5 % holes), zfactor 0.03 (the reference's commented-out call):
  throughput — the benched call shape: batches of 16 resident frames, 3 handles in flight; frames/s with the filter off
               (plain device batches, graph replay) and on (pbd_detect_batch_rgbd_enqueue_dev_u8, eager launches), interleaved;
  latency    — one detect at a time, median ms, plain pbd_detect_u8 against pbd_detect_rgbd_u8 with the filter on;
  host step  — median ms per frame of tests/depth_ref.py on the seed frame's raw records (numpy, one core);
  volume     — raw and kept records per frame, boxes needing a median and their clipped pixels per frame.
One JSON line per size.  --only-filter runs nothing but filtered batches (for a rocprofv3 --kernel-trace --stats run).
    python tests/tools_depth_filter_probe.py [--sizes 640x480,1920x1080] [--steps 40] [--only-filter]"""
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
from tests import depth_ref  # noqa: E402
from tests.tools_candidate_filter_probe import B, INFLIGHT, Out, threshold  # noqa: E402

ZF = 0.03


def scene(seed, w, hgt):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:hgt, 0:w].astype(np.float64)
    d = 3.0 + 0.002 * yy * 480.0 / hgt
    d = np.where(xx < w * 0.4, 1.2 + 0.0005 * xx * 640.0 / w, d)
    d = np.where((yy > hgt * 0.6) & (xx > w * 0.5), 2.0 + 0.001 * (xx - w * 0.5) * 640.0 / w, d)
    d = d + rng.normal(0, 0.01, d.shape)
    d[rng.random(d.shape) < 0.05] = 0.0
    return d.astype(np.float32)


def throughput(model, d_frames, d_depths, w, hgt, on, steps):
    cap = 4096 if w * hgt <= 640 * 480 else 32768
    print(f"# {w}x{hgt} throughput depth filter {'on' if on else 'off'}", file=sys.stderr, flush=True)
    hs = [capi.Handle(model, graph=1, max_candidates=cap * B) for _ in range(INFLIGHT)]
    for h in hs:
        h.set_depth_filter(on, ZF)
    outs = [Out(hs[0].max_parts, cap) for _ in hs]
    kept = 0

    def run(n):
        nonlocal kept
        for i in range(n + INFLIGHT):
            k = i % INFLIGHT
            if i >= INFLIGHT:
                outs[k].collect(hs[k])
                kept = int(outs[k].counts.sum())
            if i < n:
                if on:
                    hs[k].enqueue_batch_rgbd_dev(d_frames.data_ptr(), d_depths.data_ptr(), B, w, hgt, 3)
                else:
                    hs[k].enqueue_batch_dev(d_frames.data_ptr(), B, w, hgt, 3)
    run(3 * INFLIGHT)
    t0 = time.perf_counter()
    run(steps)
    dt = time.perf_counter() - t0
    for h in hs:
        h.close()
    return steps * B / dt, kept


def latency(model, im, depth, on, reps=30):
    h = capi.Handle(model, graph=1, max_candidates=32768)
    h.set_depth_filter(on, ZF)
    t = []
    for _ in range(reps + 5):
        t0 = time.perf_counter()
        if on:
            h.detect_rgbd(im, depth, capacity=32768)
        else:
            h.detect(im, capacity=32768)
        t.append(time.perf_counter() - t0)
    h.close()
    return statistics.median(t[5:]) * 1e3


def volume(model, raw, w, hgt):
    boxes = pixels = 0
    for i in range(len(raw[0])):
        np_ = model.nparts(int(raw[0]["component"][i]))
        if np_ < 2:
            continue
        b = raw[1][i, :np_].astype(np.int64)
        cw = np.minimum(b[:, 0] + b[:, 2], w) - np.maximum(b[:, 0], 0)
        ch = np.minimum(b[:, 1] + b[:, 3], hgt) - np.maximum(b[:, 1], 0)
        ok = (b[:, 2] > 0) & (b[:, 3] > 0) & (cw > 0) & (ch > 0)
        boxes += np_
        pixels += int((cw * ch)[ok].sum())
    return boxes, pixels


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
        d_depths = torch.from_numpy(np.stack([scene(i % 8, w, hgt) for i in range(B)])).cuda()
        if a.only_filter:
            fps, _ = throughput(model, d_frames, d_depths, w, hgt, True, a.steps)
            print(json.dumps({"size": sz, "filtered_fps": round(fps, 1)}), flush=True)
            continue
        runs = {False: [], True: []}
        for rep in range(2):                       # interleaved: off, on, off, on
            for on in (False, True):
                fps, n = throughput(model, d_frames, d_depths, w, hgt, on, a.steps)
                runs[on].append((fps, n))
        im, depth = make_image(0, w, hgt), scene(0, w, hgt)
        lat_off = latency(model, im, depth, False)
        lat_on = latency(model, im, depth, True)
        h = capi.Handle(model, max_candidates=32768)
        raw = h.detect(im, capacity=32768)
        h.set_depth_filter(True, ZF)
        got = h.detect_rgbd(im, depth, capacity=32768)
        h.close()
        t = []
        for _ in range(3 if w * hgt <= 640 * 480 else 1):
            t0 = time.perf_counter()
            ref = depth_ref.depth_filter(model, *raw, depth, ZF)
            t.append(time.perf_counter() - t0)
        nbox, npix = volume(model, raw, w, hgt)
        print(json.dumps({"size": sz, "batch": B, "inflight": INFLIGHT, "zfactor": ZF,
                          "fps_off": [round(r[0], 1) for r in runs[False]], "fps_on": [round(r[0], 1) for r in runs[True]],
                          "records_per_batch_raw": runs[False][-1][1], "kept_per_batch": runs[True][-1][1],
                          "latency_ms_off": round(lat_off, 3), "latency_ms_on": round(lat_on, 3),
                          "host_restatement_ms_per_frame": round(statistics.median(t) * 1e3, 1),
                          "seed_frame_raw": len(raw[0]), "seed_frame_kept": len(got[0]),
                          "seed_frame_matches_restatement": bool(len(got[0]) == len(ref[0]) and got[0].tobytes() == ref[0].tobytes()),
                          "boxes_per_frame": nbox, "box_pixels_per_frame": npix}), flush=True)


if __name__ == "__main__":
    main()
