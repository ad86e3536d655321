"""What the boundary padding (pbd_set_boundary_pad) costs.

The person model (26 parts x 6 mixtures) with bench.py's kind of threshold (99.9th percentile of the seed frame's unpadded root
scores), at 640x480, pad 0 and 3 on two handles, in interleaved rounds (pad 0, pad 3, pad 0, ... so that clock state moves both alike):
  detect  — one pbd_detect_u8 at a time, graph replay, median ms per round;
  batch   — pbd_detect_batch_u8 of 16 frames, graph replay, median ms per frame per round;
  stages  — pbd_get_stage_ms of profiled single frames (eager), median of each stage;
  cells   — the plan's cell counts (pbd_get_work).
One JSON line.
    python tests/tools_pad_probe.py [--size 640x480] [--rounds 5] [--steps 30]"""
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

B = 16


def threshold(model, w, hgt):
    model.thresh = 3.0e38
    h = capi.Handle(model)
    h.detect(make_image(0, w, hgt))
    h._geo = h.geometry(w, hgt)
    vals = np.concatenate([h.root(l, 0)[0].ravel() for l in range(h._geo["nlevels"])])
    h.close()
    return float(np.float32(np.percentile(vals, 99.9)))


def timed(fn, steps):
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    w, hgt = (int(v) for v in a.size.split("x"))
    model = make_person_model()
    model.thresh = threshold(model, w, hgt)
    frames = [make_image(i, w, hgt) for i in range(B)]
    pads = (0, 3)
    res = {"size": a.size, "rounds": a.rounds, "steps": a.steps, "thresh": model.thresh}
    single, batch = {}, {}
    for p in pads:
        single[p] = capi.Handle(model, graph=1, max_candidates=32768)
        batch[p] = capi.Handle(model, graph=1, max_candidates=32768 * 4)
        single[p].set_boundary_pad(p)
        batch[p].set_boundary_pad(p)
        for _ in range(5):   # eager, capture, replay
            single[p].detect(frames[0], 32768)
            batch[p].detect_batch(frames, 8192)
        res[f"cells_pad{p}"] = single[p].work()["cells"]
        res[f"candidates_pad{p}"] = len(single[p].detect(frames[0], 32768)[0])
    det = {p: [] for p in pads}
    bat = {p: [] for p in pads}
    for _ in range(a.rounds):
        for p in pads:
            det[p].append(timed(lambda: single[p].detect(frames[0], 32768), a.steps))
        for p in pads:
            bat[p].append(timed(lambda: batch[p].detect_batch(frames, 8192), max(3, a.steps // 4)) / B)
    for p in pads:
        res[f"detect_ms_pad{p}"] = [round(v, 4) for v in det[p]]
        res[f"batch16_ms_per_frame_pad{p}"] = [round(v, 4) for v in bat[p]]
        single[p].close()
        batch[p].close()
    for p in pads:   # stage times: eager, profiled
        h = capi.Handle(model, max_candidates=32768)
        h.set_boundary_pad(p)
        h.set_profiling(True)
        rows = []
        for i in range(12):
            h.detect(frames[0], 32768)
            if i >= 2:
                rows.append(h.stage_ms())
        res[f"stage_ms_pad{p}"] = {k: round(float(np.median([r[k] for r in rows])), 4) for k in rows[0]}   # (hog: k_hog + the ring)
        h.close()
    res["detect_ratio"] = round(statistics.median(det[3]) / statistics.median(det[0]), 4)
    res["batch_ratio"] = round(statistics.median(bat[3]) / statistics.median(bat[0]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
