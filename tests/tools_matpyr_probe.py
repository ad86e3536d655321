"""What the MATLAB pyramid kind (pbd_set_pyramid_kind) costs.

The person model (26 parts x 6 mixtures) with bench.py's kind of threshold (99.9th percentile of the seed frame's root scores in the
default kind), at 640x480, in both kinds, in interleaved rounds (opencv, matlab, opencv, ... so that clock state moves both alike):
  detect  — single pbd_detect_u8 calls on two graph-replaying handles, one per kind: median ms per round, frames/s from it;
  stages  — pbd_get_stage_ms of profiled single frames (eager) on ONE handle switched between the kinds each round (a switch drops
            the plan: the first frames of a round re-plan and are left out): median pyramid and HOG stage per round;
  levels  — the two geometries' level counts, level-image bytes and cells.
One JSON line.
    python tests/tools_matpyr_probe.py [--size 640x480] [--rounds 5] [--steps 30]"""
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

KINDS = (("opencv", capi.PBD_PYRAMID_OPENCV), ("matlab", capi.PBD_PYRAMID_MATLAB))
CAP = 32768


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
        fn()                        # (detect returns after the stream has been synchronised)
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
    im = make_image(0, w, hgt)
    res = {"size": a.size, "rounds": a.rounds, "steps": a.steps, "thresh": model.thresh}
    single = {}
    for name, kind in KINDS:
        h = single[name] = capi.Handle(model, graph=1, max_candidates=CAP)
        h.set_pyramid_kind(kind)
        for _ in range(5):          # eager, capture, replay
            n = len(h.detect(im, CAP)[0])
        g = h.geometry(w, hgt)
        res[f"levels_{name}"] = int(g["nlevels"])
        res[f"level_image_bytes_{name}"] = int(sum(int(x) * int(y) for x, y in zip(g["img_w"], g["img_h"])) * 3 * (8 if kind else 1))
        res[f"cells_{name}"] = h.work()["cells"]
        res[f"candidates_{name}"] = n
    det = {name: [] for name, _ in KINDS}
    for _ in range(a.rounds):
        for name, _ in KINDS:
            det[name].append(timed(lambda: single[name].detect(im, CAP), a.steps))
    for name, _ in KINDS:
        res[f"detect_ms_{name}"] = [round(v, 4) for v in det[name]]
        res[f"frames_per_s_{name}"] = round(1e3 / statistics.median(det[name]), 2)
        single[name].close()
    h = capi.Handle(model, max_candidates=CAP)       # stage times: eager, profiled, both kinds on the same handle
    h.set_profiling(True)
    stages = {name: [] for name, _ in KINDS}
    for _ in range(a.rounds):
        for name, kind in KINDS:
            h.set_pyramid_kind(kind)
            rows = []
            for i in range(a.steps // 2 + 2):
                h.detect(im, CAP)
                if i >= 2:
                    rows.append(h.stage_ms())
            stages[name].append({k: round(float(np.median([r[k] for r in rows])), 4) for k in rows[0]})
    h.close()
    for name, _ in KINDS:
        res[f"stage_ms_{name}"] = stages[name]
    res["detect_ratio"] = round(statistics.median(det["matlab"]) / statistics.median(det["opencv"]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
