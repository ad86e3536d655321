"""What the 3-D boxes (pbd_set_box3d / pbd_candidates_box3d, k_box3d.hip) cost, against the host restatement they replace.

The person model (26 parts x 6 mixtures) with bench.py's threshold (99.9th percentile of the seed frame's root scores) and a
fixed synthetic depth scene (three planes, 1 cm noise, 5 % holes), the camera of a 640x480 Kinect-class sensor:
  primitive  — pbd_candidates_box3d on the RAW records of the seed frame and on 1 000 records (the raw records repeated),
               median ms, against tests/box3d_ref.py on one core (numpy);
  throughput — batches of 16 resident frames, SORT_NMS 0.1, 3 handles in flight: frames/s of
               pbd_detect_batch_rgbd_enqueue_dev_u8 with the step off and on, interleaved;
  volume     — raw records and their points (valid depth pixels under the boxes, with multiplicity) per frame.
One JSON line per size.
    python tests/tools_box3d_probe.py [--sizes 640x480] [--steps 40]"""
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
from tests import box3d_ref  # noqa: E402
from tests.tools_candidate_filter_probe import B, INFLIGHT, Out, threshold  # noqa: E402
from tests.tools_depth_filter_probe import scene  # noqa: E402

CAM = (525.0, 525.0, 319.5, 239.5, 0.0, 0.0)


def throughput(model, d_frames, d_depths, w, hgt, on, steps):
    cap = 4096 if w * hgt <= 640 * 480 else 32768
    print(f"# {w}x{hgt} throughput box3d {'on' if on else 'off'}", file=sys.stderr, flush=True)
    hs = [capi.Handle(model, graph=1, max_candidates=cap * B, cand_filter=(capi.PBD_CAND_SORT_NMS, 0.1)) for _ in range(INFLIGHT)]
    for h in hs:
        h.set_box3d(on, CAM if on else None)
    outs = [Out(hs[0].max_parts, cap) for _ in hs]

    def run(n):
        for i in range(n + INFLIGHT):
            k = i % INFLIGHT
            if i >= INFLIGHT:
                outs[k].collect(hs[k])
            if i < n:
                hs[k].enqueue_batch_rgbd_dev(d_frames.data_ptr(), d_depths.data_ptr(), B, w, hgt, 3)
    run(3 * INFLIGHT)
    t0 = time.perf_counter()
    run(steps)
    dt = time.perf_counter() - t0
    for h in hs:
        h.close()
    return steps * B / dt


def timed(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480")
    ap.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    import torch
    for sz in a.sizes.split(","):
        w, hgt = map(int, sz.split("x"))
        model = make_person_model()
        model.thresh = threshold(model, w, hgt)
        im, depth = make_image(0, w, hgt), scene(0, w, hgt)
        h = capi.Handle(model, max_candidates=32768)
        heads, boxes, _ = h.detect(im, capacity=32768)
        n = len(heads)
        reps = int(np.ceil(1000 / max(n, 1)))
        h1k, b1k = np.tile(heads, reps)[:1000], np.tile(boxes, (reps, 1, 1))[:1000]
        h.candidates_box3d(heads, boxes, depth, w, hgt, CAM)
        prim_frame = timed(lambda: h.candidates_box3d(heads, boxes, depth, w, hgt, CAM), 10)
        prim_1k = timed(lambda: h.candidates_box3d(h1k, b1k, depth, w, hgt, CAM), 5)
        got, _ = h.candidates_box3d(heads, boxes, depth, w, hgt, CAM)
        h.close()
        t0 = time.perf_counter()
        exp, _ = box3d_ref.box3d(heads, boxes, depth, w, hgt, CAM)
        ref_frame = (time.perf_counter() - t0) * 1e3
        pts = [0 if (p := box3d_ref.points_of(boxes[i, :heads["nparts"][i]], depth, w, hgt)) is None else len(p) for i in range(n)]
        d_frames = torch.from_numpy(np.stack([make_image(i % 8, w, hgt) for i in range(B)])).cuda()
        d_depths = torch.from_numpy(np.stack([scene(i % 8, w, hgt) for i in range(B)])).cuda()
        runs = {False: [], True: []}
        for rep in range(2):
            for on in (False, True):
                runs[on].append(throughput(model, d_frames, d_depths, w, hgt, on, a.steps))
        same = bool(np.array_equal(got["valid"], exp["valid"]) and np.array_equal(got["zmin"], exp["zmin"], equal_nan=True)
                    and np.array_equal(got["zmax"], exp["zmax"], equal_nan=True))
        print(json.dumps({"size": sz, "seed_frame_raw": n, "points_per_record_median": int(np.median(pts)) if pts else 0,
                          "points_per_record_max": max(pts, default=0), "points_per_frame": int(sum(pts)),
                          "primitive_ms_frame": round(prim_frame, 3), "primitive_ms_1000": round(prim_1k, 3),
                          "host_restatement_ms_frame": round(ref_frame, 1),
                          "host_restatement_ms_1000_est": round(ref_frame * 1000 / max(n, 1), 1),
                          "seed_frame_matches_restatement": same,
                          "batch": B, "inflight": INFLIGHT, "fps_off": [round(r, 1) for r in runs[False]],
                          "fps_on": [round(r, 1) for r in runs[True]]}), flush=True)


if __name__ == "__main__":
    main()
