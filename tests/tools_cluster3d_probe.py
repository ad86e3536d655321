"""What the object clusters (pbd_set_cluster3d / pbd_candidates_cluster3d, k_cluster3d.hip) cost, against the host restatement.

The person model with bench.py's threshold, the fixed synthetic depth scene of tools_depth_filter_probe.py, the camera of
tools_box3d_probe.py, the reference's tolerance 0.010:
  volume     — the seed frame's raw records, their 3-D boxes (pbd_candidates_box3d) and the points cropped per record;
  primitive  — pbd_candidates_cluster3d on those boxes and on 1 000 records (the boxes repeated), median ms, against
               tests/cluster3d_ref.py on one core (numpy / scipy);
  throughput — batches of 16 resident frames, SORT_NMS 0.1, 3 handles in flight, box3d on: frames/s of
               pbd_detect_batch_rgbd_enqueue_dev_u8 with the cluster step off and on, interleaved.
One JSON line per size.
    python tests/tools_cluster3d_probe.py [--sizes 640x480,1920x1080] [--steps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from partsbaseddetector_amd import capi  # noqa: E402
from partsbaseddetector_amd.model import make_image, make_person_model  # noqa: E402
from tests import cluster3d_ref  # noqa: E402
from tests.tools_box3d_probe import CAM, timed  # noqa: E402
from tests.tools_candidate_filter_probe import B, INFLIGHT, Out, threshold  # noqa: E402
from tests.tools_depth_filter_probe import scene  # noqa: E402


def throughput(model, d_frames, d_depths, w, hgt, on, steps):
    cap = 4096 if w * hgt <= 640 * 480 else 32768
    print(f"# {w}x{hgt} throughput cluster3d {'on' if on else 'off'}", file=sys.stderr, flush=True)
    hs = [capi.Handle(model, graph=1, max_candidates=cap * B, cand_filter=(capi.PBD_CAND_SORT_NMS, 0.1)) for _ in range(INFLIGHT)]
    for h in hs:
        h.set_box3d(True, CAM)
        h.set_cluster3d(on, 0.01)
    outs = [Out(hs[0].max_parts, cap) for _ in hs]

    def run(n):
        for i in range(n + INFLIGHT):
            k = i % INFLIGHT
            if i >= INFLIGHT:
                outs[k].collect(hs[k])
            if i < n:
                hs[k].enqueue_batch_rgbd_dev(d_frames.data_ptr(), d_depths.data_ptr(), B, w, hgt, 3)
    run(2 * INFLIGHT)
    t0 = time.perf_counter()
    run(steps)
    dt = time.perf_counter() - t0
    for h in hs:
        h.close()
    return steps * B / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480")
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import torch
    for sz in a.sizes.split(","):
        w, hgt = map(int, sz.split("x"))
        model = make_person_model()
        model.thresh = threshold(model, w, hgt)
        im, depth = make_image(0, w, hgt), scene(0, w, hgt)
        cloud = cluster3d_ref.depth_cloud(depth, CAM)
        h = capi.Handle(model, max_candidates=32768)
        heads, boxes, _ = h.detect(im, capacity=32768)
        b3, _ = h.candidates_box3d(heads, boxes, depth, w, hgt, CAM)
        n = len(b3)
        b1k = np.tile(b3, int(np.ceil(1000 / max(n, 1))))[:1000]
        got = h.candidates_cluster3d(cloud, b3)
        prim_frame = timed(lambda: h.candidates_cluster3d(cloud, b3), 5)
        prim_1k = timed(lambda: h.candidates_cluster3d(cloud, b1k), 3)
        h.close()
        t0 = time.perf_counter()
        exp = cluster3d_ref.cluster_objects(cloud, b3)
        ref_frame = (time.perf_counter() - t0) * 1e3
        same = bool(all(np.array_equal(got[0][f], exp[0][f]) for f in ("cropped", "nclusters", "size", "first"))
                    and np.array_equal(got[1], exp[1]))
        crop = got[0]["cropped"]
        d_frames = torch.from_numpy(np.stack([make_image(i % 8, w, hgt) for i in range(B)])).cuda()
        d_depths = torch.from_numpy(np.stack([scene(i % 8, w, hgt) for i in range(B)])).cuda()
        runs = {False: [], True: []}
        for rep in range(2):
            for on in (False, True):
                runs[on].append(throughput(model, d_frames, d_depths, w, hgt, on, a.steps))
        print(json.dumps({"size": sz, "seed_frame_raw": n, "records_with_points": int((crop > 0).sum()),
                          "cropped_per_record_median": int(np.median(crop[crop > 0])) if (crop > 0).any() else 0,
                          "cropped_per_record_max": int(crop.max(initial=0)), "kept_per_frame": int(got[0]["size"].sum()),
                          "primitive_ms_frame": round(prim_frame, 3), "primitive_ms_1000": round(prim_1k, 3),
                          "host_restatement_ms_frame": round(ref_frame, 1),
                          "host_restatement_ms_1000_est": round(ref_frame * 1000 / max(n, 1), 1),
                          "seed_frame_matches_restatement": same,
                          "batch": B, "inflight": INFLIGHT, "fps_box3d_only": [round(r, 1) for r in runs[False]],
                          "fps_with_clusters": [round(r, 1) for r in runs[True]]}), flush=True)


if __name__ == "__main__":
    main()
