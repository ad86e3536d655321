"""What the virtual copies of one frame cost on the device beside the same definition on the host (pbd_augment_host_u8, one thread) on the
same machine.

One 640 x 480 x 3 frame into ten variants: the frame and its mirror, each as a plain copy and turned by +-7.5 and +-15 degrees
(bilinear).  Three routes: pbd_augment_u8 (host in, host out: the frame goes up, ten canvases come back), pbd_augment_dev_u8 (the
frame and the canvases are resident: only the ops' descriptors cross PCIe) and pbd_augment_host_u8.  Warm-up rounds first; then the
routes are timed interleaved, one call each per round, with the host clock around each synchronous call (the device calls allocate and
free their own buffers every call, as a caller sees them).  One JSON line: median [first quartile, third quartile] in ms per route, the
bytes that cross PCIe per route, and whether all three gave the same bytes.
    python tests/tools_augment_probe.py [--w 640] [--h 480] [--rounds 21]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from partsbaseddetector_amd import capi  # noqa: E402


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(ms), 4))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    im = np.random.default_rng(1).integers(0, 256, (a.h, a.w, 3), dtype=np.uint8)
    specs = [(f, d, "bilinear") for f in (False, True) for d in (None, 7.5, -7.5, 15.0, -15.0)]
    ops = capi.augment_ops(specs)
    canv = [capi.augment_canvas(a.w, a.h, ops[i]) for i in range(len(specs))]
    out_bytes = sum(r * c * 3 for r, c in canv)
    t = torch.from_numpy(im).cuda()
    host_bufs = [np.zeros((r, c * 3), np.uint8) for r, c in canv]
    up_bufs = [np.zeros((r, c * 3), np.uint8) for r, c in canv]
    dev_bufs = [torch.zeros((r, c * 3), dtype=torch.uint8, device="cuda") for r, c in canv]
    ms = dict(upload=[], resident=[], host=[])
    for r in range(a.warmup + a.rounds):
        for name, call in (("upload", lambda: capi.augment(im, ops, outs=up_bufs)), ("resident", lambda: capi.augment_dev(t, ops, outs=dev_bufs)),
                           ("host", lambda: capi.augment_host(im, ops, outs=host_bufs))):
            t0 = time.perf_counter()
            call()
            if r >= a.warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(h, u) and np.array_equal(h, d.cpu().numpy()) for h, u, d in zip(host_bufs, up_bufs, dev_bufs))
    desc_bytes = 88 * len(specs)      # sizeof(AugDesc) per op
    print(json.dumps(dict(w=a.w, h=a.h, variants=len(specs), canvas_bytes=out_bytes, upload_ms=stats(ms["upload"]), resident_ms=stats(ms["resident"]),
                          host_ms=stats(ms["host"]), pcie_bytes=dict(upload=im.nbytes + out_bytes + desc_bytes, resident=desc_bytes, host=0),
                          host_over_upload=round(statistics.median(ms["host"]) / statistics.median(ms["upload"]), 2),
                          host_over_resident=round(statistics.median(ms["host"]) / statistics.median(ms["resident"]), 2), same_bytes=same)))


if __name__ == "__main__":
    main()
