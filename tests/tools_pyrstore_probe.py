"""What the pyramid store (include/pbd_c.h "pyramid store", k_pyrstore.hip) costs and saves.  One session, the image path and the stored
path alternating; one JSON line per measurement:
  load       k_pyrstore_load at 640x480, intervals 2 and 10, a float handle with the split bank and a double handle: GPU time from the
             handle's stage events (the load stands where the image pyramid stood: stage 0), its bytes (read + written, the split parts
             included) over that time, and beside it a device-to-device copy of the frame's feature block alone (torch, device events):
             the copy half of the hipMemcpyAsync + k_feat_split pair the load replaces.  The split half is not timed on its own.
  front      the share of a plain frame the store removes: stage times (image pyramid + HOG) / total of the same handles, profiling on.
  mine       QpCache.mine_stored against QpCache.mine per frame (host clock around the synchronous call, the cache cleared outside the
             window), interval 2, for init_model's one-filter model and the 26 x 6 person model.
  train      train_model wall time with and without share_pyramids on a synthetic set (ten 96 x 96 positives of three parts,
             --negatives noise frames of 320 x 240).
  footprint  bytes of a slot per 640x480 frame, both intervals, float and double (host arithmetic: pbd_pyrstore_layout).
    python tests/tools_pyrstore_probe.py [--reps 30] [--negatives 16] [--skip-train | --only-train]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from partsbaseddetector_amd import capi  # noqa: E402
from partsbaseddetector_amd.model import init_model, make_image, make_person_model  # noqa: E402
from partsbaseddetector_amd.train import train_model  # noqa: E402

W, H = 640, 480


def at_interval(model, iv):
    model.interval = iv
    return model


def one_filter():
    m = init_model(None, None, 4, tsize=(5, 5))
    m.filtersw[0][:] = np.random.default_rng(7).standard_normal(m.filtersw[0].shape).astype(np.float32) * 0.1
    return m


def threshold(h, im, pct):
    h.pyramid(im); h.pdf(); h.dp_min()
    v = np.concatenate([h.root(l, c)[0].ravel() for l in range(h._geo["nlevels"]) for c in range(h.model.ncomponents)])
    return float(np.float32(np.percentile(v[np.isfinite(v)], pct)))


def load_probe(iv, dtype, bank, reps):
    import torch
    ims = [make_image(s, W, H) for s in range(4)]
    prod = capi.Handle(at_interval(one_filter(), iv), dtype=dtype, conv_mode=capi.PBD_CONV_EXACT)
    cons = capi.Handle(at_interval(make_person_model(), iv), dtype=dtype, conv_mode=bank, max_candidates=32768)
    cons.set_threshold(threshold(cons, ims[0], 99.9))
    store = capi.PyramidStore(prod, len(ims), W, H)
    for i, im in enumerate(ims):
        store.put(i, im)
    esz = np.dtype(dtype).itemsize
    elems = capi.pyrstore_layout(W, H, 4, iv)[2]
    parts = {capi.PBD_CONV_SPLIT: 3, capi.PBD_CONV_SPLIT_F16: 2}.get(cons.conv_mode, 0)
    nbytes = elems * esz * 2 + elems * 2 * parts            # the slot read, the features written, the 16-bit parts written
    cons.set_profiling(True)
    t_load, t_front, t_total = [], [], []
    for r in range(reps + 5):                                # alternating: a stored frame, a plain frame
        cons.detect_stored(store, r % len(ims), capacity=32768)
        a = cons.stage_ms()
        cons.detect(ims[r % len(ims)], capacity=32768)
        b = cons.stage_ms()
        if r >= 5:
            t_load.append(a["image_pyramid"]); t_front.append(b["image_pyramid"] + b["hog"]); t_total.append(b["total"])
    src = torch.empty(elems * esz, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    t_copy = []
    for r in range(reps + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record(); e1.synchronize()
        if r >= 5:
            t_copy.append(e0.elapsed_time(e1))
    ms = statistics.median(t_load)
    out = dict(what="load", interval=iv, dtype=np.dtype(dtype).name, split_parts=parts, feature_bytes=elems * esz, moved_bytes=nbytes,
               load_ms=round(ms, 4), load_ms_min=round(min(t_load), 4), load_GBps=round(nbytes / ms / 1e6, 1),
               d2d_copy_ms=round(statistics.median(t_copy), 4), d2d_copy_GBps=round(2 * elems * esz / statistics.median(t_copy) / 1e6, 1),
               plain_front_end_ms=round(statistics.median(t_front), 4), plain_total_ms=round(statistics.median(t_total), 4),
               front_end_share=round(statistics.median(t_front) / statistics.median(t_total), 3))
    store.close(); prod.close(); cons.close()
    return out


def mine_probe(name, model, reps):
    ims = [make_image(s, W, H) for s in range(4)]
    prod = capi.Handle(at_interval(one_filter(), 2))
    h = capi.Handle(at_interval(model, 2), max_candidates=32768)
    h.set_threshold(threshold(h, ims[0], 99.9))
    q = capi.QpCache(h, 4096, 0.004, 0.002)
    store = capi.PyramidStore(prod, len(ims), W, H)
    for i, im in enumerate(ims):
        store.put(i, im)
    t = {"image": [], "stored": []}
    recs = 0
    for r in range(reps + 5):
        for how in ("image", "stored"):
            q.clear()
            t0 = time.perf_counter()
            got = q.mine(ims[r % 4], 1) if how == "image" else q.mine_stored(store, r % 4, 1)
            dt = time.perf_counter() - t0
            recs = got[0]
            if r >= 5:
                t[how].append(dt * 1e3)
    out = dict(what="mine", model=name, interval=2, records_per_frame=recs, mine_u8_ms=round(statistics.median(t["image"]), 4),
               mine_stored_ms=round(statistics.median(t["stored"]), 4),
               saved_share=round(1 - statistics.median(t["stored"]) / statistics.median(t["image"]), 3))
    q.close(); store.close(); prod.close(); h.close()
    return out


def train_probe(nneg):
    from tests.test_gpu_train import KS, PARENTS, synthetic
    positives, _ = synthetic()
    rng = np.random.default_rng(5)
    negatives = [rng.integers(90, 130, (240, 320, 3)).astype(np.uint8) for _ in range(nneg)]
    kw = dict(tsize=(5, 5), R=4, max_iter=200, max_candidates=65536)   # (every root cell of a negative is a record at threshold -1)
    t = {False: [], True: []}
    models = {}
    for rep in range(2):                                     # alternating: plain, shared, plain, shared
        for share in (False, True):
            t0 = time.perf_counter()
            models[share], _ = train_model(positives, negatives, KS, PARENTS, 4, share_pyramids=share, **kw)
            t[share].append(time.perf_counter() - t0)
    return dict(what="train", positives=len(positives), negatives=nneg, trainings=sum(KS) + 2, plain_s=[round(v, 3) for v in t[False]],
                shared_s=[round(v, 3) for v in t[True]], same_weights=bool(models[False].weight_vector().tobytes() == models[True].weight_vector().tobytes()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--negatives", type=int, default=16)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--only-train", action="store_true")
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                            # (torch's runtime first, as the other probes have it: it finds no device behind the library's)
    if a.only_train:
        print(json.dumps(train_probe(a.negatives)), flush=True)
        return
    for iv in (2, 10):
        n, _, total = capi.pyrstore_layout(W, H, 4, iv)
        print(json.dumps(dict(what="footprint", size=f"{W}x{H}", interval=iv, levels=n, float_bytes=total * 4, double_bytes=total * 8)), flush=True)
    for iv in (2, 10):
        for dtype, bank in ((np.float32, capi.PBD_CONV_SPLIT), (np.float64, capi.PBD_CONV_MFMA)):
            print(json.dumps(load_probe(iv, dtype, bank, a.reps)), flush=True)
    print(json.dumps(mine_probe("one_filter", one_filter(), a.reps)), flush=True)
    print(json.dumps(mine_probe("person_26x6", make_person_model(), a.reps)), flush=True)
    if not a.skip_train:
        print(json.dumps(train_probe(a.negatives)), flush=True)


if __name__ == "__main__":
    main()
