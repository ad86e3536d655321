"""What the training example cache on the device (pbd_qp_write / _score / _lincomb) costs beside the route available without it.

The person model (26 parts x 6 mixtures) at 640x480, batch off: one detect at thresh = -1 (raised, if need be, to the score of the
--records-th best root) with sort + nms.m's part-wise NMS (overlap 0.3, the 1000 best), then
  write      pbd_qp_write of the frame's records into an empty cache: hipEvents on the handle's stream around the call (the records'
             upload is inside), and the host clock around call + synchronise;
  host write pbd_candidates_features to the host, then tests/qp_ref.py's write of them: host clock, the two parts apart;
  score      pbd_qp_score_dev over a FULL cache of --examples examples (the frame's records, repeated), hipEvents; beside it the
             compiled-order numpy score (qp_ref.score_ref) of the same columns, host clock;
  lincomb    pbd_qp_lincomb_dev over the same cache, all examples in order, hipEvents; beside it qp_ref.lincomb_ref, host clock.
Warm-up calls first, then --reps timed calls each; one JSON line: median [first quartile, third quartile] in ms, the cache's size, and
whether the device results equal the numpy ones in bits.
    python tests/tools_qp_probe.py [--size 640x480] [--reps 20] [--examples 1024] [--records 20000]"""
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
from tests import qp_ref  # noqa: E402

CAP = 65536


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(ms), 4))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--examples", type=int, default=1024)
    ap.add_argument("--records", type=int, default=20000)
    ap.add_argument("--host-examples", type=int, default=128, help="examples the numpy sweeps are timed on (scaled to the cache)")
    a = ap.parse_args()
    w, hgt = (int(v) for v in a.size.split("x"))
    im = make_image(0, w, hgt)
    model = make_person_model()
    model.thresh = 3.0e38
    h = capi.Handle(model)
    h.detect(im)
    g = h.geometry(w, hgt)
    h._geo = g
    vals = np.sort(np.concatenate([h.root(l, 0)[0].ravel() for l in range(g["nlevels"])]))[::-1]
    h.close()
    model.thresh = max(-1.0, float(vals[min(a.records, len(vals) - 1)]))
    h = capi.Handle(model, max_candidates=CAP, cand_filter=(capi.PBD_CAND_SORT_NMS, 0.3), cand_nms=(capi.PBD_NMS_PARTS, 1000))
    stream = torch.cuda.Stream()
    h.set_stream(stream.cuda_stream)
    heads, _, locs = h.detect(im, CAP)
    n = len(heads)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record(stream)
        t0 = time.perf_counter()
        fn()
        ev[1].record(stream)
        stream.synchronize()
        return ev[0].elapsed_time(ev[1]), (time.perf_counter() - t0) * 1e3

    out = dict(size=a.size, thresh=model.thresh, records_after_nms=n, reps=a.reps)
    # ---- write ----
    q = capi.QpCache(h, max(n, 1), 0.002, 0.002)
    length, k, _, _ = q.dims()
    gpu, wall = [], []
    for r in range(a.warmup + a.reps):
        q.keep(np.zeros(0, np.int32))
        e, t = timed(lambda: q.write(heads, locs, -1, 0))
        if r >= a.warmup:
            gpu.append(e); wall.append(t)
    got = q.get()
    out["write_events_ms"], out["write_wall_ms"] = stats(gpu), stats(wall)
    _, wreg, w0, _ = model.qp_vectors()
    feat, ref = [], []
    for r in range(1 + max(a.reps // 4, 2)):
        t0 = time.perf_counter()
        blocks, windows = h.candidates_features(heads, locs)
        t1 = time.perf_counter()
        exp = qp_ref.write_ref(model, heads, locs, blocks, windows, -1, 0, 0.002, 0.002, wreg, w0, k)
        t2 = time.perf_counter()
        if r:
            feat.append((t1 - t0) * 1e3); ref.append((t2 - t1) * 1e3)
    out["host_features_ms"], out["host_qp_ref_write_ms"] = stats(feat), stats(ref)
    out["write_equal_bits"] = all(x.tobytes() == y.tobytes() for x, y in zip(got, exp))
    q.close()
    # ---- score and lincomb over a full cache ----
    N = a.examples
    q = capi.QpCache(h, N, 0.002, 0.002)
    while q.dims()[3] < N:
        q.write(heads, locs, -1, 0)
    out["cache"] = dict(examples=N, k=k, len=length, column_bytes=4 * k * N, footprint=q.footprint())
    rng = np.random.default_rng(0)
    wv, av = rng.normal(0.0, 1.0, length), np.abs(rng.normal(0.0, 1.0, N))
    d_w, d_a = torch.from_numpy(wv).cuda(), torch.from_numpy(av).cuda()
    d_s = torch.zeros(N, dtype=torch.float64, device="cuda")
    d_o = torch.zeros(length, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sc, lc = [], []
    for r in range(a.warmup + a.reps):
        e1, _ = timed(lambda: q.score_dev(d_w.data_ptr(), 0, N, d_s.data_ptr()))
        e2, _ = timed(lambda: q.lincomb_dev(d_a.data_ptr(), 0, N, d_o.data_ptr()))
        if r >= a.warmup:
            sc.append(e1); lc.append(e2)
    out["score_events_ms"], out["lincomb_events_ms"] = stats(sc), stats(lc)
    M = min(a.host_examples, N)
    x = q.get(0, M)[0]
    t0 = time.perf_counter()
    s_ref = qp_ref.score_ref(x, wv, np.arange(M))
    t1 = time.perf_counter()
    l_ref = qp_ref.lincomb_ref(x, av, np.arange(M), length)
    t2 = time.perf_counter()
    out["numpy_score_ms_scaled_to_cache"] = round((t1 - t0) * 1e3 * N / M, 2)
    out["numpy_lincomb_ms_scaled_to_cache"] = round((t2 - t1) * 1e3 * N / M, 2)
    out["numpy_examples_timed"] = M
    out["score_equal_bits"] = d_s.cpu().numpy()[:M].tobytes() == s_ref.tobytes()
    q.lincomb_dev(d_a.data_ptr(), 0, M, d_o.data_ptr())
    stream.synchronize()
    out["lincomb_equal_bits"] = d_o.cpu().numpy().tobytes() == l_ref.tobytes()
    q.close()
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
