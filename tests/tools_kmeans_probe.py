"""What clusterparts.m's k-means restarts cost on the device (pbd_cluster_parts) beside the same definition on the host
(pbd_cluster_parts_host, one thread) on the same machine.

The person tree (26 parts), --k clusters per part, --trials restarts per part, --n positives whose part offsets are drawn around six
poses per part.  In one process: the device call (upload, the three kernels, the winners and per-trial scalars back; it allocates and
frees its own buffers every call), warm-up calls first, then --reps timed calls; then --host-reps calls of the host function.  Host
clock around each synchronous call; one JSON line: median [first quartile, third quartile] in ms, the ratio of the medians, and whether both
gave the same bytes.
    python tests/tools_kmeans_probe.py [--n 2000] [--k 6] [--trials 100] [--reps 10]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from partsbaseddetector_amd import capi  # noqa: E402
from partsbaseddetector_amd.model import PERSON_TREE  # noqa: E402


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    P = len(PERSON_TREE)
    rng = np.random.default_rng(1)
    poses = rng.uniform(-20, 20, (P, 6, 2))
    d = np.stack([poses[p][rng.integers(0, 6, a.n)] + rng.normal(0, 1.5, (a.n, 2)) for p in range(P)])
    args = dict(R=a.trials, seed=7, max_iter=1000)
    dev_ms, host_ms = [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        got = capi.cluster_parts(d, PERSON_TREE, a.k, **args)
        t1 = time.perf_counter()
        if r >= a.warmup:
            dev_ms.append((t1 - t0) * 1e3)
    for r in range(a.host_reps):
        t0 = time.perf_counter()
        want = capi.cluster_parts_host(d, PERSON_TREE, a.k, **args)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    same = all(got[k].tobytes() == want[k].tobytes() for k in ("idx", "centres", "sumdist", "best_trial", "trial_sumdist", "trial_iters"))
    print(json.dumps(dict(parts=P, k=a.k, trials=a.trials, n=a.n, device_ms=stats(dev_ms), host_ms=stats(host_ms),
                          host_over_device=round(statistics.median(host_ms) / statistics.median(dev_ms), 2), same_bytes=same,
                          capped=got["capped"], passes_mean=float(got["trial_iters"].mean()), passes_max=int(got["trial_iters"].max()))))


if __name__ == "__main__":
    main()
