"""tests/cluster3d_ref.py (the restatement the GPU's k_cluster3d is checked against) against a brute-force O(n^2) transcription
of the contract in include/pbd_c.h: the crop, the epsilon-graph in float32, the largest cluster with the tie rule, the double
centroid, and the depth -> cloud rule of the in-frame step."""
import math

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from tests import cluster3d_ref as ref

F32 = np.float32


def box(x, y, z, w, h, d):
    b = np.zeros(1, capi.BOX3D_DTYPE)[0]
    b["x3d"], b["y3d"], b["z3d"], b["width3d"], b["height3d"], b["depth3d"] = x, y, z, w, h, d
    return b


def brute(pts, b, tol):
    """the contract literally: python floats for the box, float32 scalars op by op for d2, a DFS, the tie rule by discovery"""
    w, h, d = float(b["width3d"]), float(b["height3d"]), float(b["depth3d"])
    nan3 = [math.nan] * 3
    if not ((w * h) * d >= 1e-6):
        return 0, 0, 0, -1, nan3, []
    x, y, z = float(b["x3d"]) - w * 0.1, float(b["y3d"]) - h * 0.1, float(b["z3d"]) - d * 0.1
    w, h, d = w * 1.2, h * 1.2, d * 1.2
    lo = [F32(x), F32(y), F32(z)]
    hi = [F32(x + w), F32(y + h), F32(z + d)]
    kept = [i for i, p in enumerate(pts) if all(math.isfinite(float(p[k])) and lo[k] <= p[k] <= hi[k] for k in range(3))]
    if not kept:
        return 0, 0, 0, -1, nan3, []
    tf = F32(tol)
    with np.errstate(over="ignore"):
        r2 = F32(tf * tf)
    n = len(kept)
    adj = [[] for _ in range(n)]
    for a in range(n):
        for c in range(a + 1, n):
            p, q = pts[kept[a]], pts[kept[c]]
            dx, dy, dz = F32(p[0] - q[0]), F32(p[1] - q[1]), F32(p[2] - q[2])
            d2 = F32(F32(F32(dx * dx) + F32(dy * dy)) + F32(dz * dz))
            if d2 <= r2:
                adj[a].append(c); adj[c].append(a)
    seen = [False] * n
    clusters = []
    for s in range(n):   # discovery order = smallest point index first
        if seen[s]:
            continue
        comp, stack = [], [s]
        seen[s] = True
        while stack:
            u = stack.pop()
            comp.append(u)
            for v in adj[u]:
                if not seen[v]:
                    seen[v] = True
                    stack.append(v)
        clusters.append(sorted(comp))
    best = clusters[0]
    for c in clusters[1:]:
        if len(c) > len(best):
            best = c
    ind = [kept[k] for k in best]
    cen = [sum(float(pts[i][k]) for i in ind) / len(ind) for k in range(3)]
    return n, len(clusters), len(ind), ind[0], cen, ind


def check(pts, boxes, tol, exact_centre=False):
    pts = np.asarray(pts, F32).reshape(-1, 3)
    for b in boxes:
        got = ref.cluster_record(pts, b, tol)
        exp = brute(pts, b, tol)
        assert got[:4] == exp[:4], (got[:4], exp[:4])
        assert list(got[5]) == exp[5]
        if exp[2] == 0:
            assert np.all(np.isnan(got[4]))
        elif exact_centre:
            assert list(got[4]) == exp[4]
        else:
            np.testing.assert_allclose(got[4], exp[4], rtol=1e-12)


@pytest.mark.parametrize("seed", range(6))
def test_random_clouds(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(20, 300))
    pts = rng.uniform(0, 0.08, (n, 3)).astype(F32)
    pts[rng.random(n) < 0.05] = np.nan
    pts[rng.random(n) < 0.02, int(rng.integers(3))] = np.inf
    boxes = [box(0.0, 0.0, 0.0, 0.08, 0.08, 0.08), box(0.01, 0.02, 0.0, 0.03, 0.05, 0.06),
             box(*rng.uniform(-0.02, 0.05, 3), *rng.uniform(0.01, 0.08, 3))]
    check(pts, boxes, 0.01 * (1 + seed % 3))


def test_quantised_clouds_exact_centres():
    rng = np.random.default_rng(11)
    pts = (rng.integers(0, 96, (250, 3)) * 2.0 ** -10).astype(F32)
    check(pts, [box(0.0, 0.0, 0.0, 0.09, 0.09, 0.09)], 0.004, exact_centre=True)


def test_faces_inclusive():
    b = box(0.25, 0.25, 0.25, 0.5, 0.5, 0.5)
    lo, hi = ref.crop_bounds(b)
    pts = np.array([lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf),
                    [lo[0], hi[1], lo[2]], [np.nextafter(lo[0], -np.inf), hi[1], lo[2]]], F32)
    assert list(ref.crop(pts, b)) == [0, 1, 4]
    check(pts, [b], 10.0)


def test_non_finite_points():
    pts = np.array([[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [0.51, 0.5, 0.5]], F32)
    b = box(-1e39, -1e39, -1e39, 2e39, 2e39, 2e39)   # min / max at -inf / +inf in float32: only the finiteness test decides
    lo, hi = ref.crop_bounds(b)
    assert np.all(np.isinf(lo)) and np.all(np.isinf(hi))
    assert list(ref.crop(pts, b)) == [0, 4]
    check(pts, [b], 0.02)


def test_volume_threshold_and_sign():
    pts = np.array([[0.0005, 0.5, 0.5], [0.0, 0.0, 0.0]], F32)
    v = box(0.0, 0.0, 0.0, 1e-6, 1.0, 1.0)
    assert float(v["width3d"]) * float(v["height3d"]) * float(v["depth3d"]) == 1e-6
    below = box(0.0, 0.0, 0.0, np.nextafter(1e-6, 0), 1.0, 1.0)
    neg = box(1.0, 0.0, 0.0, -1.0, 1.0, 1.0)            # negative volume: skipped
    inverted = box(1.0, 1.0, 0.0, -1.0, -1.0, 1.0)      # positive volume, min > max on x and y: keeps nothing
    assert ref.crop_bounds(v) is not None and ref.crop_bounds(below) is None and ref.crop_bounds(neg) is None
    lo, hi = ref.crop_bounds(inverted)
    assert lo[0] > hi[0] and lo[1] > hi[1]
    assert ref.cluster_record(pts, v, 0.01)[0] == 1
    for b in (below, neg, inverted):
        assert ref.cluster_record(pts, b, 0.01)[:4] == (0, 0, 0, -1)
    check(pts, [v, below, neg, inverted], 0.01)


def test_d2_equal_r2_joins():
    """tol 2^-4 on a 2^-6 grid: every d2 and r2 is exact, d2 == r2 joins, one grid step more does not"""
    s = 2.0 ** -6
    pts = np.array([[0, 0, 0], [4, 0, 0], [8, 0, 0], [13, 0, 0], [13, 4, 0], [13, 4, 4], [20, 4, 4], [23, 5, 4]], np.float64) * s
    got = ref.cluster_record(pts.astype(F32), box(0, 0, 0, 0.5, 0.5, 0.5), 0.0625)
    assert got[1] == 3 and got[2] == 3 and list(got[5]) == [0, 1, 2]   # {0, 1, 2}, {3, 4, 5}: a tie, {6, 7}
    check(pts, [box(0, 0, 0, 0.5, 0.5, 0.5)], 0.0625, exact_centre=True)


def test_tie_goes_to_smallest_index():
    pts = np.array([[0.5, 0.5, 0.5], [0.9, 0.9, 0.9], [0.505, 0.5, 0.5], [0.905, 0.9, 0.9], [0.2, 0.2, 0.2]], F32)
    for order in ([0, 1, 2, 3, 4], [1, 0, 3, 2, 4], [4, 3, 2, 1, 0]):
        p = pts[order]
        got = ref.cluster_record(p, box(0, 0, 0, 1, 1, 1), 0.01)
        assert got[1] == 3 and got[2] == 2
        assert got[3] == min(np.flatnonzero(np.all(np.abs(p - p[got[3]]) < 0.1, axis=1)))
        assert got[3] == (0 if order[0] != 4 else 1)
        check(p, [box(0, 0, 0, 1, 1, 1)], 0.01)


def test_infinite_r2_joins_everything():
    pts = np.array([[0, 0, 0], [1e30, 0, 0], [-1e30, 5, 0]], F32)
    got = ref.cluster_record(pts, box(-1e31, -1e31, -1e31, 2e31, 2e31, 2e31), 1e20)
    assert got[1] == 1 and got[2] == 3


def test_depth_cloud_rule():
    cam = (525.0, 523.5, 319.5, 239.5, 0.25, -0.5)
    d = np.array([[1.0, 0.0, np.nan, np.inf], [-1.5, 2.0000001, 1e-3, -np.inf]], np.float64)
    c = ref.depth_cloud(d, cam)
    assert c.dtype == F32 and c.shape == (2, 4, 3)
    for v in range(2):
        for u in range(4):
            dv = F32(d[v, u])
            if dv == 0 or not np.isfinite(dv):
                assert np.all(np.isnan(c[v, u]))
                continue
            x = F32(((u - cam[2] - cam[4]) / cam[0]) * float(dv))
            y = F32(((v - cam[3] - cam[5]) / cam[1]) * float(dv))
            assert (c[v, u, 0], c[v, u, 1], c[v, u, 2]) == (x, y, dv)
    assert c[1, 1, 2] == F32(2.0000001)   # a 64F depth is rounded to float first


def test_restatement_table():
    rng = np.random.default_rng(3)
    cloud = rng.uniform(0, 0.05, (6, 7, 3)).astype(F32)
    boxes = np.array([box(0, 0, 0, 0.05, 0.05, 0.05), box(0, 0, 0, 0, 0, 0)])
    out, idx = ref.cluster_objects(cloud, boxes, 0.01)
    assert out["size"].sum() == len(idx) and out["first"][1] == -1 and np.isnan(out["cx"][1])
    assert idx[0] == out["first"][0]
