"""numpy / scipy restatement of PointCloudClusterer::clusterObjects (include/PointCloudClusterer.hpp:156-290): the rule the GPU's
k_cluster3d must reproduce (include/pbd_c.h).  It shares nothing with the kernel: candidate pairs come from a k-d
tree at a slightly larger radius and are filtered by the exact float32 d2 <= r2; components from scipy's csgraph.

- crop: volume() in double on the unexpanded box, then x -= 0.1 * w, w *= 1.2 (likewise y, z); min / max rounded to float32;
  a point is kept iff x, y, z are finite and min <= p <= max on every axis as float32 compares;
- d2 = ((dx * dx) + (dy * dy)) + (dz * dz) in float32 (numpy rounds every operation: no FMA), r2 = tol * tol in float32;
- the largest cluster, ties to the one with the smallest point index; its centroid summed in double; its indices ascending.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

F32 = np.float32


def depth_cloud(depth, cam):
    """the in-frame cloud of a depth image (HxW; float64 is rounded to float32 first) through (fx, fy, cx, cy[, tx, ty]):
    z = d, x = (float)(((u - cx - tx) / fx) * d), y = (float)(((v - cy - ty) / fy) * d) in double; d == 0 or non-finite: NaN"""
    fx, fy, cx, cy = (float(v) for v in cam[:4])
    tx, ty = (float(cam[4]), float(cam[5])) if len(cam) > 4 else (0.0, 0.0)
    d = np.asarray(depth).astype(F32)
    h, w = d.shape
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    dd = d.astype(np.float64)
    x = (((u - cx - tx) / fx) * dd).astype(F32)
    y = (((v - cy - ty) / fy) * dd).astype(F32)
    out = np.stack([x, y, d], axis=-1)
    out[(d == 0) | ~np.isfinite(d)] = np.nan
    return out


def crop_bounds(box):
    """(lo, hi) float32 [3] of the expanded box, or None when volume() < 1e-6 (a negative or NaN volume included)"""
    x3d, y3d, z3d = float(box["x3d"]), float(box["y3d"]), float(box["z3d"])
    w, h, d = float(box["width3d"]), float(box["height3d"]), float(box["depth3d"])
    if not (w * h * d >= 1e-6):
        return None
    x, y, z = x3d - w * 0.1, y3d - h * 0.1, z3d - d * 0.1
    w, h, d = w * 1.2, h * 1.2, d * 1.2
    with np.errstate(over="ignore"):   # (beyond float's range: +-inf, as the C cast)
        return (np.array([x, y, z], np.float64).astype(F32), np.array([x + w, y + h, z + d], np.float64).astype(F32))


def crop(pts, box):
    """point indices (ascending) of the flat float32 [n, 3] cloud inside the expanded box"""
    b = crop_bounds(box)
    if b is None:
        return np.zeros(0, np.int64)
    lo, hi = b
    ok = np.all(np.isfinite(pts), axis=1) & np.all(pts >= lo, axis=1) & np.all(pts <= hi, axis=1)
    return np.flatnonzero(ok)


def d2_f32(a, b):
    """float32 ((dx * dx) + (dy * dy)) + (dz * dz) of the rows of a and b"""
    dx, dy, dz = (a[:, k] - b[:, k] for k in range(3))
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def components(p, tol):
    """labels of the epsilon-graph's components over the float32 [n, 3] points p (label = the component's smallest position)"""
    n = len(p)
    tf = F32(tol)
    with np.errstate(over="ignore"):
        r2 = F32(tf * tf)
    if n == 0:
        return np.zeros(0, np.int64)
    if np.isinf(r2):
        return np.zeros(n, np.int64)
    # candidate pairs at a radius safely above every pair with float d2 <= r2 (k-d tree distances are in double)
    rad = float(tf) * (1 + 2.0 ** -10) + 2.0 ** -70
    pairs = cKDTree(p.astype(np.float64)).query_pairs(rad, output_type="ndarray")
    if len(pairs):
        keep = d2_f32(p[pairs[:, 0]], p[pairs[:, 1]]) <= r2
        pairs = pairs[keep]
    g = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    first = np.full(lab.max() + 1, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    return first[lab]


def cluster_record(pts, box, tol):
    """(cropped, nclusters, size, first, centre[3] double, indices) of one record; pts the flat float32 [n, 3] cloud"""
    ci = crop(pts, box)
    nan3 = np.full(3, np.nan)
    if len(ci) == 0:
        return 0, 0, 0, -1, nan3, np.zeros(0, np.int32)
    p = pts[ci]
    lab = components(p, tol)
    roots, sizes = np.unique(lab, return_counts=True)
    best = roots[np.lexsort((roots, -sizes))[0]]    # the largest, ties to the smallest root
    sel = lab == best
    kept = ci[sel]
    centre = p[sel].astype(np.float64).sum(axis=0) / len(kept)
    return len(ci), len(roots), len(kept), int(kept[0]), centre, kept.astype(np.int32)


def cluster_objects(cloud, boxes, tol=0.01):
    """(results as capi.CLUSTER3D_DTYPE, the kept clusters' indices one after the other) for an organized [h, w, 3] cloud"""
    from partsbaseddetector_amd import capi
    pts = np.ascontiguousarray(cloud, F32).reshape(-1, 3)
    out = np.zeros(len(boxes), capi.CLUSTER3D_DTYPE)
    idx = []
    for i, b in enumerate(boxes):
        c, ncl, s, f, cen, ind = cluster_record(pts, b, tol)
        out[i] = (c, ncl, s, f, cen[0], cen[1], cen[2])
        idx.append(ind)
    return out, (np.concatenate(idx) if idx else np.zeros(0, np.int32)).astype(np.int32)
