"""matlab/learning/train.m, trainmodel.m and pointtobox.m on a live detector.

train() is one call for what train.m:73-121 does around the entry points of include/pbd_c.h: clear the example cache, write the
positives (warped or latent), solve, mine the negatives at interval 2, solve again, take the threshold from the positives' scores.
Every step runs on the GPU through PartsBasedDetector and capi.QpCache; no per-example data crosses PCIe.  train_model() is
trainmodel.m on top of it: boxes from keypoints, part mixtures by k-means, one warped training per (part, mixture), the joint model,
and two latent rounds.
"""
from __future__ import annotations

import numpy as np

from . import capi
from .augment import augment_positives
from .detector import PartsBasedDetector
from .model import Model, build_model, data_def, init_model, merge_models

_SETTERS = ("pyramid_kind", "boundary_pad")   # handle_options that are setters of PartsBasedDetector, not constructor arguments


def _new_detector(model, dtype, handle_options):
    opts = dict(handle_options)
    kind, pad = opts.pop("pyramid_kind", None), opts.pop("boundary_pad", None)
    det = PartsBasedDetector(dtype=dtype, **opts)
    if kind is not None:
        det.setPyramidKind(kind)
    if pad is not None:
        det.setBoundaryPad(pad)
    det.distributeModel(model)
    return det


def train(model, positives, negatives, warp, iter=1, C=0.002, wpos=2, overlap=0.6, capacity=None, tol=.05, max_iter=1000, seed=0,
          dtype=np.float32, detector=None, cache=None, **handle_options):
    """matlab/learning/train.m: `iter` rounds of a structured SVM with latent positives -> (model, report).

    model      the Model to start from (its interval, sbin and structure are kept; weights and threshold are trained).
    positives  an item's image is an 8-bit array or a capi.DeviceFrame (a frame in device memory, as augment_positives(...,
               keep_on_device=True) returns them), read in place with the array's results in bits.
               warp > 0: items (image, box) with box = (x1, y1, x2, y2), 1-based inclusive, of component 0's root (train.m's poswarp;
               boxes below prod(maxsize * sbin) are skipped inside writeWarped).  warp == 0: items (image, truth[, mix]) with
               truth [nparts, 4] rows (x, y, width, height) as detect() returns boxes, and the optional mixture label per part
               (trainmodel.m:48-50), as PartsBasedDetector.latentPositives takes them (its skip, croppos and ids are in place).
    negatives  8-bit images without the object; an item may be a capi.StoredFrame (a slot of a pyramid store whose signature is the
               detector's at interval 2): it is mined from the slot, with the image's results in bits.
    C, wpos    cpos = C * wpos, cneg = C (train.m:69-70).  overlap: the minimum overlap of a latent positive's parts.
    capacity   examples the cache holds; default 10 * (wpos + 1) * len(positives) (train.m:30-31,46).
    tol, max_iter, seed   of every qp_opt (capi.QpCache.opt) and of the solver steps inside mining.
    dtype, handle_options   the detector's scalar type and PartsBasedDetector's constructor arguments; pyramid_kind= and
               boundary_pad= go to its setters.
    detector, cache   run on a detector that exists (model may then be None: the detector's is taken) and / or on a cache bound to
               it, instead of creating them; they are left open, so their state can be looked at afterwards.

    One round, in train.m's order (:73-121):
      cache.clear()                                                        :75   qp.n = 0
      writeWarped per positive with id i + 1 / latentPositives(overlap)    :76-80
      fix(n), prune(), opt(tol, max_iter, seed), apply_weights()           :90-94
      interval0 = interval; setInterval(2); setThresh(-1)                  :95-96,102
      mineNegatives(negatives, first_id=1): ids as train.m:102 gives them; stops behind the image after which sum(sv) == capacity (:105)
      opt(...), apply_weights()                                            :111-112
      thresh, _ = cache.positive_threshold(.05); setThresh(float32(thresh)) :116-118
      setInterval(interval0)                                               :121
    If anything from the interval change on raises, the interval is restored and the threshold set back to what it was before the
    exception goes on.  The returned model is detector.model: the one given, with the weights and the threshold set since.

    report: one dict per round — numpositives (per component; warped: [n]), n and sv (three counts each: after the positives, after
    mining, after the last solve), lb, ub (the last solve's bounds), thresh (as set: float32), mined (per frame mined its (records,
    written, action)), passes (the first and the last solve's pbd_qp_one calls).

    Deviations from train.m, each stated: the default capacity has no 6 GB floor (train.m:32: the MATLAB cache is sized for a
    workstation's memory, this one for its positives); clear() also resets the solver's a, sv and bounds, where train.m:75 leaves
    stale ones behind for rounds after the first (trainmodel.m only ever runs one); and those mineNegatives states — the model is
    constant over a frame (detect.m updates it between levels), the levels and components are visited in a fixed, not a random,
    order, and the solver's shuffles are seeded."""
    own_det = detector is None
    det = _new_detector(model, dtype, handle_options) if own_det else detector
    own_cache = cache is None
    try:
        _, wreg, w0, noneg = det.model.qp_vectors()
        if own_cache:
            cap = int(capacity) if capacity is not None else int(10 * (wpos + 1) * len(positives))
            cache = capi.QpCache(det.handle, cap, C * wpos, C, wreg, w0)
        cache.noneg(noneg)
        report = []
        for _t in range(int(iter)):
            rep = dict(n=[], sv=[], passes=[], mined=[])
            cache.clear()
            if warp > 0:
                for i, item in enumerate(positives):
                    det.writeWarped(item[0], [item[1]], cache, ids=[i + 1])
                rep["numpositives"] = [int(cache.dims()[3])]
            else:
                counts, _ = det.latentPositives(positives, cache, overlap)
                rep["numpositives"] = [int(c) for c in counts]
            _count(cache, rep)
            cache.fix(rep["n"][0])
            cache.prune()
            rep["passes"].append(cache.opt(tol, max_iter, seed)[2])
            cache.apply_weights()
            interval0, thresh0 = det.interval, det.model.thresh
            done = False
            try:
                det.setInterval(2)
                det.setThresh(-1)
                rep["mined"] = [tuple(int(v) for v in m) for m in det.mineNegatives(negatives, cache, 1, tol, max_iter, seed)]
                _count(cache, rep)
                lb, ub, passes = cache.opt(tol, max_iter, seed)
                cache.apply_weights()
                rep["passes"].append(passes)
                _count(cache, rep)
                thresh, _ = cache.positive_threshold(.05)
                det.setThresh(float(np.float32(thresh)))
                rep.update(lb=lb, ub=ub, thresh=float(np.float32(thresh)))
                done = True
            finally:
                if not done:
                    det.setThresh(thresh0)
                det.setInterval(interval0)
            report.append(rep)
        return det.model, report
    finally:
        if own_cache and cache is not None:
            cache.close()
        if own_det:
            det.handle.close()


def _count(cache, rep):
    rep["n"].append(int(cache.dims()[3]))
    rep["sv"].append(int(np.asarray(cache.support()).sum()))


def point_to_box(points, parents):
    """matlab/learning/pointtobox.m: square part boxes around keypoints.  points [n, P, 2] (x, y) of part p in positive i; parents
    0-based with -1 at part 0.  -> boxes [n, P, 4] float64 rows (x1, y1, x2, y2) = point -+ boxsize_i / 2.
    Per non-root part the limb length to its parent, sqrt(dx * dx + dy * dy); r_j = exp(median_i(log len[i, j] - log len[i, 0])), the
    limbs' typical ratio to limb 1; boxsize_i = the 0.85 quantile of len[i, :] / r — quantile(x, 0.85, 1, 7), the linear rule that
    numpy's default implements."""
    pts = np.asarray(points, np.float64)
    if pts.ndim != 3 or pts.shape[2] != 2 or pts.shape[1] < 2 or len(parents) != pts.shape[1]:
        raise ValueError("point_to_box: points [n, P, 2] with P >= 2, one parent per part")
    n, P = pts.shape[:2]
    length = np.zeros((n, P - 1), np.float64)
    for p in range(1, P):
        d = np.abs(pts[:, p] - pts[:, int(parents[p])])
        length[:, p - 1] = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    r = np.zeros(P - 1, np.float64)
    for i in range(P - 1):
        r[i] = np.exp(np.median(np.log(length[:, i]) - np.log(length[:, 0])))
    boxsize = np.array([np.quantile(length[i] / r, 0.85) for i in range(n)], np.float64)
    half = (boxsize / 2)[:, None]
    return np.stack([pts[:, :, 0] - half, pts[:, :, 1] - half, pts[:, :, 0] + half, pts[:, :, 1] + half], axis=2)


def _truth(box):
    """(x1, y1, x2, y2) rows, 1-based inclusive and fractional, as the latent entries' integer truth (x, y, width, height), 0-based,
    covering x .. x + width: the corners rounded half away from zero as MATLAB rounds, then x = x1 - 1, width = x2 - x1."""
    b = np.asarray(box, np.float64).reshape(-1, 4)
    c = np.copysign(np.floor(np.abs(b) + .5), b)
    return np.stack([c[:, 0] - 1, c[:, 1] - 1, c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]], axis=1).astype(np.int32)


_TRAIN_ARGS = ("iter", "C", "wpos", "overlap", "capacity", "tol", "max_iter", "seed", "dtype", "detector", "cache")   # train()'s own; the rest are the detector's


def _share_negatives(model, negatives, train_options, make):
    """train_model(share_pyramids=True): a producer detector on `model` at interval 2 (train.m:96: what every round mines at), with the
    trainings' dtype, pyramid kind, boundary pad and device, and a pyramid store that holds every negative's pyramid, put once
    -> (producer, store, [capi.StoredFrame per negative])"""
    opts = {k: v for k, v in train_options.items() if k not in _TRAIN_ARGS}
    det = make(model, train_options.get("dtype", np.float32), opts)
    store = None
    try:
        det.setInterval(2)
        shapes = [np.asarray(im).shape for im in negatives]
        store = det.pyramidStore(max(len(negatives), 1), max([s[1] for s in shapes] + [1]), max([s[0] for s in shapes] + [1]))
        return det, store, [store.put(i, im) for i, im in enumerate(negatives)]
    except BaseException:
        if store is not None:
            store.close()
        det.handle.close()
        raise


def _root_sizes(positives, parents):
    """(w, h) of the root boxes point_to_box gives the positives: init_model's first two arguments"""
    P = len(parents)
    points = np.stack([np.asarray(it[1], np.float64).reshape(P, 2) for it in positives])
    boxes = point_to_box(points, [int(v) for v in parents])
    return boxes[:, 0, 2] - boxes[:, 0, 0] + 1, boxes[:, 0, 3] - boxes[:, 0, 1] + 1


def train_model(positives, negatives, K, parents, sbin, tsize=None, R=100, cluster_seed=0, cluster_max_iter=1000, device=0,
                share_pyramids=False, _train=None, _cluster=None, _producer=None, mirror=None, degrees=(), augment_method="bilinear",
                _augment=None, **train_options):
    """matlab/learning/trainmodel.m -> (model, reports).  positives = [(image, points [P, 2])] with the keypoints in the .m files'
    1-based pixel coordinates; negatives 8-bit images; K the mixtures per part (an int or one per part); parents 0-based with -1 at
    part 0 and parent < child; sbin the HOG cell size.  tsize = (rows, cols) overrides init_model's 5th-percentile template (needed
    below 20 positives).  train_options go to every train() call (C, wpos, overlap, tol, max_iter, seed, dtype and the detector's).
      boxes = point_to_box(points, parents)                                                 trainmodel.m reads pos.x1 .. y2 from it
      init = init_model(w, h, sbin, tsize); def = data_def(...); idx = capi.cluster_parts(def, parents, K, R)          :13-15
      per part p, per mixture k: train(init, the positives with idx[p] == k reduced to part p's box, negatives[:100], warp=1);
        merge_models of the part's K results                                                                           :19-40
      joint = build_model(part models, def, idx, parents)                                                              :46
      train(joint, positives with mix = idx[:, i], negatives, warp=0), then train(that, positives without mix, negatives, warp=0)  :47-63
    reports: dict(parts={(p, k): report}, final1=report, final=report, idx=idx).  Nothing is cached on disk and no .mat file is read
    or written: the caller saves the Model with the writers it has.  The latent rounds take integer truth boxes (the ABI's): the
    fractional corners are rounded half away from zero.
    share_pyramids=True: the sum(K) + 2 trainings mine the same negatives at interval 2, and a mining frame's pyramid does not depend
    on the model: one producer detector (init_model's model, interval 2, the trainings' dtype, pyramid_kind, boundary_pad and device)
    puts every negative ONCE into a pyramid store sized for the largest, and every train() receives capi.StoredFrame items instead
    of the images — mineNegatives mines them from their slots with the images' results in bits.  The store and the
    producer are closed on the way out, whatever happens.  The default stays False.
    mirror= (a permutation of the parts: the left / right swap) and / or degrees= (angles): the positives are augmented first, on the
    device — augment.augment_positives(positives, mirror, degrees, augment_method, device, keep_on_device=True): the originals, their
    mirrors, and every one of those rotated by every angle, the virtual frames staying in device memory as capi.DeviceFrame items —,
    and everything above runs over the longer list: the clusters are computed over the augmented keypoints, as the recipe does
    (DESIGN.md 5.28).  With the defaults not one call changes."""
    run = train if _train is None else _train
    if mirror is not None or len(degrees):
        aug = augment_positives if _augment is None else _augment
        positives = aug(positives, mirror=mirror, degrees=degrees, method=augment_method, device=device, keep_on_device=True)
    if share_pyramids:
        negatives = list(negatives)
        producer, store, stored = _share_negatives(init_model(*_root_sizes(positives, parents), sbin, tsize), negatives, train_options,
                                                   _new_detector if _producer is None else _producer)
        try:
            return train_model(positives, stored, K, parents, sbin, tsize, R, cluster_seed, cluster_max_iter, device, False, _train, _cluster,
                               None, **train_options)
        finally:
            store.close()
            producer.handle.close()
    cluster = (lambda d, pa, k: capi.cluster_parts(d, pa, k, R, cluster_seed, cluster_max_iter, device)) if _cluster is None else _cluster
    parents = [int(v) for v in parents]
    P = len(parents)
    images = [it[0] for it in positives]
    points = np.stack([np.asarray(it[1], np.float64).reshape(P, 2) for it in positives])
    boxes = point_to_box(points, parents)
    w, h = boxes[:, 0, 2] - boxes[:, 0, 0] + 1, boxes[:, 0, 3] - boxes[:, 0, 1] + 1
    init = init_model(w, h, sbin, tsize)
    deffeat = data_def(points, w, h, init.filter_sizes()[0])
    Ks = [int(v) for v in np.broadcast_to(np.asarray(K), (P,))]
    idx = np.asarray(cluster(deffeat, parents, Ks)["idx"])
    reports = dict(parts={}, idx=idx)
    sneg = list(negatives)[:100]
    part_models = []
    for p in range(P):
        models = []
        for k in range(Ks[p]):
            spos = [(images[i], boxes[i, p].copy()) for i in range(len(images)) if idx[p][i] == k]
            m, rep = run(init_model(w, h, sbin, tsize), spos, sneg, 1, **train_options)
            models.append(m)
            reports["parts"][(p, k)] = rep
        part_models.append(merge_models(models))
    joint = build_model(part_models, deffeat, idx, parents)
    truths = [_truth(boxes[i]) for i in range(len(images))]
    model, reports["final1"] = run(joint, [(images[i], truths[i], [int(idx[p][i]) for p in range(P)]) for i in range(len(images))],
                                   list(negatives), 0, **train_options)
    model, reports["final"] = run(model, [(images[i], truths[i]) for i in range(len(images))], list(negatives), 0, **train_options)
    return model, reports
