"""Virtual positives: the positive set of the published recipe (include/pbd_c.h "virtual positives").

The recipe trainmodel.m was written for takes every annotated image as it is, mirrored with the left and right parts swapped
(train.m:130,165), and all of these rotated by a few angles with the keypoints carried along (matlab/learning/map_rotate_points.m).
augment_positives() builds that list: the frames on the GPU (k_augment.hip, one launch per annotated image), the keypoints by the
host definitions of the same header.
"""
from __future__ import annotations

import numpy as np

from . import capi


def _device_route(device, keep_on_device):
    def route(im, specs):
        if isinstance(im, capi.DeviceFrame):
            out = capi.augment_dev(im, specs)
            return out if keep_on_device else [f.numpy() for f in out]
        if not keep_on_device:
            return capi.augment(im, specs, device)
        import torch
        a = np.ascontiguousarray(im, np.uint8)
        return capi.augment_dev(torch.from_numpy(a).to(torch.device("cuda", int(device))), specs)
    return route


def augment_positives(positives, mirror=None, degrees=(), method="bilinear", device=0, keep_on_device=False, _route=None):
    """positives = [(image, points [P, 2])] with the keypoints in the .m files' 1-based pixel coordinates -> the list
    [(image, points)] of the recipe, in a fixed order:
      the originals, first and untouched (the very objects given);
      their mirrors, in the originals' order, when `mirror` is given: a permutation of the parts, mirror[p] the part whose keypoint
        becomes part p's in the mirrored frame (left and right swapped; capi.flip_points);
      then, per angle of `degrees` in the order given, every one of those rotated by it (capi.map_rotate_points), in that order.
    So n positives become n * (1 + (mirror is not None)) * (1 + len(degrees)).  method: "bilinear" or "nearest".  Points are 1-based
    in and out: the definitions work in the 0-based frame, so 1 is subtracted before and added after.  The rotated canvas is
    map_rotate_points.m's, its quirks kept (the extent is rounded up to an even hiB: 640 x 480 becomes 641 x 481 at 0 degrees, a side of
    30 becomes 33; include/pbd_c.h "virtual positives"); the fill is black.
    The frames are computed on HIP device `device`, all virtual copies of one image in one launch.  keep_on_device=True: the virtual
    frames are capi.DeviceFrame objects over torch uint8 tensors and never reach the host — PartsBasedDetector.writeWarped,
    latentPositives and train() take them as they are.  An image that is a capi.DeviceFrame is read in place.
    _route(image, specs) -> frames replaces the device route (capi.augment_host runs without a GPU)."""
    positives = list(positives)
    degrees = [float(d) for d in degrees]
    route = _device_route(device, keep_on_device) if _route is None else _route
    flips = [False] + ([True] if mirror is not None else [])
    specs = [(True, None)] * (len(flips) - 1) + [(f, d, method) for d in degrees for f in flips]
    if not specs:
        return positives
    bases = [list(positives)] + [[] for _ in flips[1:]]          # [flip][i]
    rotated = [[[] for _ in flips] for _ in degrees]             # [angle][flip][i]
    for im, points in positives:
        hgt, w = im.shape[:2]
        p0 = np.asarray(points, np.float64).reshape(-1, 2) - 1.0
        frames = iter(route(im, specs))
        pts = [p0] + ([capi.flip_points(p0, w, mirror)] if mirror is not None else [])
        if mirror is not None:
            bases[1].append((next(frames), pts[1] + 1.0))
        for a, d in enumerate(degrees):
            for f in range(len(flips)):
                rotated[a][f].append((next(frames), capi.map_rotate_points(pts[f], w, hgt, d, capi.PBD_ROT_ORI2NEW) + 1.0))
    out = [it for b in bases for it in b]
    for a in range(len(degrees)):
        for f in range(len(flips)):
            out += rotated[a][f]
    return out
