"""Depth-consistency pruning (pbd_set_depth_filter and the *_rgbd_* entry points, pbd_candidates_depth_filter): the numpy
restatement against a literal transcription of the reference's loop, the C ABI surface and the argument checks that need
no GPU."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np

from partsbaseddetector_amd import capi
from tests import depth_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbd_set_depth_filter", "pbd_detect_rgbd_u8", "pbd_detect_rgbd_enqueue_dev_u8", "pbd_detect_batch_rgbd_u8",
         "pbd_detect_batch_rgbd_enqueue_dev_u8", "pbd_candidates_depth_filter")


def literal(model, heads, boxes, depth, zfactor, T):
    """src/SearchSpacePruning.cpp:73-94 as written: size_t p = nparts-1; p >= 1; --p with break, the p == 1 push, and
    Math::median<T> as sorted(...)[n / 2] (boxes inside the image, no NaN: where the reference is defined)."""
    out = []
    zf = T(np.float32(zfactor))
    for n in range(len(heads)):
        c = int(heads["component"][n])
        nparts = model.nparts(c)
        p = (nparts - 1) % 2**64            # size_t: nparts == 1 -> p = 0, the loop does not run
        while p >= 1 and p < 2**63:
            ax, ay = model.anchors[model.defid[c][p][0]]
            child, parent = boxes[n, p], boxes[n, model.parentid[c][p]]

            def med(b):
                x, y, w, h = (int(v) for v in b)
                v = sorted(depth[y:y + h, x:x + w].ravel().tolist())
                return T(v[len(v) // 2])
            cm, pm = med(child), med(parent)
            if cm > 0 and pm > 0:
                if float(abs(T(cm - pm))) > np.sqrt(float(ax) * ax + float(ay) * ay) * float(zf):
                    break
            if p == 1:
                out.append(n)
            p -= 1
    return out


def fake_model(rng):
    parentid = [[-1], [-1, 0], [-1, 0, 1, 1, 0], [-1, 0, 1, 2, 3, 4, 5]]   # single part, pair, tree, deep chain
    defid, anchors = [], []
    for par in parentid:
        rows = []
        for _ in par:
            k = int(rng.integers(1, 4))
            rows.append(list(range(len(anchors), len(anchors) + k)))
            anchors += [[int(rng.integers(-12, 13)), int(rng.integers(-12, 13))] for _ in range(k)]
        defid.append(rows)
    return SimpleNamespace(parentid=parentid, defid=defid, anchors=np.array(anchors), ncomponents=len(parentid),
                           nparts=lambda c: len(parentid[c]))


def test_restatement_matches_the_reference_loop():
    rng = np.random.default_rng(7)
    model = fake_model(rng)
    for trial in range(24):
        T = np.float32 if trial % 2 == 0 else np.float64
        dh, dw = int(rng.integers(5, 60)), int(rng.integers(5, 60))
        kind = trial % 4
        if kind == 0:
            depth = rng.uniform(0.3, 5.0, (dh, dw))
        elif kind == 1:
            depth = np.round(rng.uniform(0, 4000, (dh, dw))) / 1000.0      # mm / 1000: heavy ties
        elif kind == 2:
            depth = np.full((dh, dw), 1.5)
        else:
            depth = rng.uniform(-1, 3, (dh, dw))
            depth[rng.random((dh, dw)) < 0.3] = 0.0
            depth[rng.random((dh, dw)) < 0.1] = -0.0
        depth = depth.astype(T)
        n = 300
        heads = np.zeros(n, capi.HEAD_DTYPE)
        heads["component"] = rng.integers(0, model.ncomponents, n)
        heads["nparts"] = [model.nparts(c) for c in heads["component"]]
        boxes = np.zeros((n, 7, 4), np.int32)
        boxes[..., 0] = rng.integers(0, dw, (n, 7))
        boxes[..., 1] = rng.integers(0, dh, (n, 7))
        boxes[..., 2] = rng.integers(1, dw + 1, (n, 7))
        boxes[..., 3] = rng.integers(1, dh + 1, (n, 7))
        boxes[..., 2] = np.minimum(boxes[..., 2], dw - boxes[..., 0])   # inside the image: the reference is defined there
        boxes[..., 3] = np.minimum(boxes[..., 3], dh - boxes[..., 1])
        for zf in (-1.0, 0.0, 0.03, 0.3, 1e9):
            want = literal(model, heads, boxes, depth, zf, T)
            got = np.flatnonzero(depth_ref.keep_mask(model, heads, boxes, depth, zf, T)).tolist()
            assert got == want, (trial, zf)


def test_restatement_rules_outside_the_reference():
    model = SimpleNamespace(parentid=[[-1, 0]], defid=[[[0], [0]]], anchors=np.array([[3, 4]]), ncomponents=1,
                            nparts=lambda c: 2)
    heads = np.zeros(1, capi.HEAD_DTYPE)
    depth = np.array([[1.0, 2.0], [np.nan, 9.0]], np.float32)
    # upper median: rank 2 of {1, 2, 9, NaN} with NaN highest = 9
    assert depth_ref.median(depth, (0, 0, 2, 2)) == 9.0
    # clipped: the box's part inside the image; outside / empty: 0
    assert depth_ref.median(depth, (-5, -5, 6, 6)) == 1.0
    assert depth_ref.median(depth, (2, 0, 3, 3)) == 0.0 and depth_ref.median(depth, (0, 0, -1, 2)) == 0.0
    boxes = np.array([[[0, 0, 1, 1], [1, 1, 1, 1]]], np.int32)       # medians 1 and 9, |diff| 8 > 5 * zfactor unless zfactor >= 1.6
    assert not depth_ref.keep_mask(model, heads, boxes, depth, 1.0).any()
    assert depth_ref.keep_mask(model, heads, boxes, depth, 1.6).all()
    boxes = np.array([[[0, 0, 1, 1], [0, 1, 1, 1]]], np.int32)       # NaN median: no test
    assert depth_ref.keep_mask(model, heads, boxes, depth, -1.0).all()


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"\b(pbd_[a-z0-9_]+)\s*\(", hdr))
    tune = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libpbd_hip_tune.so"))
    for name in NAMES:
        assert name in declared
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name) and hasattr(tune, name)
    for m in ("set_depth_filter", "detect_rgbd", "detect_batch_rgbd", "enqueue_rgbd_dev", "enqueue_batch_rgbd_dev",
              "candidates_depth_filter"):
        assert hasattr(capi.Handle, m)
    assert capi.lib().pbd_abi_version() == 5 == capi.PBD_ABI_VERSION


def test_argument_errors_before_any_hip_call():
    L = capi.lib()
    heads = (capi.pbd_candidate_head * 2)()
    boxes = (C.c_int32 * 64)()
    kept = C.c_int(-1)
    for zf in (0.03, float("nan"), float("inf")):
        assert L.pbd_set_depth_filter(None, 1, C.c_float(zf)) == capi.PBD_ERR_ARG
    for dt in (capi.PBD_DEPTH_8U, capi.PBD_DEPTH_16U, capi.PBD_DEPTH_32F, 99):
        assert L.pbd_candidates_depth_filter(None, C.c_float(0.03), None, dt, 0, 0, 0, heads, boxes, None, 2,
                                             C.byref(kept)) == capi.PBD_ERR_ARG
    assert L.pbd_candidates_depth_filter(None, C.c_float(float("nan")), None, capi.PBD_DEPTH_32F, 0, 0, 0, heads, boxes, None, 2,
                                         C.byref(kept)) == capi.PBD_ERR_ARG
    assert L.pbd_candidates_depth_filter(None, C.c_float(0.03), None, capi.PBD_DEPTH_32F, 0, 0, 0, None, None, None, 2,
                                         C.byref(kept)) == capi.PBD_ERR_ARG
    assert kept.value == -1
    assert L.pbd_detect_rgbd_u8(None, None, 4, 4, 3, 12, None, capi.PBD_DEPTH_32F, 16, None, None, None, 0, None) == capi.PBD_ERR_ARG
    assert L.pbd_detect_rgbd_enqueue_dev_u8(None, None, 4, 4, 3, 12, None, capi.PBD_DEPTH_32F, 16) == capi.PBD_ERR_ARG
    assert L.pbd_detect_batch_rgbd_u8(None, None, None, 1, 4, 4, 3, 12, capi.PBD_DEPTH_32F, 16, None, None, None, 0, None) == capi.PBD_ERR_ARG
    assert L.pbd_detect_batch_rgbd_enqueue_dev_u8(None, None, None, 1, 4, 4, 3, capi.PBD_DEPTH_32F) == capi.PBD_ERR_ARG


def test_detector_exposes_the_setting():
    from partsbaseddetector_amd import PartsBasedDetector
    det = PartsBasedDetector()
    assert det._zfactor is None
    det.setDepthFilter(0.05)             # before distributeModel: remembered for the handle
    assert det._zfactor == 0.05
    det.setDepthFilter(None)
    assert det._zfactor is None
    host = open(os.path.join(ROOT, "partsbaseddetector_amd", "host", "pbd_host.hpp")).read()
    assert "void setDepthFilter(bool on, float zfactor" in host
    assert "void filterCandidatesByDepth(Parts& parts, vectorCandidate& candidates, const Mat& depth, const float zfactor)" in host
