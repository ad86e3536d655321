"""Host-side mirror of the reference's detector interfaces over the C ABI.

Same names, call order and argument meaning as the reference so that callers
(and the parity tests) read like code written against it:

    reference (C++)                                   here
    ------------------------------------------------  --------------------------------
    PartsBasedDetector<T>::distributeModel(Model&)    PartsBasedDetector.distributeModel(model)
    PartsBasedDetector<T>::detect(im, candidates)     PartsBasedDetector.detect(im) -> [Candidate]
    IFeatures::{binsize,nscales,scales,pyramid}       HOGFeatures.*
    IConvolutionEngine::{setFilters,pdf}              SpatialConvolutionEngine.*
    DynamicProgram<T>::{min,argmin}                   DynamicProgram.*
    Candidate::{sort,nonMaximaSuppression}            Candidate.*

(src/PartsBasedDetector.cpp:69-127, include/IFeatures.hpp:49-73,
include/IConvolutionEngine.hpp:44-68, include/DynamicProgram.hpp:61-77,
include/Candidate.hpp:56-111,277-304.)  All numerics run in libpbd_hip.so.
The three stage objects share one device handle: features, responses and DP
tables stay resident in HBM between the calls, exactly like the fused detect().
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import capi
from .model import Model


@dataclass
class Candidate:
    """include/Candidate.hpp:56-111: part boxes (x, y, w, h), part confidences, component."""

    parts: np.ndarray        # [nparts, 4] cv::Rect per part
    confidence: np.ndarray   # [nparts]; root = score, others 0 (src/DynamicProgram.cpp:241-244)
    component: int
    level: int = -1
    locs: Optional[np.ndarray] = None  # [nparts, 3] (x, y, mixture) in cells of `level`
    box3d: Optional[np.ndarray] = None          # setBoundingBoxes3D: this record's pbd_box3d (capi.BOX3D_DTYPE)
    part_centers: Optional[np.ndarray] = None   # setBoundingBoxes3D: [nparts, 3] (empty when the box was skipped)
    centre3d: Optional[np.ndarray] = None       # setObjectClusters: the kept cluster's centroid (3 doubles, NaN when none)
    cluster: Optional[np.ndarray] = None        # setObjectClusters: its point indices (row * w + col), ascending, int32
    part_scores: Optional[np.ndarray] = None    # setPartScores: [nparts, 3] float64 (app, def, bias) of every part

    def partScores(self) -> Optional[np.ndarray]:
        """The three terms of every part's score, score_p = app + def + bias ([nparts, 3] float64); None with setPartScores off."""
        return self.part_scores

    def score(self) -> float:
        return float(self.confidence[0]) if len(self.confidence) else float("-inf")

    def setScore(self, confidence: float) -> None:
        """Candidate::setScore (:76)."""
        if len(self.confidence) == 0:
            self.confidence = np.zeros(1, np.float32)
        self.confidence[0] = np.float32(confidence)

    def resize(self, factor: float) -> None:
        """Candidate::resize (:82-89): `int *= float` — float product truncated toward zero, per field."""
        f = np.float32(factor)
        self.parts = np.trunc(self.parts.astype(np.float32) * f).astype(self.parts.dtype)

    def boundingBox(self):
        x, y, w, h = [int(v) for v in self.parts[0]]
        for q in self.parts:
            x1, y1 = min(x, int(q[0])), min(y, int(q[1]))
            w = max(x + w, int(q[0] + q[2])) - x1
            h = max(y + h, int(q[1] + q[3])) - y1
            x, y = x1, y1
        return x, y, w, h

    def boundingBoxNorm(self):
        """Candidate::boundingBoxNorm (:117-130): cvRound centroids (half to even), cv::meanStdDev (sums times 1. / n), Rect of
        doubles truncated toward zero"""
        p = np.asarray(self.parts, np.int64)
        out = []
        for c in (np.rint((2 * p[:, 0] + p[:, 2]) * 0.5), np.rint((2 * p[:, 1] + p[:, 3]) * 0.5)):
            sc = 1.0 / len(c)
            m = float(np.sum(c)) * sc
            out.append((m, float(np.sqrt(max(float(np.sum(c * c)) * sc - m * m, 0.0)))))
        (mx, sx), (my, sy) = out
        return int(mx - 1.5 * sx), int(my - 1.5 * sy), int(3 * sx), int(3 * sy)

    @staticmethod
    def _pack(cands: List["Candidate"]):
        mp = max((len(c.parts) for c in cands), default=1)
        heads = np.zeros(len(cands), capi.HEAD_DTYPE)
        boxes = np.zeros((len(cands), mp, 4), np.int32)
        locs = np.zeros((len(cands), mp, 3), np.int32)
        for i, c in enumerate(cands):
            heads[i] = (c.score(), c.component, c.level, len(c.parts))
            boxes[i, : len(c.parts)] = c.parts
            if c.locs is not None:
                locs[i, : len(c.parts)] = c.locs
        return heads, boxes, locs

    @staticmethod
    def _unpack(heads, boxes, locs, part_scores=None) -> List["Candidate"]:
        """part_scores ([n, max_parts, 3], setPartScores): confidence[p] = (float)score_p for p >= 1; confidence[0] stays the
        root score, which callers sort and suppress by"""
        out = []
        for i in range(len(heads)):
            n = int(heads[i]["nparts"])
            conf = np.zeros(n, np.float32)
            ps = None
            if part_scores is not None:
                ps = np.asarray(part_scores[i][:n], np.float64).copy()
                conf[:] = ((ps[:, 0] + ps[:, 1]) + ps[:, 2]).astype(np.float32)
            conf[0] = heads[i]["score"]
            out.append(Candidate(boxes[i, :n].copy(), conf, int(heads[i]["component"]), int(heads[i]["level"]),
                                 locs[i, :n].copy(), part_scores=ps))
        return out

    @staticmethod
    def sort(candidates: List["Candidate"]) -> List["Candidate"]:
        """Candidate::sort — descending root score."""
        return Candidate._unpack(*capi.candidates_sort(*Candidate._pack(candidates)))

    @staticmethod
    def nonMaximaSuppression(im_shape, candidates: List["Candidate"], overlap: float = 0.0) -> List["Candidate"]:
        """Candidate::nonMaximaSuppression(im, candidates, overlap)."""
        h, w = im_shape[:2]
        return Candidate._unpack(*capi.candidates_nms(*Candidate._pack(candidates), w, h, overlap))

    @staticmethod
    def nonMaximaSuppressionParts(candidates: List["Candidate"], overlap: float = 0.3, top: int = 1000) -> List["Candidate"]:
        """matlab/detection/nms.m on sorted candidates: part by part and by the covering box, over the kept detection's area,
        after a cut to the `top` best (0: none)."""
        return Candidate._unpack(*capi.candidates_nms_parts(*Candidate._pack(candidates), overlap, top))

    @staticmethod
    def bestOverlap(candidates: List["Candidate"], gt, overlap: float = 0.3):
        """matlab/detection/bestoverlap.m per gt box (x1, y1, x2, y2): (index of the highest-scoring candidate whose box of part
        centres covers more than `overlap` of the box, or -1; its overlap) — the first of equal scores."""
        heads, boxes, _ = Candidate._pack(candidates)
        return capi.candidates_best_overlap(heads, boxes, gt, overlap)


class HOGFeatures:
    """IFeatures implementation (include/HOGFeatures.hpp:52-88) on the device."""

    def __init__(self, handle: capi.Handle):
        self._h = handle
        self._scales = np.zeros(0, np.float32)
        self._nscales = handle.model.interval

    def binsize(self) -> int:
        return self._h.model.sbin

    def nscales(self) -> int:
        return self._nscales

    def scales(self) -> np.ndarray:
        return self._scales

    def pyramid(self, im: np.ndarray) -> List[np.ndarray]:
        """HOGFeatures<T>::pyramid: returns the feature pyramid (fine to coarse),
        each level H x (W*flen) like the reference's cv::Mat; it also stays resident.  The image's dtype is its depth (:136-146:
        uint8, uint16, float32, float64; anything else raises like CV_Error(StsUnsupportedFormat))."""
        if np.asarray(im).dtype == np.uint8:
            self._h.pyramid(im)
        elif np.asarray(im).dtype in capi.DEPTH_OF:
            self._h.pyramid_image(im)
        else:
            raise capi.PbdError(capi.PBD_ERR_UNSUPPORTED, "Unsupported image type")
        g = self._h._geo
        self._nscales, self._scales = g["nlevels"], g["scales"]
        return [self._h.level_features(l).reshape(g["cell_h"][l], -1) for l in range(g["nlevels"])]


class SpatialConvolutionEngine:
    """IConvolutionEngine implementation (include/SpatialConvolutionEngine.hpp:44-58)."""

    def __init__(self, handle: capi.Handle):
        self._h = handle

    def setFilters(self, filters) -> None:
        """Filters are uploaded (transposed for the kernels) at distributeModel time;
        like the reference this must precede pdf()."""
        if len(filters) != len(self._h.model.filtersw):
            raise ValueError("setFilters: filter bank differs from the distributed model")

    def pdf(self, features: Optional[List[np.ndarray]] = None) -> List[List[np.ndarray]]:
        """pdf(features, responses): responses[level][filter].  `features=None`
        uses the pyramid already resident on the device."""
        g = self._h._geo
        if features is not None:
            for l, f in enumerate(features):
                # the handle's T (float or double): a double detector must not round injected features to float
                self._h.set_level_features(l, np.asarray(f, self._h.dtype).reshape(g["cell_h"][l], g["cell_w"][l], 32))
        self._h.pdf()
        nf = len(self._h.model.filtersw)
        return [[self._h.level_response(l, n) for n in range(nf)] for l in range(g["nlevels"])]


class DynamicProgram:
    """DynamicProgram<T> (include/DynamicProgram.hpp:61-77)."""

    def __init__(self, handle: capi.Handle):
        self._h = handle

    def min(self, scores: Optional[List[List[np.ndarray]]] = None):
        """min(parts, scores, Ix, Iy, Ik, rootv, rooti): returns (Ix, Iy, Ik, rootv, rooti)
        indexed [level][component][part][parent mixture] / [level][component]."""
        h, g, m = self._h, self._h._geo, self._h.model
        if scores is not None:
            for l in range(g["nlevels"]):
                for n, r in enumerate(scores[l]):
                    h.set_level_response(l, n, r)
        h.dp_min()
        Ix, Iy, Ik, rootv, rooti = [], [], [], [], []
        for l in range(g["nlevels"]):
            lx, ly, lk, rv, ri = [], [], [], [], []
            for c in range(m.ncomponents):
                cx, cy, ck = [[]], [[]], [[]]
                for p in range(1, m.nparts(c)):
                    L = len(m.filterid[c][m.parentid[c][p]])
                    trip = [h.dp_pointers(l, c, p, pm) for pm in range(L)]
                    cx.append([t[0] for t in trip]); cy.append([t[1] for t in trip]); ck.append([t[2] for t in trip])
                lx.append(cx); ly.append(cy); lk.append(ck)
                a, b = h.root(l, c)
                rv.append(a); ri.append(b)
            Ix.append(lx); Iy.append(ly); Ik.append(lk); rootv.append(rv); rooti.append(ri)
        return Ix, Iy, Ik, rootv, rooti

    def argmin(self, rootv=None, rooti=None, Ix=None, Iy=None, Ik=None, capacity=4096) -> List[Candidate]:
        """argmin(parts, rootv, rooti, scales, Ix, Iy, Ik, candidates).  With no arguments it walks the tables min() left
        on the device; tables passed in (another engine's, or edited ones) are uploaded first and honoured."""
        h, g, m = self._h, self._h._geo, self._h.model
        if rootv is not None:
            for l in range(g["nlevels"]):
                for c in range(m.ncomponents):
                    h.set_root(l, c, rootv[l][c], rooti[l][c])
        if Ix is not None:
            for l in range(g["nlevels"]):
                for c in range(m.ncomponents):
                    for p in range(1, m.nparts(c)):
                        for pm in range(len(Ix[l][c][p])):
                            h.set_dp_pointers(l, c, p, pm, Ix[l][c][p][pm], Iy[l][c][p][pm], Ik[l][c][p][pm])
        return Candidate._unpack(*h.dp_argmin(capacity))

    def latentMask(self, truth, overlap: float, mix=None, component: int = -1) -> np.ndarray:
        """Between pdf() and min(): the response planes resident on the device masked by one box per part (capi.Handle.latent_mask);
        returns admissible [level][component]."""
        return self._h.latent_mask(truth, overlap, mix, component)

    def argbest(self) -> List[Candidate]:
        """After min(): the best root over the remaining (level, component) pairs, back-tracked like argmin; one Candidate or none."""
        return Candidate._unpack(*self._h.dp_argbest())


class PartsBasedDetector:
    """PartsBasedDetector<T> (include/PartsBasedDetector.hpp:152-175); dtype = np.float32 (src/demo.cpp:85)
    or np.float64 (ros/Node.hpp:121, cells/detect.cpp:93) picks the instantiation."""

    def __init__(self, device: int = 0, conv_mode: int = capi.PBD_CONV_AUTO, max_candidates: int = 4096,
                 level_begin: int = 0, level_end: int = 0, dtype=np.float32, cand_filter=None, cand_nms=None):
        """cand_filter=(mode, overlap): see setCandidateFilter; cand_nms=(kind, top): see setCandidateNms."""
        self._device, self._conv, self._cap = device, conv_mode, max_candidates
        self._cand_filter = cand_filter
        self._cand_nms = cand_nms
        self._zfactor: Optional[float] = None   # setDepthFilter: None = off
        self._camera = None                      # setBoundingBoxes3D: None = off
        self._cluster_tol: Optional[float] = None   # setObjectClusters: None = off
        self._part_scores = False                # setPartScores
        self._boundary_pad = 0                   # setBoundaryPad
        self._pyramid_kind = "opencv"            # setPyramidKind
        self._dtype = np.dtype(dtype)
        self._lb, self._le = level_begin, level_end
        self._h: Optional[capi.Handle] = None
        self._name = ""
        self.features_ = self.convolution_engine_ = self.dp_ = None

    def name(self) -> str:
        return self._name

    def distributeModel(self, model: Model) -> None:
        """src/PartsBasedDetector.cpp:102-127."""
        self._name = model.name
        self._h = capi.Handle(model, self._device, self._conv, self._cap, 0, self._lb, self._le, dtype=self._dtype,
                              cand_filter=self._cand_filter, cand_nms=self._cand_nms)
        self.features_ = HOGFeatures(self._h)
        self.convolution_engine_ = SpatialConvolutionEngine(self._h)
        self.convolution_engine_.setFilters(model.filtersw)
        self.dp_ = DynamicProgram(self._h)
        if self._zfactor is not None:
            self._h.set_depth_filter(True, self._zfactor)
        if self._camera is not None:
            self._h.set_box3d(True, self._camera)
        if self._cluster_tol is not None:
            self._h.set_cluster3d(True, self._cluster_tol)
        if self._part_scores:
            self._h.set_part_scores(True)
        if self._boundary_pad:
            self._h.set_boundary_pad(self._boundary_pad)
        if self._pyramid_kind != "opencv":
            self._h.set_pyramid_kind(self._PYRAMID_KINDS[self._pyramid_kind])

    _PYRAMID_KINDS = {"opencv": capi.PBD_PYRAMID_OPENCV, "matlab": capi.PBD_PYRAMID_MATLAB}

    @property
    def pyramid_kind(self) -> str:
        """"opencv" or "matlab" (setPyramidKind)"""
        return self._pyramid_kind

    def setPyramidKind(self, kind: str = "matlab") -> None:
        """The image pyramid under the features.  "opencv" (the default): HOGFeatures<T>::pyramid, cv::resize and cv::pyrDown in the
        pixel type (src/HOGFeatures.cpp:95-127).  "matlab": matlab/detection/featpyramid.m:13-34 — the frame goes to double once,
        matlab/mex/resize.cc makes the first octave, matlab/mex/reduce.cc every further one, nothing is rounded back to 8 bits —
        with its level count, level sizes and box scales: the levels the MATLAB pipeline trains and evaluates its models on.
        8-bit frames only.  With setBoundaryPad the two together are featpyramid.m.  Kept across distributeModel()."""
        if kind not in self._PYRAMID_KINDS:
            raise ValueError('setPyramidKind: "opencv" or "matlab"')
        if self._h is not None:
            self._h.set_pyramid_kind(self._PYRAMID_KINDS[kind])
        self._pyramid_kind = kind

    @property
    def boundary_pad(self) -> int:
        """cells of boundary padding around every pyramid level (setBoundaryPad); 0 = off"""
        return self._boundary_pad

    def setBoundaryPad(self, pad: int = 3) -> None:
        """The step src/HOGFeatures.cpp:147-148 leaves commented out: every pyramid level surrounded by `pad` cells that hold 0 and,
        in the last channel, 1 — the value the models' last channel is trained on for cells outside the image
        (matlab/detection/featpyramid.m:37-44) — so that a detection may reach over the frame border.  Boxes are shifted back by the
        padding (matlab/detection/detect.m:266-267); feature / response planes and part locations are those of the padded levels.
        0 = off (the default), 3 = the reference's literal, at most 8.  Kept across distributeModel()."""
        pad = int(pad)
        if not 0 <= pad <= 8:
            raise ValueError("setBoundaryPad: 0 (off) .. 8 cells")
        if self._h is not None:
            self._h.set_boundary_pad(pad)
        self._boundary_pad = pad

    def setPartScores(self, on: bool = True) -> None:
        """Every detect() fills Candidate.confidence[p], p >= 1, with the part's own score (appearance + deformation + bias of
        the returned configuration, computed on the GPU) instead of the reference's 0.0, and Candidate.partScores() with the three
        terms; confidence[0] stays the root score.  Off (the default): zeros, as the reference.  Kept across distributeModel()."""
        if self._h is not None:
            self._h.set_part_scores(on)
        self._part_scores = bool(on)

    def _ps(self):
        return self.handle.part_scores(0) if self._part_scores else None

    @property
    def model(self) -> Model:
        """the model the detector runs now: distributeModel's, with the weights and the threshold set since"""
        return self.handle.model

    def setWeights(self, w) -> None:
        """matlab/learning/vec2model.m on the live detector: its biases, deformations and filters become `w`'s elements (in
        Model.feature_layout()'s order, rounded to float32) — a numpy vector or a float64 torch tensor on the detector's device.  Every
        setter's state is kept, and so is an ExampleCache bound to this detector; self.model.weight_vector() agrees with the device."""
        self.handle.set_weights(w)

    def setThresh(self, t: float) -> None:
        """The model's threshold for every detect from now on (train.m: 0 for latent positives, -1 for mining, then
        Model.positive_threshold of the positives' scores)."""
        self.handle.set_threshold(t)

    def setInterval(self, interval: int) -> None:
        """train.m:95-96,121 model.interval = 2 on the live detector: the pyramid's levels per octave from the next frame on (1..16).
        The detector then behaves like one given the same model with that interval; an ExampleCache bound to it stays valid."""
        self.handle.set_interval(interval)

    @property
    def interval(self) -> int:
        """the interval the detector runs now"""
        return self.handle.interval

    def updateFrom(self, cache: "capi.QpCache") -> None:
        """train.m:94,112 model = vec2model(qp_w, model): the solver's weights into this detector, without leaving the device"""
        if cache.handle is not self.handle:
            raise ValueError("updateFrom: the cache is bound to another detector")
        cache.apply_weights()

    def setBoundingBoxes3D(self, camera=None) -> None:
        """camera = (fx, fy, cx, cy[, tx, ty]) or a capi.pbd_camera: every detect(im, depth) with a non-empty depth image attaches
        to each returned Candidate its `box3d` (Candidate::boundingBox3D projected as PointCloudClusterer::computeBoundingBoxes
        does, capi.BOX3D_DTYPE) and `part_centers`, computed on the GPU; None turns it off (the default).  Kept across
        distributeModel()."""
        cam = None if camera is None else capi.camera(camera)
        if self._h is not None:
            self._h.set_box3d(cam is not None, cam)
        self._camera = cam

    def setObjectClusters(self, tolerance: Optional[float] = 0.01) -> None:
        """With setBoundingBoxes3D on, every detect(im, depth) with a non-empty depth image also attaches to each returned Candidate
        the object PointCloudClusterer::clusterObjects keeps for its box: `centre3d` (the largest Euclidean cluster's centroid,
        NaN when none) and `cluster` (its point indices in the frame's cloud), computed on the GPU from the depth image through
        the camera (pbd_c.h states the cloud rule).  None turns it off (the default).  Kept across distributeModel()."""
        if self._h is not None:
            self._h.set_cluster3d(tolerance is not None, 0.01 if tolerance is None else tolerance)
        self._cluster_tol = tolerance

    def cluster_objects(self, cloud, boxes3d, tolerance=0.01):
        """PointCloudClusterer::clusterObjects (include/PointCloudClusterer.hpp:156-290) through pbd_candidates_cluster3d: cloud an
        organized [h, w, 3] float32 cloud, boxes3d the records' pbd_box3d (capi.BOX3D_DTYPE, e.g. Candidate.box3d, or what
        get_box3d returns) -> (clusters, centres): per record its kept cluster's point indices (row * w + col, ascending; empty
        when none) and its centroid (3 doubles, NaN when none)."""
        b = np.ascontiguousarray(np.asarray(boxes3d).reshape(-1), capi.BOX3D_DTYPE)
        res, idx = self.handle.candidates_cluster3d(cloud, b, tolerance)
        starts = np.concatenate([[0], np.cumsum(res["size"], dtype=np.int64)])
        clusters = [idx[starts[i]:starts[i + 1]].copy() for i in range(len(res))]
        centres = [np.array([r["cx"], r["cy"], r["cz"]], np.float64) for r in res]
        return clusters, centres

    def computeBoundingBoxes(self, im_shape, depth, candidates: List[Candidate], camera):
        """PointCloudClusterer::computeBoundingBoxes (include/PointCloudClusterer.hpp:53-150) without its point cloud: per candidate
        the Rect3d (x, y, z, width, height, depth) — (0, 0, 0, 0, 0, 0) for a skipped one ("contains nans") — and its part
        centres ([nparts, 3]; empty when skipped), through pbd_candidates_box3d.  depth: HxW float32 / float64 (any size)."""
        if not candidates:
            return [], []
        h, w = im_shape[:2]
        d = np.asarray(depth)
        heads, boxes, _ = Candidate._pack(candidates)
        out, cen = self.handle.candidates_box3d(heads, boxes, d, w, h, camera, depth_dtype=d.dtype)
        rects, centers = [], []
        for i, c in enumerate(candidates):
            o = out[i]
            rects.append(tuple(float(o[k]) for k in ("x3d", "y3d", "z3d", "width3d", "height3d", "depth3d")))
            centers.append(cen[i, :len(c.parts)].copy() if o["valid"] else np.zeros((0, 3)))
        return rects, centers

    def setDepthFilter(self, zfactor: Optional[float] = 0.03) -> None:
        """SearchSpacePruning.filterCandidatesByDepth(parts, candidates, depth, zfactor) inside every detect(im, depth) with a
        non-empty depth image — the call the reference leaves commented out (src/PartsBasedDetector.cpp:91-93, zfactor 0.03) —
        on the GPU; None turns it off (the default: depth is ignored).  Kept across distributeModel()."""
        if self._h is not None:
            self._h.set_depth_filter(zfactor is not None, 0.0 if zfactor is None else zfactor)
        self._zfactor = zfactor

    def setCandidateNms(self, kind: int, top: int = 0) -> None:
        """What the NMS of capi.PBD_CAND_SORT_NMS is: capi.PBD_NMS_PAINTED (default, Candidate.nonMaximaSuppression) or
        capi.PBD_NMS_PARTS (Candidate.nonMaximaSuppressionParts: matlab/detection/nms.m, which testmodel.m runs as nms(box, 0.3);
        top = 1000 reproduces its cut, 0 = none).  Kept across distributeModel()."""
        if kind not in (capi.PBD_NMS_PAINTED, capi.PBD_NMS_PARTS) or top < 0:
            raise capi.PbdError(capi.PBD_ERR_ARG, "candidate NMS: kind PBD_NMS_PAINTED / _PARTS, top >= 0")
        if self._h is not None:
            self._h.set_candidate_nms(kind, top)
        self._cand_nms = (kind, top)

    def setCandidateFilter(self, mode: int, overlap: float = 0.0) -> None:
        """Candidate.sort (capi.PBD_CAND_SORT), or sort + Candidate.nonMaximaSuppression(overlap) (capi.PBD_CAND_SORT_NMS), of
        every detect() on the GPU — what the reference's callers run after detect() (ros/Node.cpp:192-196); capi.PBD_CAND_RAW
        (the default) turns it off.  Kept across distributeModel()."""
        if self._h is not None:
            self._h.set_candidate_filter(mode, overlap)
        self._cand_filter = (mode, overlap)

    @property
    def handle(self) -> capi.Handle:
        if self._h is None:
            raise RuntimeError("detect() before distributeModel()")
        return self._h

    def detect(self, im: np.ndarray, depth=None, candidates: Optional[List[Candidate]] = None) -> List[Candidate]:
        """src/PartsBasedDetector.cpp:69-95.  `depth` is ignored like the reference (:91-93) unless setDepthFilter() is on: then
        a non-empty depth image (HxW, converted to T) prunes the 8-bit frame's candidates on the GPU.  Results are APPENDED to
        `candidates` (DynamicProgram.cpp:250)."""
        out = candidates if candidates is not None else []
        if (self._zfactor is not None or self._camera is not None) and depth is not None and np.asarray(depth).size > 0:
            if np.asarray(im).dtype != np.uint8:
                raise capi.PbdError(capi.PBD_ERR_UNSUPPORTED, "depth pruning / 3-D boxes: 8-bit colour frames only")
            got = Candidate._unpack(*self.handle.detect_rgbd(im, depth, self._cap), self._ps())
            if self._camera is not None:
                b3, cen = self.handle.get_box3d(0)
                for i, c in enumerate(got):
                    c.box3d = b3[i].copy()
                    c.part_centers = cen[i, :len(c.parts)].copy() if b3[i]["valid"] else np.zeros((0, 3))
                if self._cluster_tol is not None:
                    res, idx = self.handle.get_cluster3d(0)
                    starts = np.concatenate([[0], np.cumsum(res["size"], dtype=np.int64)])
                    for i, c in enumerate(got):
                        c.centre3d = np.array([res[i]["cx"], res[i]["cy"], res[i]["cz"]], np.float64)
                        c.cluster = idx[starts[i]:starts[i + 1]].copy()
            out.extend(got)
            return out
        # (the image's dtype is its depth: uint8 -> pbd_detect_u8, the other accepted depths -> pbd_detect_image; unsupported ones raise)
        res = self.handle.detect(im, self._cap) if np.asarray(im).dtype == np.uint8 else self.handle.detect_image(im, self._cap)
        out.extend(Candidate._unpack(*res, self._ps()))
        return out

    def pyramidStore(self, slots: int, max_w: int, max_h: int) -> "capi.PyramidStore":
        """A pyramid store with this detector as its producer (include/pbd_c.h "pyramid store"): `slots` device-resident feature
        pyramids of frames up to max_w x max_h, computed once by put() and then detected (detectStored) or mined (mineNegatives, train)
        by any detector on the same device with this one's sbin, interval, pyramid kind, boundary pad and dtype — whatever its model.
        Close it before this detector's handle (the handle's close() does)."""
        return capi.PyramidStore(self.handle, slots, max_w, max_h)

    def detectStored(self, frame: "capi.StoredFrame", candidates: Optional[List[Candidate]] = None) -> List[Candidate]:
        """detect() on a frame of a pyramid store: what detect(image) returns for the image that was put, in bits, without the image
        pyramid and HOG.  No depth stages; with setPartScores on, the Candidates carry their parts' scores."""
        out = candidates if candidates is not None else []
        out.extend(Candidate._unpack(*self.handle.detect_stored(frame.store, frame.slot, self._cap), self._ps()))
        return out

    def detect_latent(self, im: np.ndarray, truth, overlap: float, mix=None, component: int = -1) -> List[Candidate]:
        """detect(im, model, thresh, bbox, overlap) of matlab/detection/detect.m: the single highest-scoring pose whose every part
        overlaps its box in `truth` ([nparts, 4] rows of x, y, width, height as detect() returns them) by more than `overlap`
        (in [0, 1)); mix[p] >= 0 fixes part p's mixture (-1 / None: free); component = -1 searches all.  Returns one Candidate or
        an empty list; the model's threshold plays no part.  With setPartScores on, the Candidate carries its parts' scores."""
        return Candidate._unpack(*self.handle.detect_latent(im, truth, overlap, mix, component), self._ps())

    def detectGtBox(self, im: np.ndarray, gt, overlap: float = 0.3):
        """matlab/detection/testmodel_gtbox.m:17-21: detect at the model's threshold, then per gt box (x1, y1, x2, y2) the
        highest-scoring pose whose box of part centres covers more than `overlap` of it (bestoverlap.m) — selected on the GPU, only
        the winners come home.  Returns (one Candidate or None per gt box, their overlaps).  RAW candidate mode, no depth stages,
        no per-part scores."""
        heads, boxes, locs, found, o = self.handle.detect_gtbox(im, gt, overlap)
        hit = np.flatnonzero(found)
        cands = iter(Candidate._unpack(heads[hit], boxes[hit], locs[hit]))
        return [next(cands) if f else None for f in found], o

    def features(self, candidates: List[Candidate]):
        """The feature vectors of `candidates` (what detect() or detect_latent() of the LAST frame returned, or a selection of them):
        (blocks [n, max_parts] capi.FEATURE_BLOCK_DTYPE, windows [n, max_parts, wmax] in the handle's dtype), gathered on the GPU
        from the frame's resident feature planes — the ex.blocks of matlab/detection/detect.m:272-308.  model.dense_feature_vectors
        scatters them into Model.weight_vector()'s order."""
        heads, _, locs = Candidate._pack(candidates)
        return self.handle.candidates_features(heads, locs)

    def writeExamples(self, candidates: List[Candidate], cache: "capi.QpCache", label: int, id: int) -> int:
        """detect(im, model, thresh, [], 0, id, label)'s qp_write of every detection (matlab/learning/train.m:102): `candidates` (of
        the LAST frame, or a selection of them) are appended to `cache` (capi.QpCache on this detector's handle) as standardised
        block-sparse examples, gathered on the GPU from the frame's resident feature planes.  Returns how many were written: a full
        cache takes no more and is no error."""
        heads, _, locs = Candidate._pack(candidates)
        return cache.write(heads, locs, label, id)

    def writeWarped(self, im: np.ndarray, boxes, cache: "capi.QpCache", filter: int = None, bias: int = None, ids=None):
        """poswarp of matlab/learning/train.m:131-161: the positive boxes ((x1, y1, x2, y2), 1-based inclusive, of the 8-bit frame `im`)
        warped to the root filter's size (warppos.m), HOGed and appended to `cache` as [bias | window] positives, all on the GPU.
        filter / bias default to component 0's root (warppos.m:6, model.bias.i).  Boxes smaller than prod(maxsize * sbin) — the
        largest filter height and width of the model, train.m:135 — are skipped.  -> (written, status per box).  `im` may be a
        capi.DeviceFrame: the frame is then read from device memory (capi.QpCache.write_warped_dev), with the same result in bits."""
        m = self.handle.model
        filter = int(m.filterid[0][0][0]) if filter is None else int(filter)
        bias = int(m.biasid[0][0][0]) if bias is None else int(bias)
        maxsize = m.filter_sizes().max(axis=0)
        min_area = float(maxsize[0] * m.sbin) * float(maxsize[1] * m.sbin)
        if isinstance(im, capi.DeviceFrame):
            return cache.write_warped_dev(im, boxes=boxes, filter=filter, bias=bias, min_area=min_area, ids=ids)
        return cache.write_warped(im, boxes, filter, bias, min_area, ids)

    def latentPositives(self, positives, cache: "capi.QpCache", overlap: float = 0.6, first_id: int = 1):
        """poslatent of matlab/learning/train.m:166-193: every item (image, truth[, mix]) — truth [nparts, 4] rows of x, y, width,
        height as detect() returns them — whose parts all have a box area (width + 1) * (height + 1) of at least prod(maxsize * sbin)
        (the largest filter rows and columns of the model, train.m:170,179-182) is cropped around its boxes (croppos.m; the crop is a
        view, nothing is copied), and the best pose overlapping them becomes one positive of `cache` without leaving the GPU
        (capi.QpCache.write_latent).  The image id is the item's index, first_id + i (MATLAB: 1-based), skipped items included.
        Returns (numpositives [ncomponents]: the found poses per component, blocks: per item its capi.LATENT_EXAMPLE_DTYPE record or
        None where the item was skipped).  Fixing the positives as support vectors (train.m:90-91) stays the caller's cache.fix.
        An item's image may be a capi.DeviceFrame: the crop is then pointer arithmetic on its device pointer and the frame is read in
        place (capi.QpCache.write_latent_dev), with the array item's result in bits."""
        if cache.handle is not self.handle:
            raise ValueError("latentPositives: the cache is bound to another detector")
        m = self.handle.model
        maxsize = m.filter_sizes().max(axis=0)
        minsize = float(maxsize[0] * m.sbin) * float(maxsize[1] * m.sbin)
        counts, blocks = np.zeros(m.ncomponents, np.int64), []
        for i, item in enumerate(positives):
            dev = isinstance(item[0], capi.DeviceFrame)
            im, truth = item[0] if dev else np.asarray(item[0]), np.asarray(item[1], np.int32).reshape(-1, 4)
            mix = item[2] if len(item) > 2 else None
            area = (truth[:, 2].astype(np.float64) + 1) * (truth[:, 3].astype(np.float64) + 1)
            if np.any(area < minsize):
                blocks.append(None)
                continue
            (x, y, w, h), tr = capi.croppos(truth, len(truth), im.shape[1], im.shape[0])
            if dev:
                v = im.crop(x, y, w, h)
                v.sync()
                blk = cache.write_latent_dev(v.dptr, v.w, v.hgt, v.cn, tr, overlap, first_id + i, mix, stride=v.stride)
            else:
                blk = cache.write_latent(im[y:y + h, x:x + w], tr, overlap, first_id + i, mix)
            blocks.append(blk)
            if blk["found"]:
                counts[int(blk["component"])] += 1
        return counts, blocks

    def mineNegatives(self, images, cache: "capi.QpCache", first_id: int = 0, tol: float = .05, max_iter: int = 1000, seed: int = 0):
        """matlab/learning/train.m:99-108 with detect.m's optimize at frame granularity: every image is mined into `cache`
        (capi.QpCache.mine with id first_id + i: detected on this detector at its threshold — train.m uses -1, setThresh —, the records
        written as negatives on the GPU, ub grown by their slack); on PBD_MINE_OPT the cache runs opt(tol, max_iter, seed) then prune(),
        on PBD_MINE_ONE one() over a shuffle of find(sv) drawn as opt draws it; after either the weights go into this detector
        (apply_weights).  Stops behind the image after which sum(sv) == capacity (train.m:105).  Returns (records, written, action) per
        image mined.  Not done here: detect.m updates the model in the middle of a frame and visits levels and components in a random
        order.  train.m:96's model.interval = 2 while mining is setInterval(2) around this call (train.train does it)."""
        if cache.handle is not self.handle:
            raise ValueError("mineNegatives: the cache is bound to another detector")
        out = []
        for i, im in enumerate(images):
            # (an item that is a capi.StoredFrame is mined from its pyramid-store slot: the same records, examples and action in bits)
            rec, wr, act = cache.mine_stored(im.store, im.slot, first_id + i) if isinstance(im, capi.StoredFrame) else cache.mine(im, first_id + i)
            out.append((rec, wr, act))
            if act == capi.PBD_MINE_OPT:
                cache.opt(tol, max_iter, seed)
                cache.prune()
            elif act == capi.PBD_MINE_ONE:
                cache.one(shuffled_support(cache, seed))
            if act != capi.PBD_MINE_NONE:
                cache.apply_weights()
            if int(cache.support().sum()) == cache.dims()[2]:
                break
        return out

    def evaluation(self, max_instances: int, max_detections: int, apk_thresh: float = .5) -> "Evaluation":
        """An evaluation ledger on this detector's handle (include/pbd_c.h "evaluation ledger"): eval_pck.m / eval_apk.m / VOCap.m with
        the records left on the device.  One keypoint per part: every component of the model must have the same number of parts."""
        return Evaluation(capi.Eval(self.handle, self.model.nparts(0), max_instances, max_detections, apk_thresh))


class Evaluation:
    """matlab/evaluation on the GPU: test frames go in with their annotated persons (points [ngt, P, 2], scale [ngt]); per frame only
    counts and found flags come back; pck() and apk() return P doubles each.  addPck runs testmodel_gtbox.m's protocol (the best pose
    on every person's keypoint box), addApk testmodel.m's (the detector's threshold, candidate filter and NMS: setCandidateFilter(
    PBD_CAND_SORT_NMS, 0.3) with setCandidateNms(PBD_NMS_PARTS, 1000) is nms.m)."""
    SCALE_LAST, SCALE_OWN = capi.PBD_EVAL_SCALE_LAST, capi.PBD_EVAL_SCALE_OWN

    def __init__(self, ledger: "capi.Eval"):
        self.ledger = ledger

    def addPck(self, im: np.ndarray, points, scale, overlap: float = 0.3) -> np.ndarray:
        """-> found [ngt]: which persons have a pose"""
        return self.ledger.pck_frame(im, points, scale, overlap)

    def addPckBatch(self, frames, persons, overlap: float = 0.3):
        """persons = [(points, scale)] per frame -> [found] per frame"""
        return self.ledger.pck_batch(frames, persons, overlap)

    def addApk(self, im: np.ndarray, points, scale) -> int:
        """-> the frame's final records"""
        return self.ledger.apk_frame(im, points, scale)

    def addApkBatch(self, frames, persons) -> np.ndarray:
        return self.ledger.apk_batch(frames, persons)

    def pck(self, thresh: float = .5, rule: int = capi.PBD_EVAL_SCALE_LAST) -> np.ndarray:
        """rule: SCALE_LAST is eval_pck.m:13 as written (the last instance's scale for all), SCALE_OWN each instance's own"""
        return self.ledger.pck(thresh, rule)

    def apk(self, curves: bool = False):
        return self.ledger.apk(curves)

    def reset(self) -> None:
        self.ledger.reset()

    def dims(self):
        return self.ledger.dims()

    def close(self) -> None:
        self.ledger.close()


def shuffled_support(cache: "capi.QpCache", seed: int = 0) -> np.ndarray:
    """find(qp.sv) of the cache's examples, shuffled the way pbd_qp_opt shuffles its first pass: Fisher-Yates from the back, the
    draws SplitMix64(seed) modulo the positions left"""
    I = [int(i) for i in np.flatnonzero(cache.support())]
    s, M = int(seed) & 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF
    for u in range(len(I) - 1, 0, -1):
        s = (s + 0x9E3779B97F4A7C15) & M
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        j = z % (u + 1)
        I[u], I[j] = I[j], I[u]
    return np.asarray(I, np.int32)
