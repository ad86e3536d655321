"""Model container + synthetic model / image generators.

`Model` mirrors the reference's `Model` (include/Model.hpp:49-122): the same
fields with the same meaning, numpy instead of cv::Mat.  The reference's model
files are an un-vendored submodule (.gitmodules:1-3), so benchmarks and tests
use seeded synthetic models with the structure the reference's MATLAB side
produces (matlab/learning/buildmodel.m:19-80): see SURVEY.md §8(d).

init_model, data_def, merge_models and build_model are that MATLAB side itself
(initmodel.m, data_def.m, mergemodels.m, buildmodel.m): with capi.cluster_parts
(clusterparts.m) they make a model and its mixture labels from annotations.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List

import numpy as np


class pbd_model_desc(C.Structure):
    """ctypes mirror of include/pbd_c.h `pbd_model_desc`."""

    _fields_ = [
        ("nfilters", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("flen", C.c_int32),
        ("norient", C.c_int32), ("sbin", C.c_int32), ("interval", C.c_int32), ("thresh", C.c_float),
        ("filters", C.POINTER(C.c_float)),
        ("ndefs", C.c_int32), ("defw", C.POINTER(C.c_float)), ("anchors", C.POINTER(C.c_int32)),
        ("nbias", C.c_int32), ("biasw", C.POINTER(C.c_float)),
        ("ncomponents", C.c_int32),
        ("part_offset", C.POINTER(C.c_int32)), ("parentid", C.POINTER(C.c_int32)),
        ("mix_offset", C.POINTER(C.c_int32)), ("filterid", C.POINTER(C.c_int32)),
        ("defid", C.POINTER(C.c_int32)), ("biasid", C.POINTER(C.c_int32)),
    ]


@dataclass
class Model:
    """include/Model.hpp:49-122.  Index vectors are 0-based (after zeroIndex)."""

    filtersw: List[np.ndarray]            # filters(): each kh x (kw*flen) float32, interleaved
    biasw: np.ndarray                     # bias()
    anchors: np.ndarray                   # anchors(): [ndefs, 2] (x, y)
    defw: np.ndarray                      # def(): [ndefs, 4]
    filterid: List[List[List[int]]]       # [component][part][mixture]
    biasid: List[List[List[int]]]
    defid: List[List[List[int]]]
    parentid: List[List[int]]             # [component][part]
    interval: int = 10                    # nscales()
    thresh: float = 0.0
    sbin: int = 4                         # binsize()
    norient: int = 18
    flen: int = 32
    name: str = "synthetic"
    _keep: list = field(default_factory=list, repr=False)

    @property
    def ncomponents(self) -> int:
        return len(self.filterid)

    def nparts(self, c: int) -> int:
        return len(self.filterid[c])

    @property
    def max_parts(self) -> int:
        return max(self.nparts(c) for c in range(self.ncomponents))

    def filter_sizes(self) -> np.ndarray:
        """[nfilters, 2] int32: (rows kh, cols kw) of every filter."""
        return np.asarray([(f.shape[0], f.shape[1] // self.flen) for f in self.filtersw], np.int32).reshape(-1, 2)

    def is_uniform(self) -> bool:
        """True when every filter has one size (what pbd_create and the binary dump take)."""
        fs = self.filter_sizes()
        return bool((fs == fs[0]).all())

    def save(self, path: str) -> None:
        """Flat little-endian dump read by pbd::BinaryModel (partsbaseddetector_amd/host/pbd_host.hpp).
        The format has ONE kh, kw: a mixed bank is refused (ValueError) before the file is opened."""
        import struct
        if not self.is_uniform():
            raise ValueError("binary model dump: the format carries one filter size; this model's filters have "
                             f"several ({sorted(set(map(tuple, self.filter_sizes().tolist())))}) — use save_filestorage")
        kh = self.filtersw[0].shape[0]
        kw = self.filtersw[0].shape[1] // self.flen
        with open(path, "wb") as f:
            f.write(b"PBDMODL1")
            f.write(struct.pack("<12i", len(self.filtersw), kh, kw, self.flen, self.norient, self.sbin, self.interval,
                                len(self.defw), len(self.biasw), self.ncomponents, 0, 0))
            f.write(struct.pack("<f", float(np.float32(self.thresh))))
            for w in self.filtersw:
                f.write(np.ascontiguousarray(w, np.float32).tobytes())
            f.write(np.ascontiguousarray(self.defw, np.float32).tobytes())
            f.write(np.ascontiguousarray(self.anchors, np.int32).tobytes())
            f.write(np.ascontiguousarray(self.biasw, np.float32).tobytes())
            for c in range(self.ncomponents):
                f.write(struct.pack("<i", self.nparts(c)))
                for p in range(self.nparts(c)):
                    k = len(self.filterid[c][p])
                    d = (list(self.defid[c][p]) + [0] * k)[:k] if p > 0 else [0] * k
                    b = list(self.biasid[c][p])
                    b = (b + [b[0] if b else 0] * k)[:k]
                    f.write(struct.pack("<2i", self.parentid[c][p] if p > 0 else -1, k))
                    f.write(np.asarray(self.filterid[c][p], np.int32).tobytes())
                    f.write(np.asarray(d, np.int32).tobytes())
                    f.write(np.asarray(b, np.int32).tobytes())

    @staticmethod
    def load(path: str) -> "Model":
        """Read the flat dump written by `save` / pbd::BinaryModel::serialize / pbd_modelconv."""
        import struct
        with open(path, "rb") as f:
            if f.read(8) != b"PBDMODL1":
                raise ValueError("not a PBDMODL1 file")
            nf, kh, kw, flen, norient, sbin, interval, ndefs, nbias, ncomp, _, _ = struct.unpack("<12i", f.read(48))
            thresh = struct.unpack("<f", f.read(4))[0]
            filt = [np.frombuffer(f.read(kh * kw * flen * 4), np.float32).reshape(kh, kw * flen).copy() for _ in range(nf)]
            defw = np.frombuffer(f.read(ndefs * 16), np.float32).reshape(ndefs, 4).copy()
            anchors = np.frombuffer(f.read(ndefs * 8), np.int32).reshape(ndefs, 2).copy()
            biasw = np.frombuffer(f.read(nbias * 4), np.float32).copy()
            filterid, defid, biasid, parentid = [], [], [], []
            for _c in range(ncomp):
                npart = struct.unpack("<i", f.read(4))[0]
                fi, di, bi, pa = [], [], [], []
                for p in range(npart):
                    par, k = struct.unpack("<2i", f.read(8))
                    fi.append(np.frombuffer(f.read(4 * k), np.int32).tolist())
                    d = np.frombuffer(f.read(4 * k), np.int32).tolist()
                    bi.append(np.frombuffer(f.read(4 * k), np.int32).tolist())
                    di.append(d if p > 0 else [])
                    pa.append(par)
                filterid.append(fi); defid.append(di); biasid.append(bi); parentid.append(pa)
        return Model(filt, biasw, anchors, defw, filterid, biasid, defid, parentid, interval, thresh, sbin, norient,
                     flen, os.path.basename(path))

    def save_filestorage(self, path: str) -> None:
        """Write the reference's on-disk format (cv::FileStorage layout of
        FileStorageModel::serialize, src/FileStorageModel.cpp:42-94) as OpenCV 2.4 emits it:
        XML for .xml, YAML for .yaml/.yml.  Used to exercise pbd::FileStorageModel::deserialize."""
        num = lambda v: (repr(float(np.float32(v))).replace("e-0", "e-0") if float(v) != int(v) else f"{int(v)}.")
        xml = path.endswith(".xml")
        o = []
        if xml:
            o += ['<?xml version="1.0"?>', "<opencv_storage>", f"<name>{self.name}</name>", f"<interval>{self.interval}</interval>",
                  f"<thresh>{num(self.thresh)}</thresh>", f"<sbin>{self.sbin}</sbin>", f"<norient>{self.norient}</norient>",
                  f"<flen>{self.flen}</flen>", "<filtersw>"]
            for w in self.filtersw:
                data = " ".join(num(v) for v in w.ravel())
                o += ['  <_ type_id="opencv-matrix">', f"    <rows>{w.shape[0]}</rows>", f"    <cols>{w.shape[1]}</cols>",
                      "    <dt>d</dt>", "    <data>", "      " + data + "</data></_>"]
            o += ["</filtersw>", "<biasw>", "  " + " ".join(num(v) for v in self.biasw) + "</biasw>", "<anchors>"]
            for a in np.asarray(self.anchors).reshape(-1, 2):
                o += ["  <_>", f"    {int(a[0])} {int(a[1])}</_>"]
            o += ["</anchors>", "<defs>"]
            for d in np.asarray(self.defw).reshape(-1, 4):
                o += ["  <_>", "    " + " ".join(num(v) for v in d) + "</_>"]
            o += ["</defs>", "<indexers>"]
            for c in range(self.ncomponents):
                o.append(f"  <component-{c}>")
                for p in range(self.nparts(c)):
                    di = self.defid[c][p] if p > 0 else []
                    o += [f"    <part-{p}>", f"      <parentid>{self.parentid[c][p] if p > 0 else 0}</parentid>",
                          "      <filterid>" + " ".join(map(str, self.filterid[c][p])) + "</filterid>",
                          "      <biasid>" + " ".join(map(str, self.biasid[c][p])) + "</biasid>",
                          "      <defid>" + " ".join(map(str, di)) + f"</defid></part-{p}>"]
                o.append(f"  </component-{c}>")
            o += ["</indexers>", "</opencv_storage>"]
        else:
            def flow(vals, per=8, ind="       "):
                vals = list(vals)
                rows = [", ".join(vals[i:i + per]) for i in range(0, len(vals), per)]
                return "[ " + (",\n" + ind).join(rows) + " ]"
            o += ["%YAML:1.0", f"name: {self.name}", f"interval: {self.interval}", f"thresh: {num(self.thresh)}",
                  f"sbin: {self.sbin}", f"norient: {self.norient}", f"flen: {self.flen}", "filtersw:"]
            for w in self.filtersw:
                o += ["   - !!opencv-matrix", f"      rows: {w.shape[0]}", f"      cols: {w.shape[1]}", "      dt: d",
                      "      data: " + flow([num(v) for v in w.ravel()], 6, "          ")]
            o += ["biasw: " + flow([num(v) for v in self.biasw]), "anchors:"]
            o += [f"   - [ {int(a[0])}, {int(a[1])} ]" for a in np.asarray(self.anchors).reshape(-1, 2)]
            o += ["defs:"] + ["   - " + flow([num(v) for v in d]) for d in np.asarray(self.defw).reshape(-1, 4)]
            o += ["indexers:"]
            for c in range(self.ncomponents):
                o.append(f"   component-{c}:")
                for p in range(self.nparts(c)):
                    di = self.defid[c][p] if p > 0 else []
                    o += [f"      part-{p}:", f"         parentid: {self.parentid[c][p] if p > 0 else 0}",
                          "         filterid: [ " + ", ".join(map(str, self.filterid[c][p])) + " ]",
                          "         biasid: [ " + ", ".join(map(str, self.biasid[c][p])) + " ]",
                          "         defid: [ " + ", ".join(map(str, di)) + " ]"]
        with open(path, "w") as f:
            f.write("\n".join(o) + "\n")

    def feature_layout(self) -> dict:
        """Where each block of a detection's feature vector (pbd_feature_block) sits in the dense vector, and in weight_vector():
        [biasw | defw (ndefs x 4) | the filters back to back, each [kh][kw * flen]].  -> dict(bias=0, deform=nbias,
        filters=[nfilters] first element of each filter, size=total length).  The MATLAB ancestor addresses its blocks through the
        `.i` offsets of its model struct; the reference's C++ Model carries none of them, so this order is the port's own."""
        nb = int(np.asarray(self.biasw).size)
        nd = int(np.asarray(self.defw).size) // 4
        sizes = [int(np.asarray(f).size) for f in self.filtersw]
        off = nb + 4 * nd + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        return dict(bias=0, deform=nb, filters=off[:-1], size=int(off[-1]))

    def weight_vector(self) -> np.ndarray:
        """The model's weights as one float64 vector in feature_layout()'s order: w . x of a detection's dense feature vector
        (dense_feature_vectors) is its score."""
        return np.concatenate([np.asarray(self.biasw, np.float32).ravel(), np.asarray(self.defw, np.float32).ravel()] +
                              [np.asarray(f, np.float32).ravel() for f in self.filtersw]).astype(np.float64)

    def qp_vectors(self):
        """matlab/learning/model2vec.m in feature_layout()'s order: (w, wreg, w0, noneg) — the weights (float64), the regulariser
        (.01 at the root bias of every component, 1 elsewhere), the weights' origin (.01 at elements 0 and 2 of every deformation, the
        minimum quadratic deformation cost, 0 elsewhere) and the 0-based indices that must stay non-negative (those same elements,
        uint32, deformation by deformation)."""
        lay = self.feature_layout()
        w = self.weight_vector()
        wreg, w0 = np.ones(lay["size"], np.float64), np.zeros(lay["size"], np.float64)
        nd = int(np.asarray(self.defw).size) // 4
        noneg = (lay["deform"] + 4 * np.repeat(np.arange(nd), 2) + np.tile([0, 2], nd)).astype(np.uint32)
        w0[noneg] = .01
        for c in range(self.ncomponents):
            wreg[lay["bias"] + int(self.biasid[c][0][0])] = .01
        return w, wreg, w0, noneg

    def with_weight_vector(self, w) -> "Model":
        """matlab/learning/vec2model.m in feature_layout()'s order, the inverse of weight_vector(): a copy of this model whose biases,
        deformations and filters are `w`'s elements (QpCache.weights() after a solve).  The model stores float32, so vec2model.m's
        closing assertion w == model2vec(model) holds on float32-ROUNDED weights: with_weight_vector(w).weight_vector() equals
        np.float32(w), and equals w exactly when w is float32-representable."""
        import copy
        lay = self.feature_layout()
        w = np.asarray(w, np.float64).ravel()
        if w.size != lay["size"]:
            raise ValueError(f"w must have feature_layout()['size'] = {lay['size']} elements")
        if not np.isfinite(w).all():
            raise ValueError("w must be finite")
        m = copy.copy(self)
        m._keep = []
        nb = int(np.asarray(self.biasw).size)
        m.biasw = w[:nb].astype(np.float32)
        m.defw = w[lay["deform"]:lay["deform"] + np.asarray(self.defw).size].astype(np.float32).reshape(np.asarray(self.defw).shape)
        m.filtersw = [w[int(o):int(o) + np.asarray(f).size].astype(np.float32).reshape(np.asarray(f).shape)
                      for o, f in zip(lay["filters"], self.filtersw)]
        return m

    @staticmethod
    def positive_threshold(scores, q: float = 0.05) -> float:
        """matlab/learning/train.m:117-118, r = sort(qp_scorepos()); model.thresh = r(ceil(length(r) * .05)): the score that a fraction
        q of the positives fall at or below — the threshold a trained model ships with.  scores: the positives' raw scores
        (QpCache.score(w, positives) / cpos), at least one."""
        r = np.sort(np.asarray(scores, np.float64).ravel())
        if r.size == 0:
            raise ValueError("positive_threshold: no scores")
        return float(r[max(int(np.ceil(r.size * np.float64(q))), 1) - 1])

    def to_desc(self) -> pbd_model_desc:
        """Flatten into the C ABI descriptor (arrays kept alive on self).  Uniform banks only (pbd_create)."""
        kh = self.filtersw[0].shape[0]
        kw = self.filtersw[0].shape[1] // self.flen
        for f in self.filtersw:
            if f.shape != (kh, kw * self.flen):
                raise ValueError("all filters must have the same size")
        filt = np.ascontiguousarray(np.stack(self.filtersw).astype(np.float32))
        return self._desc(filt, kh, kw)

    def to_desc_sized(self):
        """(desc, fsize) for pbd_create_sized: the filters back to back, each at its own size; desc.kh = desc.kw = 0 and
        fsize[n] = (kh_n, kw_n).  Any bank, uniform or mixed (arrays kept alive on self)."""
        for f in self.filtersw:
            if f.ndim != 2 or f.shape[1] % self.flen:
                raise ValueError("a filter must be kh x (kw*flen)")
        fsize = np.ascontiguousarray(self.filter_sizes())
        filt = np.ascontiguousarray(np.concatenate([np.asarray(f, np.float32).ravel() for f in self.filtersw]))
        d = self._desc(filt, 0, 0)
        self._keep.append(fsize)
        return d, fsize

    def _desc(self, filt, kh, kw) -> pbd_model_desc:
        defw = np.ascontiguousarray(np.asarray(self.defw, np.float32).reshape(-1, 4))
        anchors = np.ascontiguousarray(np.asarray(self.anchors, np.int32).reshape(-1, 2))
        biasw = np.ascontiguousarray(np.asarray(self.biasw, np.float32))
        part_offset, parentid, mix_offset, fid, did, bid = [0], [], [0], [], [], []
        for c in range(self.ncomponents):
            for p in range(self.nparts(c)):
                parentid.append(self.parentid[c][p] if p > 0 else -1)
                k = len(self.filterid[c][p])
                fid += list(self.filterid[c][p])
                d = list(self.defid[c][p]) if p > 0 else []
                did += (d + [0] * k)[:k]
                b = list(self.biasid[c][p])
                bid += (b + [b[0] if b else 0] * k)[:k]
                mix_offset.append(mix_offset[-1] + k)
            part_offset.append(part_offset[-1] + self.nparts(c))
        arrs = [np.asarray(a, np.int32) for a in (part_offset, parentid, mix_offset, fid, did, bid)]
        self._keep = [filt, defw, anchors, biasw] + arrs
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        d = pbd_model_desc()
        d.nfilters, d.kh, d.kw, d.flen = len(self.filtersw), kh, kw, self.flen
        d.norient, d.sbin, d.interval, d.thresh = self.norient, self.sbin, self.interval, float(self.thresh)
        d.filters = fp(filt)
        d.ndefs, d.defw, d.anchors = defw.shape[0], fp(defw), ip(anchors)
        d.nbias, d.biasw = biasw.shape[0], fp(biasw)
        d.ncomponents = self.ncomponents
        d.part_offset, d.parentid, d.mix_offset = ip(arrs[0]), ip(arrs[1]), ip(arrs[2])
        d.filterid, d.defid, d.biasid = ip(arrs[3]), ip(arrs[4]), ip(arrs[5])
        return d


def dense_feature_vectors(model: Model, blocks, windows) -> np.ndarray:
    """[n, feature_layout()["size"]] float64: every record's blocks (pbd_feature_block [n, max_parts]) and windows ([n, max_parts,
    wmax]) scatter-added into Model.feature_layout()'s order — 1 at bias_id, def at its def_id, the window at its filter_id.  Part
    slots with ids -1 (beyond the record's parts) are skipped.
    Asserts what matlab/learning/qp_write.m:34-35 asserts: no block index repeats within a record.  That fails for a model that uses
    one filter id (or one def / bias id) for two parts of one component — the blocks would have to be summed, which the QP's
    sparse format does not do."""
    lay = model.feature_layout()
    sizes = model.filter_sizes()
    blocks = np.asarray(blocks)
    n, mp = blocks.shape
    windows = np.asarray(windows).reshape(n, mp, -1)
    out = np.zeros((n, lay["size"]), np.float64)
    for i in range(n):
        seen = set()
        for p in range(mp):
            b = blocks[i, p]
            if b["bias_id"] < 0:
                continue
            ids = [("bias", int(b["bias_id"])), ("filter", int(b["filter_id"]))] + ([("def", int(b["def_id"]))] if b["def_id"] >= 0 else [])
            assert not seen.intersection(ids), f"record {i}: a block index repeats within the record ({sorted(seen.intersection(ids))})"
            seen.update(ids)
            out[i, lay["bias"] + int(b["bias_id"])] += 1.0
            if b["def_id"] >= 0:
                o = lay["deform"] + 4 * int(b["def_id"])
                out[i, o:o + 4] += np.asarray(b["def"], np.float64)
            f = int(b["filter_id"])
            kh, kw = int(sizes[f, 0]), int(sizes[f, 1])
            assert (kh, kw) == (int(b["kh"]), int(b["kw"])), "block size differs from the model's filter"
            o = int(lay["filters"][f])
            out[i, o:o + kh * kw * model.flen] += windows[i, p, :kh * kw * model.flen].astype(np.float64)
    return out


# PARSE-style 26-part skeleton, 0-based parents (any tree with parent < child is valid)
PERSON_TREE = [-1, 0, 1, 2, 3, 4, 5, 2, 7, 8, 9, 10, 11, 12, 1, 14, 15, 16, 17, 14, 19, 20, 21, 22, 23, 24]


def _filters(rng, n, kh, kw, flen):
    w = rng.normal(0.0, 0.05, size=(n, kh, kw, flen)).astype(np.float32)
    w[..., flen - 1] = rng.normal(-0.1, 0.02, size=(n, kh, kw)).astype(np.float32)
    return [np.ascontiguousarray(w[i].reshape(kh, kw * flen)) for i in range(n)]


def _defs(rng, n, max_anchor=4):
    d = np.stack([rng.uniform(0.005, 0.05, n), rng.uniform(-0.01, 0.01, n),
                  rng.uniform(0.005, 0.05, n), rng.uniform(-0.01, 0.01, n)], axis=1).astype(np.float32)
    a = rng.integers(-max_anchor, max_anchor + 1, size=(n, 2)).astype(np.int32)
    return d, a


def make_tree_model(parents, K, seed=1234, kh=5, kw=5, sbin=4, interval=10, thresh=0.0, name="tree") -> Model:
    """One component, `len(parents)` parts, K mixtures per part.

    Layout of matlab/learning/buildmodel.m: filter p*K+k; child deformation
    (p-1)*K+k; child bias matrix L x K with biasid(l,k) = base + k*L + l; a
    single scalar root bias (= 0).
    """
    rng = np.random.default_rng(seed)
    P = len(parents)
    flen = 32
    filt = _filters(rng, P * K, kh, kw, flen)
    defw, anchors = _defs(rng, (P - 1) * K)
    L = K
    biasw = np.concatenate([[0.0], rng.normal(0.0, 0.1, (P - 1) * K * L)]).astype(np.float32)
    filterid = [[[p * K + k for k in range(K)] for p in range(P)]]
    defid = [[[] if p == 0 else [(p - 1) * K + k for k in range(K)] for p in range(P)]]
    biasid = [[[0] if p == 0 else [1 + (p - 1) * K * L + k * L for k in range(K)] for p in range(P)]]
    return Model(filt, biasw, anchors, defw, filterid, biasid, defid, [list(parents)], interval, thresh, sbin,
                 18, flen, name)


def make_tree_model_k(parents, Ks, seed=1234, kh=5, kw=5, sbin=4, interval=10, thresh=0.0, shared=(), quantised=False,
                      name="tree-k") -> Model:
    """One component, `len(parents)` parts, Ks[p] mixtures for part p (src/DynamicProgram.cpp:99-100 allows any count per part).

    buildmodel.m layout with a count per part: the filters of part p back to back (filter sum(Ks[:p]) + k), one deformation
    row per child mixture, and for child p with parent count L = Ks[parents[p]] an L x K bias block at `base`:
    biasid[p][k] = base + k*L, so bias(k)[m] = biasw[base + k*L + m]; a single scalar root bias (= 0).
    `shared` (True, or an iterable of parts): every mixture of such a part has one deformation row and one bias row, whose
    entries are all equal — with equal responses its K weighted maps tie exactly.  `quantised`: biases are multiples of 1/4 and
    deformations dyadic (1/32 or 1/16 quadratic, 0 or +-1/128 linear), so sums of them and of small-integer responses are exact."""
    rng = np.random.default_rng(seed)
    P = len(parents)
    assert len(Ks) == P and parents[0] == -1 and all(0 <= parents[p] < p for p in range(1, P)) and min(Ks) >= 1
    flen = 32
    shared = set(range(P)) if shared is True else set(shared)
    f0 = np.concatenate([[0], np.cumsum(Ks)]).astype(int)
    filt = _filters(rng, int(f0[-1]), kh, kw, flen)
    filterid = [[[int(f0[p]) + k for k in range(Ks[p])] for p in range(P)]]
    defid, biasid, rows = [[[]]], [[[0]]], 0
    biasw = [0.0]
    for p in range(1, P):
        K, L = Ks[p], Ks[parents[p]]
        nd = 1 if p in shared else K
        defid[0].append([rows + (0 if p in shared else k) for k in range(K)])
        rows += nd
        base = len(biasw)
        if p in shared:
            v = float(rng.integers(-4, 5)) * 0.25 if quantised else float(rng.normal(0.0, 0.1))
            biasw += [v] * L
            biasid[0].append([base] * K)
        else:
            vals = rng.integers(-4, 5, K * L) * 0.25 if quantised else rng.normal(0.0, 0.1, K * L)
            biasw += [float(x) for x in vals]
            biasid[0].append([base + k * L for k in range(K)])
    defw, anchors = _defs(rng, rows)
    if quantised:
        defw = np.stack([rng.choice([1 / 32, 1 / 16], rows), rng.choice([-1 / 128, 0.0, 1 / 128], rows),
                         rng.choice([1 / 32, 1 / 16], rows), rng.choice([-1 / 128, 0.0, 1 / 128], rows)], axis=1).astype(np.float32)
    return Model(filt, np.asarray(biasw, np.float32), anchors, defw.reshape(-1, 4), filterid, biasid, defid, [list(parents)],
                 interval, thresh, sbin, 18, flen, name)


# ---- model assembly: what matlab/learning/trainmodel.m runs around the training rounds (INTEGRATION.md "From annotations to a model") ----
def init_model(w, h, sbin, tsize=None) -> Model:
    """matlab/learning/initmodel.m: the one-part model every part's warped training starts from.  w, h: the width and height
    (x2 - x1 + 1, y2 - y1 + 1) of the first part's box in every positive.  The template is square: the 5th-percentile area
    areas[floor(n * .05) - 1] of the sorted areas gives floor(sqrt(area) / sbin) cells a side, 32 features a cell; `tsize` = (rows,
    cols[, 32]) overrides it.  One bias (0) and one zero filter; interval 10.  Fewer than 20 positives without tsize: ValueError (the
    file indexes element 0 of a 1-based array)."""
    if tsize is None:
        areas = np.sort(np.asarray(h, np.float64).ravel() * np.asarray(w, np.float64).ravel())
        at = int(np.floor(areas.size * 0.05))
        if at < 1:
            raise ValueError(f"init_model: {areas.size} positives — the 5th-percentile area needs at least 20 (or pass tsize)")
        side = int(np.floor(np.sqrt(areas[at - 1]) / sbin))
        tsize = (side, side, 32)
    tsize = tuple(int(v) for v in tsize)
    if len(tsize) == 2:
        tsize += (32,)
    if tsize[0] < 1 or tsize[1] < 1 or tsize[2] != 32:
        raise ValueError(f"init_model: a template of {tsize[0]} x {tsize[1]} cells x {tsize[2]} features")
    return Model([np.zeros((tsize[0], tsize[1] * 32), np.float32)], np.zeros(1, np.float32), np.zeros((0, 2), np.int32),
                 np.zeros((0, 4), np.float32), [[[0]]], [[[0]]], [[[]]], [[-1]], 10, 0.0, int(sbin), 18, 32, "init")


def data_def(points, w, h, maxsize) -> np.ndarray:
    """matlab/learning/data_def.m: the parts' positions in HOG cells of the template.  points [n][P][2] (x, y) of part p in positive i;
    w, h [n] as for init_model; maxsize = (rows, cols) of the template (init_model(...).filter_sizes()[0]).  -> [P][n][2] float64,
    points / scale with scale_i = sqrt(w_i * h_i) / sqrt(maxsize[0] * maxsize[1]): the layout capi.cluster_parts takes."""
    points = np.asarray(points, np.float64)
    if points.ndim != 3 or points.shape[2] != 2:
        raise ValueError("data_def: points [n, P, 2]")
    w, h = np.asarray(w, np.float64).ravel(), np.asarray(h, np.float64).ravel()
    if len(w) != len(points) or len(h) != len(points):
        raise ValueError("data_def: one width and height per positive")
    scale = np.sqrt(w * h) / np.sqrt(np.float64(int(maxsize[0]) * int(maxsize[1])))
    return np.ascontiguousarray(np.transpose(points / scale[:, None, None], (1, 0, 2)))


def merge_models(models) -> Model:
    """matlab/learning/mergemodels.m in Model terms: the models' components, filters, biases and deformations appended in order, every
    id of model j shifted by what models 0 .. j-1 hold.  The scalars (interval, sbin, ...) are the first model's, as in the file.
    Every bias of every model is appended: mergemodels.m:12 writes model.bias(nb+1) inside its loop over i, which keeps only the last
    bias of a model that has several; trainmodel.m passes one-bias models, where both agree."""
    import copy
    models = list(models)
    if not models:
        raise ValueError("merge_models: no models")
    m = copy.copy(models[0])
    m._keep = []
    m.filtersw = [np.asarray(f, np.float32) for f in models[0].filtersw]
    m.biasw = np.asarray(models[0].biasw, np.float32).ravel()
    m.defw = np.asarray(models[0].defw, np.float32).reshape(-1, 4)
    m.anchors = np.asarray(models[0].anchors, np.int32).reshape(-1, 2)
    shift = lambda ids, by: [[[int(v) + by for v in mix] for mix in part] for part in ids]
    m.filterid, m.biasid, m.defid = shift(m.filterid, 0), shift(m.biasid, 0), shift(m.defid, 0)
    m.parentid = [list(c) for c in m.parentid]
    for x in models[1:]:
        nb, nf, nd = len(m.biasw), len(m.filtersw), len(m.defw)
        m.biasw = np.concatenate([m.biasw, np.asarray(x.biasw, np.float32).ravel()])
        m.filtersw = m.filtersw + [np.asarray(f, np.float32) for f in x.filtersw]
        m.defw = np.concatenate([m.defw, np.asarray(x.defw, np.float32).reshape(-1, 4)])
        m.anchors = np.concatenate([m.anchors, np.asarray(x.anchors, np.int32).reshape(-1, 2)])
        m.filterid += shift(x.filterid, nf)
        m.biasid += shift(x.biasid, nb)
        m.defid += shift(x.defid, nd)
        m.parentid += [list(c) for c in x.parentid]
    return m


def build_model(part_models, deffeat, idx, parents, interval=None, sbin=None, thresh=0.0, name="joint") -> Model:
    """matlab/learning/buildmodel.m:19-80: the per-part models put together into the tree model the joint training starts from.
    part_models[p]: part p's mixtures (merge_models of its K trained one-part models: filter k is mixture k's); deffeat [P][n][2]
    (data_def); idx [P][n] the positives' 0-based mixture labels (capi.cluster_parts); parents 0-based, -1 at the root, parent < child.
    Part p has max(idx[p]) + 1 mixtures.  Layout (make_tree_model_k's): the parts' filters back to back; one zero root bias; child p an
    L x K block of zero biases, L its parent's count, biasid[p][k] = base + k * L; one deformation [.01 0 .01 0] per child mixture whose
    anchor is round([mean x, mean y]) of child - parent over the positives labelled k — the differences summed left to right in
    float64, rounded half away from zero as the file rounds it (round(mean + 1), then the loader's - 1: a mean of exactly -.5 gives 0).
    ValueError: a label below the maximum that no positive carries (the file's anchor would be NaN), a part model with fewer filters
    than the part has mixtures, parents not as above."""
    deffeat = np.asarray(deffeat, np.float64)
    idx = np.asarray(idx)
    parents = [int(v) for v in parents]
    P = len(parents)
    if deffeat.ndim != 3 or deffeat.shape[0] != P or deffeat.shape[2] != 2 or idx.shape != deffeat.shape[:2] or len(part_models) != P:
        raise ValueError("build_model: deffeat [P, n, 2], idx [P, n], one part model and one parent per part")
    if P < 1 or parents[0] != -1 or any(not 0 <= parents[p] < p for p in range(1, P)):
        raise ValueError("build_model: parents are 0-based with -1 at part 0 only and parent < child")
    if idx.size == 0 or idx.min() < 0:
        raise ValueError("build_model: labels are 0-based and every part has at least one positive")
    Ks = [int(idx[p].max()) + 1 for p in range(P)]
    filt, biasw, defw, anchors = [], [0.0], [], []
    filterid, defid, biasid = [[]], [[]], [[]]
    for p in range(P):
        K = Ks[p]
        if len(part_models[p].filtersw) < K:
            raise ValueError(f"build_model: part {p} has {K} mixtures, its part model {len(part_models[p].filtersw)} filters")
        if p == 0:
            biasid[0].append([0])
        else:
            L = Ks[parents[p]]
            biasid[0].append([len(biasw) + k * L for k in range(K)])
            biasw += [0.0] * (K * L)
        filterid[0].append([len(filt) + k for k in range(K)])
        filt += [np.array(part_models[p].filtersw[k], np.float32) for k in range(K)]
        if p == 0:
            defid[0].append([])
            continue
        defid[0].append([len(defw) + k for k in range(K)])
        for k in range(K):
            sel = idx[p] == k
            if not sel.any():
                raise ValueError(f"build_model: no positive carries mixture {k} of part {p} (the anchor would be NaN)")
            mean = [np.cumsum(deffeat[p][sel, a] - deffeat[parents[p]][sel, a])[-1] / np.float64(sel.sum()) for a in (0, 1)]
            one = [v + 1.0 for v in mean]                                           # d.anchor = round([x+1 y+1 0])
            anchors.append([int(np.copysign(np.floor(abs(v) + 0.5), v)) - 1 for v in one])   # ... and zeroIndex
            defw.append([0.01, 0.0, 0.01, 0.0])
    first = part_models[0]
    return Model(filt, np.asarray(biasw, np.float32), np.asarray(anchors, np.int32).reshape(-1, 2),
                 np.asarray(defw, np.float32).reshape(-1, 4), filterid, biasid, defid, [parents],
                 first.interval if interval is None else int(interval), float(thresh), first.sbin if sbin is None else int(sbin),
                 first.norient, first.flen, name)


def make_person_model(seed=1234, K=6, thresh=0.0, interval=10, sbin=4) -> Model:
    """26 parts x K mixtures: 156 filters / 150 deformations / 901 biases for K=6."""
    return make_tree_model(PERSON_TREE, K, seed=seed, thresh=thresh, interval=interval, sbin=sbin,
                           name=f"person26x{K}")


def make_mixed_person_model(seed=1234, K=6, root=(7, 7), odd_sizes=((3, 5), (6, 4)), thresh=0.0, interval=10,
                            sbin=4) -> Model:
    """make_person_model with a size per filter: the K root filters root[0] x root[1], the filters of parts 1 .. len(odd_sizes) the
    sizes of odd_sizes (all K mixtures of a part one size), every other filter 5 x 5."""
    m = make_person_model(seed=seed, K=K, thresh=thresh, interval=interval, sbin=sbin)
    rng = np.random.default_rng(seed + 1)
    sizes = {0: tuple(root)}
    sizes.update({1 + i: tuple(sz) for i, sz in enumerate(odd_sizes)})
    for p, (kh, kw) in sizes.items():
        new = _filters(rng, K, kh, kw, m.flen)
        for k in range(K):
            m.filtersw[m.filterid[0][p][k]] = new[k]
    m.name = f"person26x{K}-mixed"
    return m


def make_voc_like_model(seed=11, roots=((6, 4), (7, 7), (5, 8)), part_size=(4, 4), nparts=(6, 5, 6), thresh=0.0,
                        interval=5, sbin=4) -> Model:
    """The layout matlab/modelTransfer.m modelTransferVOC2Face (:76-150) writes for a Felzenszwalb VOC model: one component per
    root, a star tree (every part's parent is the root), one mixture per part, a root filter of the component's own size and part
    filters of another size (here 4 x 4, an even size).  Filters of component c: its root, then its parts; a bias per component
    root and per part (1 x 1 bias matrices), a deformation per part.  Sides stay within the library's 1..9."""
    rng = np.random.default_rng(seed)
    flen = 32
    filt, filterid, defid, biasid, parentid = [], [], [], [], []
    ndefs = 0
    biasw = []
    for c, rs in enumerate(roots):
        P = nparts[c % len(nparts)]
        f0 = len(filt)
        filt += _filters(rng, 1, rs[0], rs[1], flen) + _filters(rng, P - 1, part_size[0], part_size[1], flen)
        filterid.append([[f0 + p] for p in range(P)])
        defid.append([[] if p == 0 else [ndefs + p - 1] for p in range(P)])
        ndefs += P - 1
        b0 = len(biasw)
        biasw += [float(x) for x in rng.normal(0.0, 0.1, P)]
        biasid.append([[b0 + p] for p in range(P)])
        parentid.append([-1] + [0] * (P - 1))
    defw, anchors = _defs(rng, ndefs, max_anchor=3)
    return Model(filt, np.asarray(biasw, np.float32), anchors, defw, filterid, biasid, defid, parentid, interval,
                 thresh, sbin, 18, flen, "voc-like")


def make_face_like_model(seed=77, ncomp=13, nfilters=146, part_counts=(39, 68), thresh=0.0, interval=5,
                         sbin=4) -> Model:
    """13 single-mixture components sharing one filter pool (matlab/modelTransfer.m:188-229):
    root bias per component, a dummy zero bias shared by all children."""
    rng = np.random.default_rng(seed)
    flen = 32
    filt = _filters(rng, nfilters, 5, 5, flen)
    filterid, defid, biasid, parentid = [], [], [], []
    ndefs = 0
    biasw = [0.0]  # index 0: the children's dummy zero bias
    for c in range(ncomp):
        P = part_counts[c % len(part_counts)]
        ids = rng.permutation(nfilters)[:P]
        par = [-1] + [int(rng.integers(max(0, p - 3), p)) for p in range(1, P)]
        filterid.append([[int(ids[p])] for p in range(P)])
        defid.append([[] if p == 0 else [ndefs + p - 1] for p in range(P)])
        ndefs += P - 1
        biasw.append(float(rng.normal(0.0, 0.1)))
        biasid.append([[len(biasw) - 1] if p == 0 else [0] for p in range(P)])
        parentid.append(par)
    defw, anchors = _defs(rng, ndefs, max_anchor=2)
    return Model(filt, np.asarray(biasw, np.float32), anchors, defw, filterid, biasid, defid, parentid, interval,
                 thresh, sbin, 18, flen, "face-like")


def make_image(seed: int, w: int, h: int, cn: int = 3) -> np.ndarray:
    """uint8 BGR test image: oriented gratings + filled rectangles/ellipses + noise,
    so every one of the 18 orientation bins and a wide range of magnitudes occur."""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.full((h, w, 3), 110.0, np.float32)
    for _ in range(6):
        th = rng.uniform(0, np.pi)
        f = rng.uniform(0.02, 0.25)
        amp = rng.uniform(8, 30, size=3)
        ph = rng.uniform(0, 2 * np.pi)
        g = np.sin((xx * np.cos(th) + yy * np.sin(th)) * f * 2 * np.pi + ph)
        img += g[..., None] * amp[None, None, :]
    for _ in range(40):
        x0, y0 = rng.integers(0, w), rng.integers(0, h)
        sw, sh = rng.integers(4, max(5, w // 4)), rng.integers(4, max(5, h // 4))
        col = rng.uniform(0, 255, size=3)
        if rng.random() < 0.5:
            m = (xx >= x0) & (xx < x0 + sw) & (yy >= y0) & (yy < y0 + sh)
        else:
            m = ((xx - x0) / sw) ** 2 + ((yy - y0) / sh) ** 2 < 1.0
        a = rng.uniform(0.4, 1.0)
        img[m] = (1 - a) * img[m] + a * col
    img += rng.normal(0, 8, size=img.shape)
    out = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if cn == 1:
        out = np.ascontiguousarray(out[..., 1])
    return np.ascontiguousarray(out)


def make_wide_image(kind, seed: int, w: int, h: int, cn: int = 3) -> np.ndarray:
    """A test image of one of the other depths the reference accepts (src/HOGFeatures.cpp:136-146) whose values USE the depth's range (not
    an 8-bit image in a wider container): np.uint16 -> the full 16 bits; np.float32 -> [0, 1] floats; np.float64 -> doubles incl. negative ones."""
    rng = np.random.default_rng(seed)
    base = make_image(seed, w, h, cn)
    kind = np.dtype(kind)
    if kind == np.uint16:
        return (base.astype(np.uint16) * 257) ^ rng.integers(0, 256, base.shape, dtype=np.uint16)
    noise = rng.uniform(-0.5, 0.5, base.shape)
    if kind == np.float32:
        return ((base + noise) / 255.0).astype(np.float32)
    if kind == np.float64:
        return (base + noise).astype(np.float64) * 3.0 - 100.0
    raise ValueError("make_wide_image: uint16, float32 or float64")
