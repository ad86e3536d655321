"""Model I/O: the reference's cv::FileStorage model layout (src/FileStorageModel.cpp:42-159)
read and written without OpenCV by pbd::FileStorageModel, checked through the pbd_modelconv CLI."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import Model, make_face_like_model, make_tree_model

CONV = os.path.join(os.path.dirname(capi.LIB_PATH), "host", "pbd_modelconv")


def _same(a: Model, b: Model):
    assert (a.interval, a.sbin, a.norient, a.flen) == (b.interval, b.sbin, b.norient, b.flen)
    assert np.float32(a.thresh) == np.float32(b.thresh)
    assert len(a.filtersw) == len(b.filtersw)
    for x, y in zip(a.filtersw, b.filtersw):
        np.testing.assert_array_equal(np.asarray(x, np.float32), np.asarray(y, np.float32))
    np.testing.assert_array_equal(np.asarray(a.biasw, np.float32), np.asarray(b.biasw, np.float32))
    np.testing.assert_array_equal(np.asarray(a.defw, np.float32), np.asarray(b.defw, np.float32))
    np.testing.assert_array_equal(np.asarray(a.anchors), np.asarray(b.anchors))
    assert a.filterid == b.filterid and a.parentid[0][1:] == b.parentid[0][1:]
    for c in range(a.ncomponents):
        for p in range(a.nparts(c)):
            k = len(a.filterid[c][p])
            assert (list(a.biasid[c][p]) * k)[:k] == list(b.biasid[c][p])[:k] or list(a.biasid[c][p]) == list(b.biasid[c][p])[: len(a.biasid[c][p])]
            if p > 0:
                assert list(a.defid[c][p]) == list(b.defid[c][p])


def _conv(src, dst):
    out = subprocess.run([CONV, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


@pytest.mark.parametrize("ext", [".xml", ".yaml"])
@pytest.mark.parametrize("kind", ["tree_k3", "face"])
def test_filestorage_reader_roundtrip(tmp_path, ext, kind):
    assert os.path.exists(CONV), "build() did not produce pbd_modelconv"
    m = make_tree_model([-1, 0, 1, 1, 0], 3, seed=5, thresh=-0.65) if kind == "tree_k3" else \
        make_face_like_model(seed=8, ncomp=3, nfilters=12, part_counts=(4, 6), thresh=0.25)
    m.name = "Synthetic"
    # Python writes the OpenCV-2.4 layout -> C++ FileStorageModel::deserialize -> flat dump -> Python
    src = tmp_path / ("model" + ext)
    m.save_filestorage(str(src))
    _conv(src, tmp_path / "a.bin")
    _same(m, Model.load(str(tmp_path / "a.bin")))
    # C++ FileStorageModel::serialize -> deserialize again (both text formats)
    for ext2 in (".xml", ".yml"):
        _conv(tmp_path / "a.bin", tmp_path / ("b" + ext2))
        _conv(tmp_path / ("b" + ext2), tmp_path / "c.bin")
        _same(m, Model.load(str(tmp_path / "c.bin")))


def test_binary_dump_roundtrip(tmp_path):
    m = make_tree_model([-1, 0, 0], 2, seed=6, thresh=1.5)
    m.save(str(tmp_path / "m.bin"))
    _same(m, Model.load(str(tmp_path / "m.bin")))


def test_reader_rejects_garbage(tmp_path):
    (tmp_path / "bad.xml").write_text("<opencv_storage><name>x</name></opencv_storage>")
    out = subprocess.run([CONV, str(tmp_path / "bad.xml"), str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert out.returncode != 0 and "Error deserializing" in out.stdout   # deserialize() returns false (demo.cpp:79-82)


def test_filestorage_reader_literal_defid(tmp_path):
    """--literal-defid: `defid` read exactly as src/FileStorageModel.cpp:148-152 reads it — a scalar int is kept, any other node (the K-element
    sequence of a part with several mixtures; in YAML every flow sequence) becomes {0}; the default reader keeps the sequences."""
    assert os.path.exists(CONV), "build() did not produce pbd_modelconv"
    m3 = make_tree_model([-1, 0, 1], 3, seed=5)           # K = 3: defid sequences of three
    m1 = make_tree_model([-1, 0, 1], 1, seed=5)           # K = 1: one index per part
    for m, ext, want in ((m3, ".xml", "zero"), (m1, ".xml", "kept"), (m1, ".yaml", "zero")):
        src = tmp_path / ("m" + ext)
        m.name = "Synthetic"
        m.save_filestorage(str(src))
        out = subprocess.run([CONV, "--literal-defid", str(src), str(tmp_path / "lit.bin")], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        lit = Model.load(str(tmp_path / "lit.bin"))
        _conv(src, tmp_path / "dflt.bin")
        dflt = Model.load(str(tmp_path / "dflt.bin"))
        for p in range(1, m.nparts(0)):
            assert list(dflt.defid[0][p]) == list(m.defid[0][p])
            if want == "zero":      # (the flat dump repeats the single index for every mixture of the part)
                assert set(lit.defid[0][p]) == {0} and any(v != 0 for v in m.defid[0][p]) or p == 1 and list(m.defid[0][p])[0] == 0, (ext, p, lit.defid[0][p])
            else:
                assert list(lit.defid[0][p]) == list(m.defid[0][p]), (ext, p, lit.defid[0][p])


@pytest.mark.parametrize("ext", [".xml", ".yaml"])
def test_roundtrip_mixture_count_per_part(tmp_path, ext):
    """A model whose parts have 1 to 8 mixtures (one L x K bias block per child, a part with one shared deformation and bias row):
    the binary dump, and the reference's FileStorage layout through the C++ reader and writer, keep every per-part index list."""
    from partsbaseddetector_amd.model import make_tree_model_k
    assert os.path.exists(CONV), "build() did not produce pbd_modelconv"
    m = make_tree_model_k([-1, 0, 0, 1, 1, 2], [1, 3, 6, 1, 8, 2], seed=8, shared=[5], thresh=-0.5)
    m.name = "Synthetic"
    m.save(str(tmp_path / "m.bin"))
    back = Model.load(str(tmp_path / "m.bin"))
    _same(m, back)
    assert back.biasid == m.biasid and back.defid == m.defid
    src = tmp_path / ("model" + ext)
    m.save_filestorage(str(src))
    _conv(src, tmp_path / "a.bin")
    a = Model.load(str(tmp_path / "a.bin"))
    _same(m, a)
    assert a.biasid == m.biasid and [len(f) for f in a.filterid[0]] == [1, 3, 6, 1, 8, 2]
    for ext2 in (".xml", ".yml"):
        _conv(tmp_path / "a.bin", tmp_path / ("b" + ext2))
        _conv(tmp_path / ("b" + ext2), tmp_path / "c.bin")
        c = Model.load(str(tmp_path / "c.bin"))
        _same(m, c)
        assert c.biasid == m.biasid and c.defid[0][1:] == m.defid[0][1:]
