"""Filter banks with a size per filter, the parts that need no GPU: the C ABI (header, library, binding), argument checks of
pbd_create_sized ahead of any HIP call, model I/O of mixed banks (the reference's XML / YAML layout through pbd::FileStorageModel)
and the binary dump's refusal of a bank it cannot represent."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import Model, make_mixed_person_model, make_voc_like_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV = os.path.join(os.path.dirname(capi.LIB_PATH), "host", "pbd_modelconv")


def test_sized_entry_points_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    for name in ("pbd_create_sized", "pbd_group_create_sized", "pbd_get_filter_size"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name)
    assert int(re.search(r"#define PBD_ABI_VERSION (\d+)", hdr).group(1)) == capi.PBD_ABI_VERSION == 5
    assert capi.lib().pbd_abi_version() == 5


def _create_sized(desc, fsize):
    L = capi.lib()
    h = C.c_void_p()
    opt = capi.pbd_options()
    fs = None if fsize is None else np.ascontiguousarray(fsize, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    rc = L.pbd_create_sized(C.byref(desc), fs, C.byref(opt), C.byref(h))
    msg = L.pbd_last_error(h).decode() if h else ""
    if h:
        L.pbd_destroy(h)
    return rc, msg


def test_create_sized_argument_errors_before_any_hip_call():
    m = make_voc_like_model()
    desc, fsize = m.to_desc_sized()
    assert desc.kh == 0 and desc.kw == 0 and fsize.shape == (len(m.filtersw), 2)
    assert _create_sized(desc, None)[0] == capi.PBD_ERR_ARG
    desc.kh = 5
    assert _create_sized(desc, fsize)[0] == capi.PBD_ERR_ARG
    desc.kh = 0
    for side in (0, 10):
        bad = fsize.copy()
        bad[3, 1] = side
        rc, msg = _create_sized(desc, bad)
        assert rc == capi.PBD_ERR_UNSUPPORTED and "filter 3" in msg, (rc, msg)
    # a filter id out of range is still refused by the model checks (PBD_ERR_ARG), not by the size permutation
    fid = np.ctypeslib.as_array(desc.filterid, shape=(1,))
    keep = int(fid[0])
    fid[0] = len(m.filtersw)
    assert _create_sized(desc, fsize)[0] == capi.PBD_ERR_ARG
    fid[0] = keep


def test_model_sized_descriptor_and_uniform_desc():
    m = make_mixed_person_model(K=2)
    assert not m.is_uniform()
    with pytest.raises(ValueError):
        m.to_desc()                      # the oracle's uniform descriptor keeps refusing a mixed bank
    desc, fsize = m.to_desc_sized()
    assert desc.nfilters == len(m.filtersw)
    total = sum(int(a) * int(b) for a, b in fsize) * m.flen
    flat = np.ctypeslib.as_array(desc.filters, shape=(total,))
    np.testing.assert_array_equal(flat, np.concatenate([f.ravel() for f in m.filtersw]))
    v = make_voc_like_model()
    sizes = {tuple(s) for s in v.filter_sizes().tolist()}
    assert len(sizes) >= 3 and any(a % 2 == 0 or b % 2 == 0 for a, b in sizes)
    assert all(1 <= a <= 9 and 1 <= b <= 9 for a, b in sizes)
    assert all(len(k) == 1 for comp in v.filterid for k in comp)                  # K = 1
    assert all(all(p == 0 for p in par[1:]) for par in v.parentid)                # star trees


def _conv(src, dst):
    return subprocess.run([CONV, str(src), str(dst)], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("ext", [".xml", ".yml"])
def test_mixed_model_filestorage_roundtrip(tmp_path, ext):
    """Python writer -> C++ FileStorageModel (pbd_modelconv) -> writer -> reader: the per-filter sizes survive."""
    assert os.path.exists(CONV)
    m = make_voc_like_model(seed=3)
    m.name = "VocLike"
    m.save_filestorage(str(tmp_path / ("a" + ext)))
    out = _conv(tmp_path / ("a" + ext), tmp_path / ("b" + ext))
    assert out.returncode == 0, out.stdout + out.stderr
    out = _conv(tmp_path / ("b" + ext), tmp_path / ("c" + ext))
    assert out.returncode == 0, out.stdout + out.stderr
    assert (tmp_path / ("b" + ext)).read_text() == (tmp_path / ("c" + ext)).read_text()
    text = (tmp_path / ("b" + ext)).read_text()
    for kh, kw in m.filter_sizes().tolist():   # each filter written at its own size
        assert re.search(r"rows:?\s*\"?%d" % kh, text) or f"<rows>{kh}</rows>" in text
    # and the C++ reader hands the model to the text writer unchanged: the uniform-size part of the model round-trips bit-exactly
    u = make_voc_like_model(seed=3, roots=((4, 4),) * 3)
    assert u.is_uniform()
    u.save_filestorage(str(tmp_path / ("u" + ext)))
    assert _conv(tmp_path / ("u" + ext), tmp_path / "u.bin").returncode == 0
    back = Model.load(str(tmp_path / "u.bin"))
    for x, y in zip(u.filtersw, back.filtersw):
        np.testing.assert_array_equal(x, y)


def test_binary_dump_refuses_a_mixed_bank(tmp_path):
    m = make_voc_like_model()
    with pytest.raises(ValueError, match="one filter size"):
        m.save(str(tmp_path / "m.bin"))
    assert not (tmp_path / "m.bin").exists()
    m.save_filestorage(str(tmp_path / "m.xml"))
    out = _conv(tmp_path / "m.xml", tmp_path / "out.bin")
    assert out.returncode != 0 and "one filter size" in out.stdout, out.stdout
    assert not (tmp_path / "out.bin").exists()
