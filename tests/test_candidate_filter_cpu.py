"""Candidate sort + NMS on the device (pbd_set_candidate_filter, pbd_group_set_candidate_filter, pbd_candidates_filter):
the C ABI surface and its argument checks, none of which needs a GPU."""
import ctypes as C
import os
import re

from partsbaseddetector_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbd_set_candidate_filter", "pbd_group_set_candidate_filter", "pbd_candidates_filter")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pbd_c.h")).read()
    declared = set(re.findall(r"\b(pbd_[a-z0-9_]+)\s*\(", hdr))
    tune = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libpbd_hip_tune.so"))
    for name in NAMES:
        assert name in declared
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name) and hasattr(tune, name)
    assert "PBD_CAND_RAW = 0, PBD_CAND_SORT = 1, PBD_CAND_SORT_NMS = 2" in hdr
    assert (capi.PBD_CAND_RAW, capi.PBD_CAND_SORT, capi.PBD_CAND_SORT_NMS) == (0, 1, 2)
    for cls in (capi.Handle, capi.Group):
        assert hasattr(cls, "set_candidate_filter")
    assert hasattr(capi.Handle, "candidates_filter")


def test_abi_version_still_5():
    assert capi.lib().pbd_abi_version() == 5 == capi.PBD_ABI_VERSION


def test_null_handle_and_group_are_argument_errors():
    L = capi.lib()
    for mode in (0, 1, 2, 7, -1):
        assert L.pbd_set_candidate_filter(None, mode, C.c_float(0.1)) == capi.PBD_ERR_ARG
        assert L.pbd_group_set_candidate_filter(None, mode, C.c_float(0.1)) == capi.PBD_ERR_ARG
    heads = (capi.pbd_candidate_head * 2)()
    kept = C.c_int(-1)
    assert L.pbd_candidates_filter(None, 2, C.c_float(0.1), 640, 480, heads, None, None, 2, C.byref(kept)) == capi.PBD_ERR_ARG
    assert L.pbd_candidates_filter(None, 1, C.c_float(0.0), 640, 480, heads, None, None, 0, C.byref(kept)) == capi.PBD_ERR_ARG
    assert kept.value == -1


def test_detector_exposes_the_setting():
    from partsbaseddetector_amd import PartsBasedDetector
    det = PartsBasedDetector(cand_filter=(capi.PBD_CAND_SORT_NMS, 0.1))
    det.setCandidateFilter(capi.PBD_CAND_SORT, 0.0)   # before distributeModel: remembered for the handle
    assert det._cand_filter == (capi.PBD_CAND_SORT, 0.0)
    host = open(os.path.join(ROOT, "partsbaseddetector_amd", "host", "pbd_host.hpp")).read()
    assert "void setCandidateFilter(int mode, float overlap" in host
