"""The frame planner (partsbaseddetector_amd/csrc/pbd_plan.cpp) on the host, no GPU: tests/tools/plan_check.cpp plans a model and a
frame with fake buffer addresses and checks the tables the kernels would read — every pointer inside the buffer it names with its
full extent, no buffer overlaps beyond the compact plan's two aliasings, every (map, line) of a DT pass covered exactly once, LDS
within bounds, DT_G_NATURAL exactly on the x passes, the same tables when planned twice — and reports the device memory the plan
holds, pinned to what Handle.footprint()[0] returned on an MI355X (256 compute units) before the planner was split out."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import (make_face_like_model, make_mixed_person_model, make_person_model,
                                          make_tree_model)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partsbaseddetector_amd", "csrc")
NCU = 256

PERSON = make_person_model()
CASES = {   # name: (model, frame and handle options, footprint()[0] after one detect() on an MI355X)
    "person_640_b1": (PERSON, dict(), 350815894),
    "person_640_b4": (PERSON, dict(batch=4), 1403253904),
    "person_640_b16": (PERSON, dict(batch=16), 3427735000),
    "person_1080_compact": (PERSON, dict(w=1920, h=1080), 1476770584),
    "person_640_dp2": (PERSON, dict(dp_mode=2), 214234600),
    "person_640_dp1": (PERSON, dict(dp_mode=1), 507133734),
    "face_640": (make_face_like_model(), dict(), 632816892),
    "face_640_dp1": (make_face_like_model(), dict(dp_mode=1), 957937232),
    "k10_nofold": (make_tree_model([-1, 0, 1, 1, 0, 4], 10, seed=3), dict(), 213988898),
    "person_640_f64": (PERSON, dict(f64=True), 529673650),
    "mixed_640": (make_mixed_person_model(), dict(), 350858582),
    "person_640_range": (PERSON, dict(level_begin=3, level_end=30), 283367574),
    "person_640_levelset": (PERSON, dict(levels=[0, 2, 5, 11, 40]), 223621134),
    "person_640_nms": (PERSON, dict(nms_sz=5), 350956619),
    "person_640_u16": (PERSON, dict(depth=capi.PBD_DEPTH_16U), 358852030),
}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = tmp_path_factory.mktemp("plan") / "plan_check.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-I", CSRC,
                           os.path.join(ROOT, "tests", "tools", "plan_check.cpp"), os.path.join(CSRC, "pbd_plan.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.plan_check.restype = C.c_int
    return lib


def plan(lib, model, w=640, h=480, batch=1, depth=capi.PBD_DEPTH_8U, f64=False, dp_mode=0, nms_sz=0, level_begin=0, level_end=0,
         levels=()):
    if model.is_uniform():
        desc, fsize = model.to_desc(), None
    else:
        desc, fsize = model.to_desc_sized()
    opt = capi.pbd_options(0, capi.PBD_CONV_AUTO, 4096, 0, level_begin, level_end,
                           capi.PBD_SCALAR_F64 if f64 else capi.PBD_SCALAR_F32, 0, (C.c_int32 * 2)(nms_sz, dp_mode))
    lv = np.ascontiguousarray(list(levels), np.int32)
    fb = C.c_ulonglong(0)
    rep = C.create_string_buffer(4096)
    rc = lib.plan_check(C.byref(desc), None if fsize is None else fsize.ctypes.data_as(C.c_void_p), int(fsize is not None),
                        C.byref(opt), w, h, 3, batch, depth, lv.ctypes.data_as(C.c_void_p), len(lv), NCU, C.byref(fb), rep,
                        len(rep))
    return rc, fb.value, rep.value.decode()


@pytest.mark.parametrize("name", list(CASES))
def test_plan_invariants_and_footprint(planner, name):
    model, kw, footprint = CASES[name]
    rc, fb, rep = plan(planner, model, **kw)
    assert rc == capi.PBD_OK, rep
    assert fb == footprint, (fb, footprint, rep)
    compact = rep.startswith("compact")
    # compact: large frames (the responses over 400 MB) or dp_mode 2
    assert compact == (name in ("person_640_b16", "person_1080_compact", "person_640_dp2")), rep
    # the three-kernel structure (reduce jobs, no fold jobs): dp_mode 1, more than 8 mixtures a part
    legacy = name in ("person_640_dp1", "face_640_dp1", "k10_nofold")
    assert (re.search(r" 0 reduce jobs", rep) is None) == legacy and (re.search(r" 0 folds", rep) is not None) == legacy, rep


def test_plan_errors(planner):
    # the codes plan_frame answers: a frame too small for the pyramid, a level of more than 32 767 cells a side
    assert plan(planner, PERSON, w=40, h=30)[0] == capi.PBD_ERR_ARG
    rc, _, rep = plan(planner, PERSON, w=140000, h=48)
    assert rc == capi.PBD_ERR_UNSUPPORTED and "16-bit pointers" in rep, rep


@pytest.mark.parametrize("name,kw", [("foldmix7", dict()), ("siblings_1_to_8", dict(f64=True)), ("root1_children_many", dict(batch=4)),
                                     ("L6_child_K1", dict(nms_sz=2)), ("foldmix5", dict(dp_mode=1)), ("k10_among_small", dict()),
                                     ("two_profiles", dict())])
def test_plan_invariants_mixture_count_per_part(planner, name, kw):
    """Parts with different mixture counts (tests/mixture_models.py): the tables pass every check; the fold takes them up to 8
    mixtures a part (fold_mix = the largest count), a part of 10 mixtures or dp_mode 1 takes the three-kernel structure.
    (No footprint pin: none of these was measured on an MI355X.)"""
    from tests.mixture_models import het_model, two_profiles
    model = two_profiles() if name == "two_profiles" else het_model(name)
    rc, fb, rep = plan(planner, model, **kw)
    assert rc == capi.PBD_OK, rep
    assert fb > 0 and not rep.startswith("compact"), rep
    legacy = name == "k10_among_small" or kw.get("dp_mode") == 1
    assert (re.search(r" 0 reduce jobs", rep) is None) == legacy and (re.search(r" 0 folds", rep) is not None) == legacy, rep
