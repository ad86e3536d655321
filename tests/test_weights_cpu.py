"""Weight and threshold updates (include/pbd_c.h "weight and threshold updates") without a GPU: the six entry points are declared,
exported and bound, the ABI version stays 5, NULL arguments are refused before anything touches a device, and
Model.positive_threshold is train.m:117-118.  The updates themselves: tests/test_gpu_weights.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pbd_set_weights", "pbd_set_weights_dev", "pbd_get_weights", "pbd_qp_apply_weights", "pbd_set_threshold", "pbd_get_threshold"]


def test_symbols_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "pbd_c.h")) as f:
        header = f.read()
    L = capi.lib()
    for name in SYMBOLS:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in capi.EXPORTS and getattr(L, name) is not None, name
    assert re.search(r"#define PBD_ABI_VERSION 5\b", header)
    assert L.pbd_abi_version() == 5 == capi.PBD_ABI_VERSION
    for name in ("set_weights", "weights", "set_threshold", "threshold"):
        assert hasattr(capi.Handle, name), name
    assert hasattr(capi.QpCache, "apply_weights")


def test_null_arguments():
    L = capi.lib()
    w = np.zeros(4)
    t = C.c_float(7.0)
    p = w.ctypes.data_as(C.c_void_p)
    assert L.pbd_set_weights(None, p, 4) == capi.PBD_ERR_ARG
    assert L.pbd_set_weights(None, None, 0) == capi.PBD_ERR_ARG
    assert L.pbd_set_weights_dev(None, p, 4) == capi.PBD_ERR_ARG
    assert L.pbd_get_weights(None, p, 4) == capi.PBD_ERR_ARG
    assert L.pbd_qp_apply_weights(None) == capi.PBD_ERR_ARG
    assert L.pbd_set_threshold(None, C.c_float(0.0)) == capi.PBD_ERR_ARG
    assert L.pbd_get_threshold(None, C.byref(t)) == capi.PBD_ERR_ARG and t.value == 7.0


def train_m_threshold(scores):
    """train.m:117-118, literally: r = sort(qp_scorepos()); model.thresh = r(ceil(length(r)*.05)) — 1-based"""
    r = sorted(float(s) for s in scores)
    return r[math.ceil(len(r) * .05) - 1]


@pytest.mark.parametrize("n", [1, 19, 20, 21])
def test_positive_threshold(n):
    scores = np.random.default_rng(n).normal(0.0, 1.0, n)
    want = train_m_threshold(scores)
    assert Model.positive_threshold(scores) == want
    assert Model.positive_threshold(list(scores[::-1]), q=0.05) == want
    # 1..20 scores: the lowest; 21: the second lowest
    assert want == np.sort(scores)[0 if n <= 20 else 1]


def test_positive_threshold_refuses_no_scores():
    with pytest.raises(ValueError):
        Model.positive_threshold([])
