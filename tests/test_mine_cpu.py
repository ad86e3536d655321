"""Hard-negative mining (include/pbd_c.h "hard-negative mining") without a GPU: the three entry points are declared, exported and
bound; NULL arguments are refused before anything touches a device; tests/mine_ref.py's action and block sum on hand-made cases; and
the route of a mining frame (tests/tools/mine_route_check.cpp over pbd_route.hpp).  The mining itself: tests/test_gpu_mine.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from tests import mine_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partsbaseddetector_amd", "csrc")
SYMBOLS = ["pbd_qp_mine_u8", "pbd_qp_mine_dev_u8", "pbd_qp_mine_batch_u8"]


def test_symbols_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "pbd_c.h")) as f:
        header = f.read()
    L = capi.lib()
    for name in SYMBOLS:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in capi.EXPORTS and getattr(L, name) is not None, name
    for name, value in (("PBD_MINE_NONE", 0), ("PBD_MINE_ONE", 1), ("PBD_MINE_OPT", 2)):
        assert re.search(r"^#define " + name + r"\s+" + str(value) + r"\b", header, re.M), name
        assert getattr(capi, name) == value == getattr(mine_ref, name)
    assert re.search(r"#define PBD_ABI_VERSION 5\b", header) and L.pbd_abi_version() == 5
    for name in ("mine", "mine_dev", "mine_batch"):
        assert hasattr(capi.QpCache, name), name
    from partsbaseddetector_amd import PartsBasedDetector
    assert hasattr(PartsBasedDetector, "mineNegatives")


def test_null_arguments():
    L = capi.lib()
    im = np.zeros((8, 8, 3), np.uint8)
    p = im.ctypes.data_as(C.c_void_p)
    out = [C.c_int(7) for _ in range(3)]
    refs = [C.byref(v) for v in out]
    ids = (C.c_int32 * 1)(0)
    ptrs = (C.c_void_p * 1)(im.ctypes.data)
    assert L.pbd_qp_mine_u8(None, p, 8, 8, 3, 24, 0, *refs) == capi.PBD_ERR_ARG
    assert L.pbd_qp_mine_dev_u8(None, p, 8, 8, 3, 24, 0, *refs) == capi.PBD_ERR_ARG
    assert L.pbd_qp_mine_batch_u8(None, ptrs, 1, 8, 8, 3, 24, ids, *refs) == capi.PBD_ERR_ARG
    assert L.pbd_qp_mine_u8(None, None, 8, 8, 3, 24, 0, None, None, None) == capi.PBD_ERR_ARG
    assert [v.value for v in out] == [7, 7, 7]


@pytest.mark.parametrize("lb, ub, n, cap, want", [
    (.94, 1.0, 3, 64, mine_ref.PBD_MINE_ONE),     # 1 - .94 = .06 > .05
    (.96, 1.0, 3, 64, mine_ref.PBD_MINE_NONE),    # 1 - .96 = .04
    (.95, 1.0, 3, 64, mine_ref.PBD_MINE_ONE),     # 1 - .95 rounds to .05000000000000004 > .05, as in MATLAB
    (-1e-300, 1.0, 3, 64, mine_ref.PBD_MINE_OPT),   # lb < 0
    (.99, 1.0, 64, 64, mine_ref.PBD_MINE_OPT),    # a full cache
    (0.0, 0.0, 0, 64, mine_ref.PBD_MINE_NONE),    # 0 / 0 = NaN: the comparison is false
    (1.0, 0.0, 3, 64, mine_ref.PBD_MINE_NONE),    # 1 - inf = -inf
    (0.0, 2.0, 3, 64, mine_ref.PBD_MINE_ONE),     # lb = 0 is not < 0: 1 - 0 > .05
])
def test_action(lb, ub, n, cap, want):
    assert mine_ref.action(lb, ub, n, cap) == want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 192, 193, 257, 1000, 2757])   # (192 / 193: where the scan's four-loads loop starts)
def test_block_sum_against_fsum(n):
    rng = np.random.default_rng(n)
    scores = rng.normal(-1.0, 1.5, n).astype(np.float32)
    cneg = 0.004
    t = mine_ref.ub_terms(scores, cneg)
    # the terms by definition, each operation rounded once
    for s, v in zip(scores[:50], t[:50]):
        assert v == cneg * max(1.0 + float(s), 0.0)
    assert (t >= 0).all() and (t == 0).any() == bool((scores <= -1).any())
    got = mine_ref.ub_term_sum(scores, cneg)
    exact = math.fsum(float(v) for v in t)
    # n - 1 additions, each off by at most half an ulp of a partial sum that never exceeds the sum of the magnitudes
    margin = n * 2.0 ** -53 * math.fsum(abs(float(v)) for v in t)
    assert abs(float(got) - exact) <= margin, (got, exact, margin)
    if n == 1:
        assert got == t[0]


def test_block_sum_is_the_lane_strided_order():
    """65 terms: lane 0 holds t[0] + t[64]; the rest one term each; the fold pairs lane i with lane i + 32, then 16, ..."""
    t = np.ldexp(1.0, -np.arange(65) % 50) * (1 + np.arange(65) * 2.0 ** -30)
    part = t[:64].copy()
    part[0] = t[0] + t[64]
    for h in (32, 16, 8, 4, 2, 1):
        part = part[:h] + part[h:2 * h]
    assert mine_ref.block_sum(t) == part[0]
    assert mine_ref.block_sum([]) == 0.0 and not np.signbit(mine_ref.block_sum([]))


def test_route_of_a_mining_frame(tmp_path):
    exe = tmp_path / "mine_route_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "tools", "mine_route_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures"), r.stdout + r.stderr
