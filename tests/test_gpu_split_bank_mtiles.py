"""The six-product bank's 16-cell M-tiles and 16-filter tiles (k_conv_split32 on v_mfma_f32_16x16x32_bf16), bit for bit against the float64
correlation of tests/exact_bank_cases.py on small frames whose levels are picked for the tiling: levels narrower than an M-tile (M-tiles
straddle rows), of fewer than 16 cells, one cell wider / higher than a multiple of 16 (a one-cell-wide ragged unit, a one-row unit), exactly
one 16 x 16 unit, and several full units side by side; banks whose filter counts end a 16-filter tile, spill one filter into the next, leave an
odd number of 16-filter tiles, are the benched 156 (the last tile holds 12) and need a remainder launch.  Families A1-A3 (delta filters in
every tap, channel group and filter slot: they pin the lane maps of both operands and of the accumulator) and B2 (dense: whole-K sums).
np.array_equal on values, no tolerance."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from tests import exact_bank_cases as X
from tests.test_gpu_exact_banks import _first_difference, _model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [(140, 140), (33, 32)]          # w x h
FAMILIES = ("A1", "A2", "A3", "B2")
PARENT_FORM_VARIANT = 9                  # k_conv_split_variants.hip: the 32x32x16 kernel in the form the product had


def _levels(frame):
    from oracle import orc
    g = orc.geometry(frame[0], frame[1], X.SBIN, X.INTERVAL)
    return [(int(h), int(w)) for h, w in zip(g["cell_h"], g["cell_w"])]


def test_frames_hold_every_kind_of_level():
    levels = [lv for f in FRAMES for lv in _levels(f)]
    assert all(h > 0 and w > 0 for h, w in levels)
    assert any(w < 16 and h * w >= 16 for h, w in levels)          # M-tiles straddle rows
    assert any(h * w < 16 for h, w in levels)                      # less than one M-tile
    assert any(w % 16 == 1 and w > 16 for h, w in levels)          # a one-cell-wide ragged unit
    assert any(h % 16 == 1 and h > 16 for h, w in levels)          # a one-row unit
    assert (16, 16) in levels
    assert any(h >= 32 and w >= 32 for h, w in levels)             # four full units


@functools.lru_cache(maxsize=2)
def _cases(frame, sizes):
    """computed once per (frame, bank geometry), shared by whoever runs it; nobody writes to it"""
    levels = _levels(frame)
    return X.family_a(levels, list(sizes), "f32") + [c for c in X.family_b(levels, list(sizes)) if c.name == "B2"]


def run_mtile_bank(sizes):
    """every case of one bank geometry on both frames through begin_frame / set_level_features / pdf / level_response -> None, or the first
    difference as text"""
    sizes = tuple(map(tuple, sizes))
    per_frame = [_cases(f, sizes) for f in FRAMES]
    assert {c.name.split(".")[0] for c in per_frame[0]} == set(FAMILIES)
    for i, first in enumerate(per_frame[0]):
        h = capi.Handle(_model(first.filters), conv_mode=capi.PBD_CONV_SPLIT, dtype=np.float32)
        assert h.conv_mode == capi.PBD_CONV_SPLIT
        try:
            for frame, cases in zip(FRAMES, per_frame):
                case = cases[i]
                assert all(np.array_equal(a, b) for a, b in zip(case.filters, first.filters))
                h.begin_frame(frame[0], frame[1], 3)
                g = h._geo
                assert [(int(a), int(b)) for a, b in zip(g["cell_h"], g["cell_w"])] == [f.shape[:2] for f in case.feats]
                for l, f in enumerate(case.feats):
                    h.set_level_features(l, f)
                h.pdf()
                for l in range(len(case.feats)):
                    for n in range(len(sizes)):
                        got = h.level_response(l, n)
                        if not np.array_equal(got.astype(np.float64), case.ref[l][n]):
                            return (f"case {case.name} frame {frame} level {l} ({got.shape[0]} x {got.shape[1]} cells) filter {n} {sizes[n]}"
                                    + (f" (tap {case.delta[0][n]}, channel {case.delta[1][n]})" if case.delta else "") + " "
                                    + _first_difference(got, case.ref[l][n]))
        finally:
            h.close()
    return None


@pytest.mark.parametrize("nf", [16, 17, 33, 156, 161])
def test_5x5_filter_counts(gpu_required, nf):
    """a lone 16-filter tile, one filter in a second tile, an odd number of 16-filter tiles, the benched bank (the last tile holds 12), a full
    group of five n-tiles and a remainder launch"""
    diff = run_mtile_bank([(5, 5)] * nf)
    assert diff is None, diff


@pytest.mark.parametrize("kh,kw", [(3, 7), (9, 9)])
def test_other_filter_sizes(gpu_required, kh, kw):
    diff = run_mtile_bank([(kh, kw)] * 33)
    assert diff is None, diff


def test_mixed_bank(gpu_required):
    diff = run_mtile_bank(X.mixed_sizes())
    assert diff is None, diff


def test_parent_form_on_the_tuning_library(gpu_required):
    """PBD_SPLIT_VARIANT=9 on libpbd_hip_tune.so: the 32x32x16 kernel in the form the product had, on the same frames (a fresh child process:
    the library is chosen at import)"""
    tune = os.path.join(ROOT, "partsbaseddetector_amd", "libpbd_hip_tune.so")
    if not os.path.exists(tune):
        pytest.skip("tuning build absent (make -C partsbaseddetector_amd/csrc tune)")
    code = ("import sys\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "from tests.test_gpu_split_bank_mtiles import run_mtile_bank\n"
            "print('DIFF', run_mtile_bank([(5, 5)] * 161))\n")
    env = dict(os.environ, PBD_LIBRARY=tune, PBD_SPLIT_VARIANT=str(PARENT_FORM_VARIANT))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().split("DIFF")[-1].strip() == "None", r.stdout[-2000:]
