"""Every filter bank, bit for bit, on operands whose exact responses are fp32 numbers (tests/exact_bank_cases.py; what the cases prove about
themselves: tests/test_exact_bank_cases_cpu.py).  Everything here is np.array_equal on VALUES against a float64 correlation — zeros of either
sign are equal, there are no NaNs and there is no tolerance: a lost part, partial product, tap, channel, filter slot or border constant is a
difference at a reported (case, level, y, x, filter).  Every plane of every level is read (17 levels, 7 648 cells in all)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_tree_model, make_tree_model_k, make_wide_image
from tests import exact_bank_cases as X
from tests.test_split_arith_cpu import split2_f16

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BANKS = {"exact-f32": (capi.PBD_CONV_EXACT, np.float32, "f32"), "exact-f64": (capi.PBD_CONV_EXACT, np.float64, "f64"),
         "mfma-f32": (capi.PBD_CONV_MFMA, np.float32, "f32"), "mfma-f64": (capi.PBD_CONV_MFMA, np.float64, "f64"),
         "bf16x6": (capi.PBD_CONV_SPLIT, np.float32, "f32"), "f16x3": (capi.PBD_CONV_SPLIT_F16, np.float32, "f16")}


def _levels(frame):
    from oracle import orc
    g = orc.geometry(frame[0], frame[1], X.SBIN, X.INTERVAL)
    return [(int(h), int(w)) for h, w in zip(g["cell_h"], g["cell_w"])]


@functools.lru_cache(maxsize=4)
def _cases(frame, sizes, kind):
    """the reference is computed once per (frame, bank geometry, kind) and shared by the banks that run it; nobody writes to it"""
    return X.build_cases(_levels(frame), list(sizes), kind)


def _model(filters):
    """a star of one-mixture parts, one per filter; past the library's 256 parts per component: 256 parts, the first ones with two mixtures"""
    nf, maxp = len(filters), 256
    if nf <= maxp:
        m = make_tree_model([-1] + [0] * (nf - 1), 1, seed=1, sbin=X.SBIN, interval=X.INTERVAL)
    else:
        assert nf <= 2 * maxp
        m = make_tree_model_k([-1] + [0] * (maxp - 1), [2] * (nf - maxp) + [1] * (2 * maxp - nf), seed=1, sbin=X.SBIN, interval=X.INTERVAL)
    assert len(m.filtersw) == nf
    m.filtersw = [np.ascontiguousarray(f, np.float32) for f in filters]
    return m


def _first_difference(got, want):
    y, x = np.argwhere(got.astype(np.float64) != want)[0]
    bits = np.uint32 if got.dtype == np.float32 else np.uint64
    g, w = got[y, x], want[y, x].astype(got.dtype)
    return f"y {y} x {x}: got {g!r} (0x{g.view(bits):x}), want {w!r} (0x{w.view(bits):x})"


def run_bank(bank, sizes, only=None, frames=None):
    """all cases of one bank geometry on both frames (frames: on those) through begin_frame / set_level_features / pdf / level_response ->
    None, or the first difference as text"""
    mode, dtype, kind = BANKS[bank]
    sizes = tuple(map(tuple, sizes))
    frames = list(frames or X.FRAMES)
    per_frame = [_cases(f, sizes, kind) for f in frames]
    for i, first in enumerate(per_frame[0]):
        if only and not first.name.startswith(tuple(only)):
            continue
        h = capi.Handle(_model(first.filters), conv_mode=mode, dtype=dtype)
        assert h.conv_mode == mode
        assert [h.filter_size(n) for n in range(len(sizes))] == list(sizes)
        try:
            for frame, cases in zip(frames, per_frame):
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
                            return (f"{bank} case {case.name} frame {frame} level {l} ({got.shape[0]} x {got.shape[1]} cells) filter {n} "
                                    f"{sizes[n]}" + (f" (tap {case.delta[0][n]}, channel {case.delta[1][n]})" if case.delta else "") + " "
                                    + _first_difference(got, case.ref[l][n]))
        finally:
            h.close()
    return None


@pytest.mark.parametrize("bank", list(BANKS))
@pytest.mark.parametrize("nf,kh,kw", X.BANKS)
def test_every_bank_every_family(gpu_required, bank, nf, kh, kw):
    """EXACT, MFMA (float and double handles), the six-product bfloat16 bank and the three-product binary16 bank (its own families) x
    families A1-A3 (5 placement rounds each), B1-B3 (double handles: AF too) x 16 / 33 / 161 filters of 5 x 5 and 33 of 3 x 3, 9 x 9, 3 x 7, 6 x 4"""
    diff = run_bank(bank, [(kh, kw)] * nf)
    assert diff is None, diff


@pytest.mark.parametrize("bank", list(BANKS))
def test_mixed_banks(gpu_required, bank):
    """pbd_create_sized, 3 x 3 / 5 x 5 / 3 x 7 groups of 20 / 37 / 12 filters in a shuffled caller's order: both group boundaries fall inside an n-tile"""
    diff = run_bank(bank, X.mixed_sizes())
    assert diff is None, diff


def _variant_child(bank, sizes, env):
    tune = os.path.join(ROOT, "partsbaseddetector_amd", "libpbd_hip_tune.so")
    if not os.path.exists(tune):
        pytest.skip("tuning build absent (make -C partsbaseddetector_amd/csrc tune)")
    code = ("import sys\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "from tests.test_gpu_exact_banks import run_bank\n"
            f"print('DIFF', run_bank({bank!r}, {sizes!r}, only=('A1', 'A2', 'A3', 'B2')))\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PBD_LIBRARY=tune, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().split("DIFF")[-1].strip() == "None", r.stdout[-2000:]


@pytest.mark.parametrize("variant", [1, 2, 4, 6, 7, 8])
def test_split_tuning_variants(gpu_required, variant):
    """the kernels behind PBD_SPLIT_VARIANT (tuning build; a fresh child process: the library is chosen at import) on A1-A3 and B2: 161 filters
    = a full group of five n-tiles and one more (variants 7 / 8: groups of four / three)"""
    _variant_child("bf16x6", [(5, 5)] * 161, {"PBD_SPLIT_VARIANT": str(variant)})


@pytest.mark.parametrize("variant", [3, 5, 10, 18, 21])
def test_mfma_tuning_variants(gpu_required, variant):
    """the fp32 kernels behind PBD_MFMA_VARIANT on A1-A3 and B2, 33 filters (a second n-tile holding one)"""
    _variant_child("mfma-f32", [(5, 5)] * 33, {"PBD_MFMA_VARIANT": str(variant)})


# ---- the two writers of a feature's parts -------------------------------------------------------------------------------------------
def _frame(kind):
    if kind == "gray":
        return make_image(21, 130, 100, 1)
    if kind in ("u16", "f32img"):
        return make_wide_image(np.uint16 if kind == "u16" else np.float32, 22, 130, 100)
    return make_image(20, 130, 100, 3)


@pytest.mark.parametrize("mode", [capi.PBD_CONV_SPLIT, capi.PBD_CONV_SPLIT_F16], ids=["bf16x6", "f16x3"])
@pytest.mark.parametrize("kind,sbin,pad", [("colour", 4, 0), ("gray", 4, 0), ("colour", 8, 0), ("gray", 8, 0), ("colour", 6, 0),
                                           ("u16", 4, 0), ("f32img", 4, 0), ("colour", 4, 3)])
def test_both_writers_of_the_parts_agree(gpu_required, mode, kind, sbin, pad):
    """k_hog's epilogue writes the split parts of every real frame (8-bit at sbin 4 / 8, the generic cell size 6 through k_hog<T, 0, 0>, 16-bit
    and float frames, the padded pyramid's k_featpad ring); k_feat_split / k_feat_split16 write them when features are handed in.  pyramid + pdf
    = R1; the same features read back and handed in through set_level_features + pdf = R2; R1 == R2 bit for bit, every level and filter."""
    nf = 33
    m = make_tree_model([-1] + [0] * (nf - 1), 1, seed=41, sbin=sbin, interval=5)
    h = capi.Handle(m, conv_mode=mode)
    if pad:
        h.set_boundary_pad(pad)
    im = _frame(kind)
    h.pyramid(im) if im.dtype == np.uint8 else h.pyramid_image(im)
    h.pdf()
    g = h._geo
    levels = [l for l in range(g["nlevels"]) if g["cell_h"][l] and g["cell_w"][l]]
    assert len(levels) >= 5
    r1 = {l: np.stack([h.level_response(l, n) for n in range(nf)]) for l in levels}
    feats = {l: h.level_features(l) for l in levels}
    assert all(np.isfinite(r).all() for r in r1.values()) and max(float(np.abs(r).max()) for r in r1.values()) > 0.01
    for l in levels:
        h.set_level_features(l, feats[l])
    h.pdf()
    for l in levels:
        for n in range(nf):
            r2 = h.level_response(l, n)
            assert np.array_equal(r1[l][n], r2), f"level {l} filter {n} " + _first_difference(r2, r1[l][n].astype(np.float64))
    h.close()


# ---- the binary16 bank's domain -----------------------------------------------------------------------------------------------------
def test_binary16_domain_bound(gpu_required):
    """PBD_CONV_SPLIT_F16 carries f 2^12 in binary16, which rounds to inf from 65520 on: f = 65520 / 4096 = 15.99609375 and nextafter(16, 0)
    are refused (PBD_ERR_ARG, nothing uploaded: the next pdf returns the previous features' responses); nextafter(15.99609375, 0) is accepted
    and a delta filter of weight 2^k returns the two parts' sum x 2^k — here exactly 15.99609375 x 2^k — finite."""
    nf = 16
    sizes = [(5, 5)] * nf
    filters = []
    for n in range(nf):
        f = np.zeros((5, 5, X.FLEN), np.float32)
        f[2, 2, (5 * n + 3) % X.FLEN] = np.float32((-1.0) ** n * 2.0 ** (n % 10 - 6))
        filters.append(f.reshape(5, 5 * X.FLEN))
    h = capi.Handle(_model(filters), conv_mode=capi.PBD_CONV_SPLIT_F16)
    h.begin_frame(64, 48, 3)
    g = h._geo
    rng = np.random.default_rng(8)
    base = [X._full(rng, (int(ch), int(cw), X.FLEN), -3, -1, "f16") for ch, cw in zip(g["cell_h"], g["cell_w"])]
    for l, f in enumerate(base):
        h.set_level_features(l, f)
    h.pdf()
    r0 = [np.stack([h.level_response(l, n) for n in range(nf)]) for l in range(len(base))]
    for l, f in enumerate(base):
        assert np.array_equal(r0[l].astype(np.float64), X.ref_pdf(f, filters, sizes))
    edge = np.float32(65520.0 / 4096.0)
    for bad in (edge, -edge, np.nextafter(np.float32(16), np.float32(0)), np.float32(16)):
        f = base[0].copy()
        f[1, 2, 7] = bad
        with pytest.raises(capi.PbdError) as e:
            h.set_level_features(0, f)
        assert e.value.code == capi.PBD_ERR_ARG, bad
    h.pdf()
    for l in range(len(base)):
        assert np.array_equal(np.stack([h.level_response(l, n) for n in range(nf)]), r0[l])      # nothing was uploaded
    ok = np.nextafter(edge, np.float32(0))
    f = base[0].copy()
    f[1, 2, :] = ok
    f[2, 3, :] = -ok
    h.set_level_features(0, f)
    h.pdf()
    hi, lo, rest = split2_f16(np.array([ok], np.float32), 12)
    carried = (hi.astype(np.float64) + lo.astype(np.float64))[0] / 4096.0           # the 22 bits the two parts hold
    assert carried == 15.99609375 and abs(rest[0]) <= 2.0 ** -8
    for n in range(nf):
        w = float(filters[n].max() + filters[n].min())
        got = h.level_response(0, n)
        assert np.isfinite(got).all()
        assert got[1, 2] == np.float32(carried * w) and got[2, 3] == np.float32(-carried * w), (n, got[1, 2], carried * w)
    h.close()
