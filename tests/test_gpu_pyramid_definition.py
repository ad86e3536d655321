"""The first-stage KERNELS (k_pyramid.hip, k_hog.hip) against the definitions of tests/hog_ref.py / tests/pyramid_ref.py and the recorded
output of the compiled reference HOG (tests/golden/ref_hog_v1.npz) — directly, not through oracle/.  Same frames, same derived bounds as
tests/test_pyramid_definition_cpu.py (hog_ref.float_bound, pyramid_ref.*_bound, pyramid_checks.F64_TOL); every check prints its figure.
Wide depths reach the device through pbd_pyramid_image / pbd_detect_image (there is no 16-bit / float entry point of the single
primitives), so their HOG, resize and pyrDown are checked level by level on the device's own level images.  Planes a detect call left
behind — a batch's included — are read with Handle.frame_planes (pbd_get_frame_level_*)."""
import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.model import make_image, make_person_model, make_tree_model, make_wide_image
from tests import boundary_pad_ref as bp
from tests.hog_ref import hog_def
from tests.pyramid_cases import (GOLDEN, PYRDOWN_SIZES, RESIZE_CASES, WIDE_DETECT_FRAME, fixture_frames, hog_frames_u8, hog_frames_wide, noise,
                                 pyramid_resize_cases)
from tests.pyramid_checks import F64_TOL, check_geometry, check_hog, check_pyrdown, check_resize
from tests.pyramid_ref import geometry_def

pytestmark = pytest.mark.gpu
TREE = [-1, 0, 1, 1, 0]
T_IDS = ["T_float", "T_double"]


def tree(sbin, interval=5):
    m = make_tree_model(TREE, 3, seed=5, sbin=sbin, interval=interval)
    m.thresh = 1e9           # no candidates: these tests read stages, not detections
    return m


def check_pyramid(h, im, model, label, frame=0):
    """EVERY level of the pyramid the handle's current plan holds for `im` (frame `frame` of the plan): geometry == geometry_def; level
    image vs resize_def of the frame (levels below `interval`) or pyrdown_def of the DEVICE's own level l - interval (so errors do
    not stack); level features vs hog_def of the device's own level image."""
    hgt, w = im.shape[:2]
    cn = 1 if im.ndim == 2 else im.shape[2]
    g = h.geometry(w, hgt)
    check_geometry(g, geometry_def(w, hgt, model.sbin, model.interval), label)
    planes = [h.frame_planes(frame, l, w, hgt, cn, im.dtype) for l in range(g["nlevels"])]
    for l, (raw, feat) in enumerate(planes):
        if l < model.interval:
            check_resize(raw, im, f"{label} level {l}")
        else:
            check_pyrdown(raw, planes[l - model.interval][0], f"{label} level {l}")
        check_hog(feat, raw, model.sbin, f"{label} level {l}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=T_IDS)
@pytest.mark.parametrize("sbin", [4, 8])
def test_hog_kernel_u8_vs_definition(gpu_required, sbin, dtype):
    """pbd_hog_u8 / pbd_hog_u8_f64 on every 8-bit frame of the CPU file, nothing excluded"""
    h = capi.Handle(tree(sbin), conv_mode=capi.PBD_CONV_EXACT, dtype=dtype)
    worst = 0.0
    for name, im, s in hog_frames_u8():
        if s != sbin:
            continue
        want = hog_def(im, s, details=True)
        try:
            got = h.hog(im)
        except capi.PbdError as e:
            assert want[0].size == 0, (name, str(e))        # only a frame without output cells may be refused by the entry point
            print(f"[hog] {name}: refused by the entry point ({e})")
            continue
        worst = max(worst, check_hog(got, im, s, name, ref=want))
    print(f"[hog kernel] sbin {sbin} {np.dtype(dtype).name}: worst over all frames {worst:.3e}")
    h.close()


def test_hog_kernel_double_vs_recorded_reference(gpu_required):
    """the device against compiled reference output with nothing of ours in between: <= 1e-12.  8-bit frames through pbd_hog_u8_f64, the
    two wide frames through pbd_pyramid_image on an interval-1 model (level 0 is the frame itself)."""
    gold = np.load(GOLDEN)
    hs = {s: capi.Handle(tree(s), conv_mode=capi.PBD_CONV_EXACT, dtype=np.float64) for s in (4, 8)}
    h1 = capi.Handle(tree(4, interval=1), conv_mode=capi.PBD_CONV_EXACT, dtype=np.float64)
    for name, im, sbin in fixture_frames():
        if im.dtype == np.uint8:
            got = hs[sbin].hog(im)
        else:
            h1.pyramid_image(im)
            assert np.array_equal(h1.level_image_raw(0), im)
            got = h1.level_features(0)
        worst = float(np.abs(got - gold[name]).max())
        print(f"[kernel f64 vs fixture] {name}: {worst:.3e}")
        assert got.shape == gold[name].shape and worst <= F64_TOL, (name, worst)
    for h in list(hs.values()) + [h1]:
        h.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=T_IDS)
@pytest.mark.parametrize("sbin", [4, 8])
def test_resize_and_pyrdown_kernels_u8_vs_definition(gpu_required, sbin, dtype):
    h = capi.Handle(tree(sbin), conv_mode=capi.PBD_CONV_EXACT, dtype=dtype)
    for w, hgt in PYRDOWN_SIZES:
        for cn in (1, 3):
            im = np.ascontiguousarray(make_image(31, max(w, 4), max(hgt, 4), cn)[:hgt, :w])
            check_pyrdown(h.pyrdown(im), im, f"{w}x{hgt}x{cn}")
    cases = RESIZE_CASES + pyramid_resize_cases(640, 480, 4, 10) + pyramid_resize_cases(200, 150, 8, 5)
    for w, hgt, ow, oh in cases:
        im = make_image(32, w, hgt, 3 if (w + ow) % 2 else 1)
        check_resize(h.resize(im, ow, oh), im, "image")
    for w, hgt, ow, oh in cases[:4]:
        check_resize(h.resize(noise(9, w, hgt), ow, oh), noise(9, w, hgt), "noise")
    h.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=T_IDS)
def test_wide_depths_through_the_pyramid_vs_definition(gpu_required, dtype):
    """16-bit, float and double frames: every level's image (resize / pyrDown) and features against the definitions"""
    hs = {s: capi.Handle(tree(s), conv_mode=capi.PBD_CONV_EXACT, dtype=dtype) for s in (4, 8)}
    for name, im, sbin in hog_frames_wide():
        hs[sbin].pyramid_image(im)
        check_pyramid(hs[sbin], im, hs[sbin].model, name)
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("case", ["640x480_float", "640x480_double", "1920x1080_float"])
def test_person_pyramid_every_level_vs_definition(gpu_required, case):
    size, t = case.split("_")
    w, hgt = (int(v) for v in size.split("x"))
    model = make_person_model(K=6)
    model.thresh = 1e9
    im = make_image(3, w, hgt)
    h = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=np.float32 if t == "float" else np.float64)
    h.pyramid(im)
    check_pyramid(h, im, model, case)
    h.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=T_IDS)
@pytest.mark.parametrize("graph", [0, 1], ids=["eager", "graph_replay"])
def test_batch_path_features_vs_definition(gpu_required, graph, dtype):
    """4 different frames through pbd_detect_batch_u8 (eager; and the replay of the captured graph): what the batched launches of
    k_pyramid / k_hog wrote for EACH frame — every level's image and features, read back from the batch plan — is the definition."""
    model = tree(4, interval=10)
    frames = [make_image(40 + i, 320, 240) for i in range(4)]
    h = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, graph=graph, dtype=dtype)
    for _ in range(2 if graph else 1):          # graph: the second call replays what the first captured
        h.detect_batch(frames, 16)
    assert h.stage_state()["features"]
    for f, fr in enumerate(frames):
        check_pyramid(h, fr, model, f"batch graph={graph} frame {f}", frame=f)
    with pytest.raises(capi.PbdError):
        h.frame_planes(4, 0, 320, 240)          # a frame the plan does not have
    h.close()


def test_device_resident_sixteen_bit_and_padded_paths_vs_definition(gpu_required):
    import torch
    model = tree(4, interval=10)
    w, hgt = 320, 240
    im = make_image(50, w, hgt)
    # detect_dev: the frame already in device memory
    h = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT)
    dev = torch.from_numpy(im).cuda()
    h.detect_dev(dev.data_ptr(), w, hgt, 3, capacity=16)
    assert h.stage_state()["features"]
    check_pyramid(h, im, model, "detect_dev")
    # detect_image with a 16-bit frame: every level
    seed, w16, h16 = WIDE_DETECT_FRAME
    im16 = make_wide_image(np.uint16, seed, w16, h16)
    h.detect_image(im16, 16)
    assert h.stage_state()["features"]
    check_pyramid(h, im16, model, "detect_image 16-bit")
    h.close()
    # boundary padding: the interior of the padded planes is the definition, the ring is boundary_pad_ref's rule
    for dtype in (np.float32, np.float64):
        hp = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dtype)
        hp.set_boundary_pad(3)
        hp.pyramid(im)
        for l in range(hp.geometry(w, hgt)["nlevels"]):
            padded, raw = hp.level_features(l), hp.level_image_raw(l)
            if padded.size == 0:
                continue
            inner = np.ascontiguousarray(padded[3:-3, 3:-3])
            check_hog(inner, raw, model.sbin, f"padded {np.dtype(dtype).name} level {l}")
            assert np.array_equal(padded, bp.pad_features(inner, 3)), l
        hp.close()
