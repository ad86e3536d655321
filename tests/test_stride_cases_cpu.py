"""The strided cases of tests/stride_cases.py are what tests/test_gpu_strides.py takes them for, and the bindings hand them over in
place: record counts from the oracle, views equal to their packed copies, padding that differs between the two fills, and
capi._frame / capi._depth_image returning (the view itself, strides[0]) for every layout and today's arguments for packed input."""
import numpy as np
import pytest

from partsbaseddetector_amd import capi
from tests import stride_cases as sc


@pytest.fixture(scope="module")
def frames():
    return sc.all_frames()


def test_oracle_record_counts(orc, frames):
    m = sc.model()
    m.thresh = sc.threshold(orc, m, frames)
    extra = {f"batch{i}": f for i, f in enumerate(sc.batch_frames())}
    extra.update({f"graph{i}": f for i, f in enumerate(sc.graph_frames())})
    for name, im in {**frames, **extra}.items():
        n = len(orc.detect(m, im)[0])
        assert sc.MIN_RECORDS <= n <= sc.MAX_RECORDS, (name, n)


def _layouts(name):
    return sc.WIDE_LAYOUTS if name in sc.WIDE else sc.LAYOUTS


def _row_bytes(a):
    return a.shape[1] * (1 if a.ndim == 2 else a.shape[2]) * a.itemsize


def test_frame_sizes_take_both_copy_branches(frames):
    assert _row_bytes(frames["bgr101x77"]) == 303 and _row_bytes(frames["bgr100x75"]) == 300 and frames["grey90x70"].ndim == 2
    assert [frames[k].dtype for k in sc.WIDE] == [np.uint16, np.float32, np.float64]


@pytest.mark.parametrize("name", list(sc.FRAMES) + list(sc.WIDE))
def test_views_hold_the_frame_and_only_the_padding_differs(frames, name):
    im = frames[name]
    row = _row_bytes(im)
    for layout in _layouts(name):
        views = [sc.embed(im, layout, fill) for fill in sc.FILLS]
        for view, parent in views:
            assert view.shape == im.shape and view.dtype == im.dtype and not view.flags["C_CONTIGUOUS"]
            assert np.ascontiguousarray(view).tobytes() == im.tobytes(), (name, layout)
            assert view.strides[0] > row and view.strides[0] % im.itemsize == 0
            assert np.shares_memory(view, parent)
            end = sc.offset_of(view, parent) + (im.shape[0] - 1) * view.strides[0] + row
            assert end <= parent.size
            if layout == "tail":
                assert end == parent.size        # the buffer ends with the last pixel of the last row
        pads = [sc.padding_bytes(v, p) for v, p in views]
        assert pads[0].size == pads[1].size > 0 and (pads[0] != pads[1]).mean() > 0.9, (name, layout)
    if name in sc.FRAMES:
        cn = 1 if im.ndim == 2 else im.shape[2]
        v = {l: sc.embed(im, l, sc.FILLS[0])[0] for l in sc.LAYOUTS}
        assert v["pad1"].strides[0] == row + 1 and v["pad3"].strides[0] == row + 3 and v["pitch512"].strides[0] == 512
        assert (v["pad1"].strides[0] % 2 == 1) == (row % 2 == 0)                          # 301 and 91 are odd strides; 303 + 1 is not
        assert any(x.strides[0] % 4 for x in v.values())                                  # rows that do not start on a word
        assert v["roi"].strides[0] == 320 * cn and v["roi"].ctypes.data % 4 != 0          # (960 for BGR) an unaligned base
    else:
        assert sc.embed(im, "pad1", sc.FILLS[0])[0].strides[0] == row + im.itemsize


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_depth_views(dtype):
    for dname, d in sc.depth_images(101, 77, dtype).items():
        for layout in sc.DEPTH_LAYOUTS:
            views = [sc.embed_depth(d, layout, fill) for fill in sc.FILLS]
            for view, parent in views:
                assert np.ascontiguousarray(view).tobytes() == d.tobytes() and not view.flags["C_CONTIGUOUS"]
                pad = sc.padding_bytes(view, parent).view(dtype)
                assert np.isnan(pad).any() and (pad == 0).any() and (pad == 1e6).any()     # values that would move a median
            pads = [sc.padding_bytes(v, p).view(f"u{d.itemsize}") for v, p in views]   # (bit patterns: NaN compares as itself)
            assert (pads[0] != pads[1]).mean() > 0.5, (dname, layout)                  # three values: two of three elements differ
            a, stride = capi._depth_image(views[0][0], dtype)
            assert a is views[0][0] and stride == a.strides[0]
        a, stride = capi._depth_image(d, dtype)                       # packed: today's arguments
        assert a is d and stride == d.shape[1] * d.itemsize
        a, stride = capi._depth_image(d.astype(np.float16), dtype)    # another dtype: converted, packed
        assert a.dtype == dtype and a.flags["C_CONTIGUOUS"] and stride == d.shape[1] * d.itemsize


@pytest.mark.parametrize("name", list(sc.FRAMES) + list(sc.WIDE))
def test_bindings_pass_views_in_place(frames, name):
    im = frames[name]
    dt = None if name in sc.WIDE else np.uint8
    hgt, w = im.shape[:2]
    cn = 1 if im.ndim == 2 else im.shape[2]
    for layout in _layouts(name):
        view, parent = sc.embed(im, layout, sc.FILLS[0])
        a, aw, ah, acn, stride = capi._frame(view, dt)
        assert a is view and (aw, ah, acn) == (w, hgt, cn), (name, layout)
        assert a.ctypes.data == parent.ctypes.data + sc.offset_of(view, parent) and stride == view.strides[0]
    a, aw, ah, acn, stride = capi._frame(im, dt)                       # packed: the array itself, stride w * cn * itemsize
    assert a is im and (aw, ah, acn, stride) == (w, hgt, cn, w * cn * im.itemsize)


def test_bindings_copy_what_is_not_rows(frames):
    im = frames["bgr101x77"]
    row = 303
    for bad in (im[:, ::2], im[:, :, ::2], im[::-1], im[:, :, ::-1], np.broadcast_to(im[0], im.shape)):
        a, w, hgt, cn, stride = capi._frame(bad)
        assert a.flags["C_CONTIGUOUS"] and a is not bad and np.array_equal(a, bad) and stride == w * cn
    a, _, _, _, stride = capi._frame(im[::2])                          # every other row: rows, 606 bytes apart
    assert a.base is im and stride == 2 * row
    a, _, _, _, stride = capi._frame(im.astype(np.int32))              # another dtype: converted, packed
    assert a.dtype == np.uint8 and stride == row and np.array_equal(a, im)
    a, w, hgt, cn, stride = capi._frame(im.tolist())
    assert a.dtype == np.uint8 and (w, hgt, cn, stride) == (101, 77, 3, row)


def test_batches_share_one_stride(frames):
    im = frames["bgr100x75"]
    hgt, w = im.shape[:2]
    parent = np.random.default_rng(5).integers(0, 256, (240, 320, 3), dtype=np.uint8)
    rois = [parent[y:y + hgt, x:x + w] for x, y in ((7, 5), (121, 3), (9, 101), (215, 160))]
    got, stride = capi._frames(rois)
    assert stride == 960 and all(g is r for g, r in zip(got, rois))
    mixed = rois[:3] + [sc.embed(im, "pad1", 1)[0]]
    got, stride = capi._frames(mixed)                                   # two strides: every frame copied
    assert stride == 300 and all(g.flags["C_CONTIGUOUS"] and np.array_equal(g, m) for g, m in zip(got, mixed))
    packed = [np.ascontiguousarray(r) for r in rois]
    got, stride = capi._frames(packed)
    assert stride == 300 and all(g is p for g, p in zip(got, packed))
