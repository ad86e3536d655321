"""Strided frames and depth images, shared by tests/test_stride_cases_cpu.py and tests/test_gpu_strides.py: every frame embedded in a
larger parent buffer of seeded noise — rows padded by 1 and by 3 bytes, a 512-byte pitch, an ROI at an odd (x0, y0) of a 320 x 240
parent (base pointer not 4-byte aligned), and a buffer that ends with the last pixel of the last row — under two different fills of
the parent.  What a view holds is the frame, bit for bit; what lies between its rows must never reach a result.

Sizes: 101 x 77 x 3 has 303-byte rows (odd: the byte tail of the word-wise level-0 copy runs), 100 x 75 x 3 has 300 (a multiple
of 4: no tail), 90 x 70 is grey.  Nothing is read from files."""
import numpy as np

from partsbaseddetector_amd.model import make_image, make_tree_model, make_wide_image
from tests.test_gpu_cluster3d import CAM, rgbd_scene          # noqa: F401  (the RGB-D tests' fixtures, at these frames' size)
from tests.test_gpu_depth_filter import scene

FRAMES = {"bgr101x77": (101, 77, 3, 21), "bgr100x75": (100, 75, 3, 22), "grey90x70": (90, 70, 1, 23)}   # name: (w, hgt, cn, seed)
WIDE = {"u16": np.uint16, "f32": np.float32, "f64": np.float64}                                          # 101 x 77 x 3, seed 24
LAYOUTS = ("pad1", "pad3", "pitch512", "roi", "tail")
WIDE_LAYOUTS = ("pad1", "pitch512")           # pad1: one ELEMENT per row
DEPTH_LAYOUTS = ("pad1", "pitch512", "roi")
OPTION_LAYOUTS = ("pad1", "roi")              # what options (pyramid kind, graph, scalar type) are crossed with
FILLS = (101, 202)
PARENT_W, PARENT_H, ROI_X0, ROI_Y0 = 320, 240, 7, 5
TAIL_PAD = 5
MIN_RECORDS, MAX_RECORDS = 20, 1000
QUANTILE = 97.0


def model():
    """the tree model of the pyramid tests"""
    return make_tree_model([-1, 0, 1, 1, 0], 3, seed=5, sbin=4, interval=5)


def frame(name):
    w, hgt, cn, seed = FRAMES[name]
    return make_image(seed, w, hgt, cn)


def wide_frame(kind):
    return make_wide_image(WIDE[kind], 24, 101, 77)


def all_frames():
    """{name: packed frame}: the three 8-bit frames and the three wide ones"""
    out = {n: frame(n) for n in FRAMES}
    out.update({k: wide_frame(k) for k in WIDE})
    return out


def batch_frames(cn=3):
    """four different 100 x 75 frames: the batches' (the last two also go with the RGB-D frame)"""
    return [make_image(s, 100, 75, cn) for s in (60, 61, 62, 80)]


def graph_frames():
    """three different 101 x 77 frames for consecutive calls on a graph handle"""
    return [make_image(s, 101, 77) for s in (70, 71, 72)]


def threshold(orc, m, frames=None):
    """one threshold for every frame (the handles are shared), chosen with the oracle as tests.util.thresh_from_oracle does: the
    smallest of the frames' QUANTILE-th percentiles of the root scores, so every frame keeps at least its top 3 %"""
    from tests.util import thresh_from_oracle
    frames = all_frames() if frames is None else frames
    return min(thresh_from_oracle(orc, m, im, QUANTILE) for im in frames.values())


def _noise(fill, nbytes):
    return np.random.default_rng(fill).integers(0, 256, nbytes, dtype=np.uint8)


def _rows_view(parent, offset, shape, dtype, stride):
    isz = np.dtype(dtype).itemsize
    cn = 1 if len(shape) == 2 else shape[2]
    strides = (stride, isz) if len(shape) == 2 else (stride, cn * isz, isz)
    return np.ndarray(shape, dtype, buffer=parent, offset=offset, strides=strides)


def _geometry(shape, isz, layout):
    """(parent bytes, offset of the view, stride) of a frame of `shape` and element size isz under `layout`"""
    hgt, w = shape[:2]
    cn = 1 if len(shape) == 2 else shape[2]
    row = w * cn * isz
    if layout == "pad1":
        stride = row + isz
    elif layout == "pad3":
        stride = row + 3 * isz
    elif layout == "pitch512":
        stride = (row + 511) // 512 * 512
    elif layout == "roi":
        stride = PARENT_W * cn * isz
        return PARENT_H * stride, ROI_Y0 * stride + ROI_X0 * cn * isz, stride
    elif layout == "tail":
        stride = row + TAIL_PAD * isz
        return (hgt - 1) * stride + row, 0, stride
    else:
        raise ValueError(layout)
    return hgt * stride, 0, stride


def embed(im, layout, fill):
    """(view, parent): `im` written into a parent buffer (1-D uint8) of seeded noise under `layout`; the view is a numpy array of
    im's shape and dtype over the parent, with strides[0] = the layout's stride"""
    nbytes, offset, stride = _geometry(im.shape, im.itemsize, layout)
    parent = _noise(fill, nbytes)
    view = _rows_view(parent, offset, im.shape, im.dtype, stride)
    view[...] = im
    return view, parent


def depth_images(w, hgt, dtype):
    """the existing RGB-D tests' scenes at w x hgt"""
    return {"planes": scene(3, w, hgt, dtype), "blobs": rgbd_scene(4, w, hgt, dtype)}


def embed_depth(depth, layout, fill):
    """embed() for a depth image: the parent holds values that would move a median — NaN, 0 and 1e6 —, chosen by the fill"""
    nbytes, offset, stride = _geometry(depth.shape, depth.itemsize, layout)
    vals = np.array([np.nan, 0.0, 1e6], depth.dtype)
    pv = vals[np.random.default_rng(fill).integers(0, 3, nbytes // depth.itemsize)]
    parent = np.zeros(nbytes, np.uint8)
    parent[:pv.nbytes] = pv.view(np.uint8)
    view = _rows_view(parent, offset, depth.shape, depth.dtype, stride)
    view[...] = depth
    return view, parent


def padding_bytes(view, parent):
    """the parent's bytes outside the view's pixels"""
    mask = np.ones(parent.size, bool)
    off = view.ctypes.data - parent.ctypes.data
    row = view.shape[1] * (1 if view.ndim == 2 else view.shape[2]) * view.itemsize
    for y in range(view.shape[0]):
        mask[off + y * view.strides[0]: off + y * view.strides[0] + row] = False
    return parent[mask]


def offset_of(view, parent):
    return view.ctypes.data - parent.ctypes.data
