"""numpy restatement of include/pbd_c.h "virtual positives": matlab/learning/map_rotate_points.m:21-46 and the image operation that
belongs to it, written from the definition and the .m file.  math.cos / math.sin are the library's libm (numpy's vectorised cos may
differ in the last bit); every array operation below is one float64 IEEE operation per element, in the definition's order."""
import math

import numpy as np

ORI2NEW, NEW2ORI = 0, 1
NEAREST, BILINEAR = 0, 1


def geometry(w, hgt, deg):
    """-> (canvas rows, canvas cols, m = (c, s, hiA_r, hiA_c, hiB_r, hiB_c))"""
    phi = (float(deg) * math.pi) / 180.0
    c, s = math.cos(phi), math.sin(phi)
    hiA_r, hiA_c = (hgt - 1) / 2.0, (w - 1) / 2.0
    loA_r = -hiA_r
    # the forward map of (row, col) = (u, v) is (u*c - v*s, u*s + v*c); the file's corners are (loA_r, hiA_c) and (hiA_r, hiA_c)
    rr = max(abs(loA_r * c - hiA_c * s), abs(hiA_r * c - hiA_c * s))
    cc = max(abs(loA_r * s + hiA_c * c), abs(hiA_r * s + hiA_c * c))
    hiB_r, hiB_c = math.ceil(rr / 2.0) * 2.0, math.ceil(cc / 2.0) * 2.0
    return int(2 * hiB_r + 1), int(2 * hiB_c + 1), (c, s, hiA_r, hiA_c, hiB_r, hiB_c)


def map_points(pts, w, hgt, deg, direction):
    """rows (x, y) -> rows (x, y), float64"""
    _, _, (c, s, hiA_r, hiA_c, hiB_r, hiB_c) = geometry(w, hgt, deg)
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    if direction == ORI2NEW:
        u, v = y - hiA_r, x - hiA_c
        return np.stack([(u * s + v * c) + hiB_c, (u * c - v * s) + hiB_r], axis=1)
    u, v = y - hiB_r, x - hiB_c
    return np.stack([(v * c - u * s) + hiA_c, (u * c + v * s) + hiA_r], axis=1)


def flip_points(pts, w, mirror=None):
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    src = p if mirror is None else p[np.asarray(mirror)]
    return np.stack([float(w - 1) - src[:, 0], src[:, 1]], axis=1)


def _taps(F, y, x):
    """F[y][x] as float64 [rows, cols, cn] with 0.0 outside the source"""
    hgt, w = F.shape[:2]
    ok = (y >= 0) & (y < hgt) & (x >= 0) & (x < w)
    v = F[np.clip(y, 0, hgt - 1), np.clip(x, 0, w - 1)].astype(np.float64)
    return np.where(ok[..., None], v, 0.0)


def augment(im, flip, deg, method=BILINEAR):
    """one op on an HxW or HxWxcn uint8 frame: the mirror first, then the rotation (deg None: none)"""
    a = np.asarray(im, np.uint8)
    F = a.reshape(a.shape[0], a.shape[1], -1)
    if flip:
        F = F[:, ::-1]
    if deg is None:
        return np.ascontiguousarray(F).reshape(a.shape)
    hgt, w = F.shape[:2]
    rows, cols, (c, s, hiA_r, hiA_c, hiB_r, hiB_c) = geometry(w, hgt, deg)
    u = (np.arange(rows, dtype=np.float64) - hiB_r)[:, None]
    v = (np.arange(cols, dtype=np.float64) - hiB_c)[None, :]
    sr = (u * c + v * s) + hiA_r
    sc = (v * c - u * s) + hiA_c
    if method == NEAREST:
        out = _taps(F, np.floor(sr + 0.5).astype(np.int64), np.floor(sc + 0.5).astype(np.int64)).astype(np.uint8)
    else:
        fy0, fx0 = np.floor(sr), np.floor(sc)
        fy, fx = (sr - fy0)[..., None], (sc - fx0)[..., None]
        y0, x0 = fy0.astype(np.int64), fx0.astype(np.int64)
        a00, a01, a10, a11 = _taps(F, y0, x0), _taps(F, y0, x0 + 1), _taps(F, y0 + 1, x0), _taps(F, y0 + 1, x0 + 1)
        val = (1.0 - fy) * ((1.0 - fx) * a00 + fx * a01) + fy * ((1.0 - fx) * a10 + fx * a11)
        out = np.minimum(255.0, np.floor(val + 0.5)).astype(np.uint8)
    return out if a.ndim == 3 else out[:, :, 0]


# the grid of tests/test_augment_cpu.py and tests/test_gpu_augment.py
ANGLES = [0.0, 7.5, -7.5, 15.0, -15.0, 45.0, 90.0, -90.0, 180.0, 360.0]
SIZES = [(37, 29), (40, 30), (640, 480), (5, 5), (1, 1)]      # (w, hgt)
FRAMES = [(37, 29, 3), (40, 30, 1)]                           # (w, hgt, cn) of the image cases


def frame(w, hgt, cn, seed=7):
    rng = np.random.default_rng(seed + w)
    return rng.integers(0, 256, (hgt, w) if cn == 1 else (hgt, w, cn), dtype=np.uint8)


def grid_specs():
    """flip alone, each angle with both methods, flip plus 15 degrees: (flip, deg, method) as capi.augment_ops takes them"""
    return [(True, None, BILINEAR)] + [(False, d, m) for d in ANGLES for m in (NEAREST, BILINEAR)] + [(True, 15.0, NEAREST), (True, 15.0, BILINEAR)]


def padded(im, pad=5, fill=0xA5):
    """a strided view of `im` inside rows `pad` bytes longer"""
    a = np.asarray(im)
    hgt, w = a.shape[:2]
    cn = 1 if a.ndim == 2 else a.shape[2]
    buf = np.full((hgt, w * cn + pad), fill, np.uint8)
    buf[:, :w * cn] = a.reshape(hgt, w * cn)
    return buf[:, :w * cn].reshape(a.shape)


def cpp_check(tmp_path, lib_dir, route):
    """build and run tests/tools/augment_check.cpp on a 41 x 31 x 3 frame -> (frame, its output lines as {first word: the rest})"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "augment_check"
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-o", str(exe), os.path.join(root, "tests", "tools", "augment_check.cpp"),
                           "-L" + lib_dir, "-lpbd_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    im = frame(41, 31, 3)
    im.tofile(str(tmp_path / "frame.bin"))
    out = subprocess.run([str(exe), str(tmp_path / "frame.bin"), "41", "31", "3", route], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    return im, dict(l.split(" ", 1) for l in out.stdout.splitlines())


def cpp_expect(im, lines, augment_host, map_points_fn, flip_points_fn):
    """the lines of cpp_check against the binding's host functions"""
    specs = [(True, None, NEAREST), (False, 15.0, BILINEAR), (True, -7.5, NEAREST), (False, 90.0, BILINEAR)]
    for i, want in enumerate(augment_host(im, specs)):
        h = 1469598103934665603
        for b in want.tobytes():
            h = ((h ^ b) * 1099511628211) & (2 ** 64 - 1)
        assert lines[f"op{i}"].split() == [str(want.shape[0]), str(want.shape[1]), str(h)], i
    pts = [[3.0, 4.0], [20.5, 11.25]]
    fwd = map_points_fn(pts, 41, 31, 15.0, ORI2NEW)
    assert [float.fromhex(v) for v in lines["fwd"].split()] == fwd.ravel().tolist()
    assert [float.fromhex(v) for v in lines["back"].split()] == map_points_fn(fwd, 41, 31, 15.0, NEW2ORI).ravel().tolist()
    assert [float.fromhex(v) for v in lines["mir"].split()] == flip_points_fn(pts, 41, [1, 0]).ravel().tolist()
    assert lines["refused"].startswith("1 ") and "unknown method" in lines["refused"] and lines["writeWarped_dev"] == "1"
