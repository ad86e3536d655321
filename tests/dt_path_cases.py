"""Named inputs that drive k_dt_pass (partsbaseddetector_amd/csrc/k_dp.hip) through its rare paths, shared by
tests/test_dt_paths_cpu.py (the host replay, tests/tools/dt_replay.cpp) and tests/test_gpu_dt_paths.py (the product library
against the oracle, and the probe build's path counters, pbd_debug_dt_counters, in a fresh child process).

A case names the paths it must reach, by counter name (COUNTERS: the probe build's eight, in its order).  dt2d cases run
pbd_dt2d (x then y pass); fold cases run the fold DP (set_level_response + dp_min) on a model with weak dyadic curvatures.

RANGE_CASES leave the usual magnitudes (values up to 3e38 and down to subnormals, curvatures from 1e-310 to 1e300), all finite.

Child mode (`python -m tests.dt_path_cases NAME`, PBD_LIBRARY = the probe build): runs one case, checks it against the oracle
and prints one JSON line {"case", "rc", "counters", "match"}.  `--replay-child SO KIND DTYPE MODE`: see replay_child_main."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partsbaseddetector_amd", "csrc")
COUNTERS = ["round_blocks", "rounds", "max_rounds", "stitch_redos", "fnew_stale", "scan_flags", "stitch_flags", "seq_redos"]
# host replay only: lines flagged inside a REDONE stitch, stitch flags for a lost invariant / a suspect quotient, blocks, lines,
# groups (of the two passes) the planner gave the fused arithmetic
HOST_COUNTERS = COUNTERS + ["redo_flags", "lost_invariants", "stitch_suspects", "blocks", "lines", "fused_groups"]
F32 = lambda v: float(np.float32(v))   # noqa: E731  a weight that is a converted float (the fused arithmetic's promise)
NOT_F32 = 1 + 2.0 ** -40               # a factor that makes any weight a double that is not a converted float (unfused)


def _smooth(rows, cols, seed, dtype=np.float32, q=0.0):
    """slow sine plus a little noise, with a dominant peak at the left end of every line: weak curvature makes that peak
    reach over many segments, so the speculative stitches walk to their neighbour's F (stale) and rounds follow one another"""
    r = np.random.default_rng(seed)
    a = np.sin(np.arange(cols) / 9.0)[None, :] * 0.5 + r.normal(0, 0.02, (rows, cols))
    if q:
        a = np.round(a / q) * q
    a[:, :3] += 8.0
    return a.astype(dtype)


def _ints(rows, cols, seed, dtype=np.float32):
    """small integers: with power-of-two curvatures, intersections land exactly on float rounding boundaries (suspect quotients)"""
    return np.round(np.random.default_rng(seed).normal(0, 1.5, (rows, cols))).astype(dtype)


def _plateaus(rows, cols, seed, dtype=np.float32):
    """runs of four equal small integers"""
    r = np.random.default_rng(seed)
    return np.repeat(np.round(r.normal(0, 2, (rows, cols // 4 + 1))), 4, axis=1)[:, :cols].astype(dtype)


def _dt2d(name, make, ax, bx, ay, by, osx, osy, paths, fused, dtype=np.float32, min_rounds=0):
    return dict(name=name, kind="dt2d", make=make, q=(ax, bx, ay, by, osx, osy), paths=paths, fused=fused, dtype=np.dtype(dtype),
                min_rounds=min_rounds)


ROUNDS = ["round_blocks", "rounds", "max_rounds", "stitch_redos"]
FLAGS = ["scan_flags", "stitch_flags", "seq_redos"]
W = 0.0005
CASES = [
    # weak curvature: rounds behind rounds, boundaries stale only through their neighbour's new F
    _dt2d("smooth_f32_fused", lambda: _smooth(64, 256, 1), -F32(W), F32(0.001), -F32(W), -F32(0.001), 0, 0,
          ROUNDS + ["fnew_stale"], fused=2, min_rounds=3),
    _dt2d("smooth_f32_unfused", lambda: _smooth(64, 256, 1), -F32(W) * NOT_F32, F32(0.001), -F32(W), -F32(0.001) * NOT_F32, 0, 0,
          ROUNDS + ["fnew_stale"], fused=0, min_rounds=3),
    _dt2d("smooth_f32_long", lambda: _smooth(32, 500, 2), -F32(W), 0.0, -F32(0.002), 0.0, 1, -2, ROUNDS + ["fnew_stale"], fused=2,
          min_rounds=3),
    _dt2d("smooth_f64", lambda: _smooth(64, 256, 3, np.float64), -W, 0.001, -W, -0.001, 0, 0, ROUNDS + ["fnew_stale"], fused=0,
          dtype=np.float64, min_rounds=3),
    _dt2d("ints_f64", lambda: _ints(64, 256, 1, np.float64), -2.0 ** -10, 0.0, -2.0 ** -10, 0.0, 0, 0, ROUNDS + ["fnew_stale"],
          fused=0, dtype=np.float64, min_rounds=3),
    # quantised values, power-of-two curvatures: suspect quotients in local scans and in stitches, lines redone sequentially
    _dt2d("ints_f32", lambda: _ints(64, 256, 0), -2.0 ** -10, 0.0, -2.0 ** -10, 0.0, 0, 0, ROUNDS + FLAGS + ["fnew_stale"],
          fused=2, min_rounds=3),
    _dt2d("ints_f32_steep", lambda: _ints(40, 160, 0), -2.0 ** -4, 0.0, -2.0 ** -4, 0.0, 0, 0, FLAGS, fused=2),
    _dt2d("plateaus_f32_unfused", lambda: _plateaus(64, 256, 0), -2.0 ** -8, 0.0, -2.0 ** -8 * NOT_F32, 0.0, 0, 0,
          ROUNDS + ["scan_flags", "seq_redos"], fused=1),
    # a line flagged inside a REDONE stitch (found by the replay; host counter redo_flags)
    _dt2d("redo_flag_f32", lambda: _plateaus(40, 160, 0), -2.0 ** -12, 2.0 ** -7, -2.0 ** -12, -2.0 ** -7, 0, 0,
          ROUNDS + FLAGS + ["fnew_stale", "redo_flags"], fused=2),
    # around the u8 / u16 index switch (stride = (len + 1) | 1 > 256 from len 255 on)
    *[_dt2d(f"len{n}_f32", (lambda n=n: _smooth(24, n, n, q=0.25)), -F32(W), 0.0, -2.0 ** -6, 0.0, 2, -1,
            ROUNDS + ["scan_flags", "seq_redos"], fused=2) for n in (254, 255, 256, 257)],
    # offsets at the fused arithmetic's limit (len + |os| <= 16384)
    _dt2d("os_at_fuse_limit", lambda: _smooth(40, 200, 5), -F32(0.01), F32(0.003), -F32(0.01), F32(0.002), 16384 - 200, -(16384 - 40),
          [], fused=2),
    _dt2d("os_past_fuse_limit", lambda: _smooth(40, 200, 5), -F32(0.01), F32(0.003), -F32(0.01), F32(0.002), 16385 - 200, -(16385 - 40),
          [], fused=0),
    # beyond the limit (|os| up to 40 000: the reference squares the INT distance, which stays exact below 46 341), where fusing
    # the read-out's a * d^2 + b * d would change low bits
    _dt2d("os_40000", lambda: _smooth(40, 200, 6), -F32(0.01), F32(0.003), -F32(0.013), F32(0.002), 40000, -40000 + 41, [], fused=0),
    _dt2d("os_40000_f64", lambda: _smooth(40, 200, 7, np.float64), -0.01, 0.003, -0.013, 0.002, -40000 + 201, 40000 - 41, [],
          fused=0, dtype=np.float64),
]


# ---- fold cases: the DP's own distance transforms (set_level_response + dp_min) ----------------------------------------------
def fold_model(K, seed):
    """a tree with K mixtures per part whose deformations are weak: mixture 0 a power-of-two curvature (with the small-integer
    responses below: suspect quotients, flagged lines), the other mixtures curvatures that are not (unflagged lines of the same
    blocks), all weak enough for rounds"""
    from partsbaseddetector_amd.model import make_tree_model
    m = make_tree_model([-1, 0, 1, 1, 0], K, seed=seed)
    for d in range(len(m.defw)):
        k = d % K
        m.defw[d] = (2.0 ** -10, 0.0, 2.0 ** -9, 0.0) if k == 0 else (0.0007 * (k + 1), 0.001, 0.0011 * k, -0.001)
    m.defw = np.asarray(m.defw, np.float32)
    return m


FOLD_CASES = [
    dict(name="fold_f32_k3", kind="fold", K=3, seed=31, wh=(320, 240), dtype=np.dtype(np.float32), paths=ROUNDS + FLAGS, min_rounds=3),
    dict(name="fold_f32_k2", kind="fold", K=2, seed=32, wh=(400, 300), dtype=np.dtype(np.float32), paths=ROUNDS + FLAGS, min_rounds=3),
    dict(name="fold_f64_k3", kind="fold", K=3, seed=33, wh=(320, 240), dtype=np.dtype(np.float64), paths=ROUNDS, min_rounds=3),
]


# ---- range cases: the whole float range, finite ----------------------------------------------------------------------------
# dt_isect's EXACT = false path (float maps) promises: a quotient outside [2^-124, 2^128) in magnitude is flagged and the line redone with
# IEEE divisions; no intermediate under- or overflows unless the result itself leaves the float range; i2a = RN(1 / 2a) of a tiny,
# subnormal or not-a-float curvature is safe (an infinite or inexact reciprocal only ever flags).  These families leave |value| ~ 1,
# |a| in [1e-4, 1]: every one is FINITE (the distance transform's input domain) and each comes as a float and as a double map.  The
# float cases whose quotients must leave the float range name scan_flags; how many lines flag is the replay's to say
# (tests/test_gpu_dt_paths.py holds the GPU to the replay's count).
RANGE_SHAPE = (24, 200)
_QA = (-F32(0.01), F32(0.002), -F32(0.02), -F32(0.001))   # an ordinary pair of quadratics (converted floats)


def _normal(scale, seed, shape):
    return np.random.default_rng(seed).normal(0, 1.5, shape) * scale


def _range_family(shape):
    """[(family, make(dtype) -> map, (ax, bx, ay, by), paths of the float case)]: shared by RANGE_CASES (24 x 200) and the recorded
    subset of tests/golden/ref_dt_v1.npz (16 x 72)"""
    def tiny(seed):
        r = np.random.default_rng(seed)
        return r.normal(0, 1.5, shape) * np.where(r.random(shape) < 0.5, 1e-38, 1e-42)
    return [
        ("big_1e30", lambda: _normal(1e30, 101, shape), _QA, []),
        ("uniform_3e38", lambda: np.random.default_rng(102).uniform(-3e38, 3e38, shape), _QA, ["scan_flags"]),
        ("big_1e36_weak", lambda: _normal(1e36, 103, shape), (-F32(1e-4), 0.0, -F32(1e-4), 0.0), ["scan_flags"]),
        ("tiny_subnormal", lambda: tiny(104), _QA, []),
        ("a_1e-30_1e-38_float", lambda: _normal(1.0, 105, shape), (-F32(1e-30), 0.0, -F32(1e-38), 0.0), []),
        ("a_1e-300_1e-310_double", lambda: _normal(1.0, 106, shape), (-1e-300, 0.0, -1e-310, 0.0), ["scan_flags"]),
        ("a_1e30_1e20", lambda: _normal(1.0, 107, shape), (-F32(1e30), 0.0, -F32(1e20), 0.0), []),
        ("a_1e300", lambda: _normal(1.0, 108, shape), (-1e300, 0.0, -1e300, 0.0), []),
        ("b_1e36", lambda: _normal(1.0, 109, shape), (-F32(0.01), F32(1e36), -F32(0.02), -F32(1e35)), []),
        ("a_positive", lambda: _normal(1.0, 110, shape), (F32(0.01), F32(0.002), F32(0.02), -F32(0.001)), []),
        ("constant", lambda: np.full(shape, 0.75), _QA, []),
    ]


def _is_f32(v):
    return float(np.float32(v)) == v


def range_cases(shape, prefix):
    out = []
    for fam, make, (ax, bx, ay, by), paths in _range_family(shape):
        osx, osy = (1, -2) if (bx != 0 or by != 0) else (0, 0)
        for dt, sfx in ((np.float32, "f32"), (np.float64, "f64")):
            f32 = dt == np.float32
            with np.errstate(over="ignore", under="ignore"):
                fused = (int(_is_f32(ax) and _is_f32(bx)) + int(_is_f32(ay) and _is_f32(by))) if f32 else 0
            out.append(_dt2d(f"{prefix}{fam}_{sfx}", (lambda make=make, dt=dt: make().astype(dt)), ax, bx, ay, by, osx, osy,
                             paths if f32 else [], fused=fused, dtype=dt))
    return out


RANGE_CASES = range_cases(RANGE_SHAPE, "range_")
# The subset whose COMPILED-REFERENCE outputs are recorded in tests/golden/ref_dt_v1.npz (tests/golden/make_ref_dt.py): 16 x 72 maps — nine
# segments per x line, enough for stitches — of every range family, plus two ordinary maps: small
# integers under a power-of-two curvature (exact ties in the pop test `s <= z[k]`) and a smooth map under weak curvature (rounds).
RECORDED_SHAPE = (16, 72)
RECORDED_CASES = range_cases(RECORDED_SHAPE, "rec_") + [
    _dt2d("rec_ints_f32", lambda: _ints(*RECORDED_SHAPE, 130), -2.0 ** -4, 0.0, -2.0 ** -4, 0.0, 1, -2, [], fused=2),
    _dt2d("rec_ints_f64", lambda: _ints(*RECORDED_SHAPE, 130, np.float64), -2.0 ** -4, 0.0, -2.0 ** -4, 0.0, 1, -2, [], fused=0, dtype=np.float64),
    _dt2d("rec_smooth_f32", lambda: _smooth(*RECORDED_SHAPE, 131), -F32(W), F32(0.001), -F32(0.002), -F32(0.001), 1, -2, [], fused=2),
    _dt2d("rec_smooth_f64", lambda: _smooth(*RECORDED_SHAPE, 131, np.float64), -W, 0.001, -0.002, -0.001, 1, -2, [], fused=0, dtype=np.float64),
]
REF_DT_FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_dt_v1.npz")


def recorded(fix, name):
    """(out, ix, iy) of one recorded case: scores in the case's type, pointers widened from the stored int16"""
    return fix[name + "_out"], fix[name + "_ix"].astype(np.int32), fix[name + "_iy"].astype(np.int32)


# the fold DP on responses of magnitude 2^96 .. 2^99 (small integers times 2^96: every sum and difference of the DP stays exact)
FOLD_CASES.append(dict(name="fold_f32_big", kind="fold", K=3, seed=34, wh=(320, 240), dtype=np.dtype(np.float32), paths=[], min_rounds=0,
                       scale=2.0 ** 96))
ALL_CASES = CASES + FOLD_CASES + RANGE_CASES
BY_NAME = {c["name"]: c for c in ALL_CASES}


# ---- non-finite maps: OUTSIDE the domain (refused by pbd_dt2d and by the replay; never handed to a kernel) -------------------------
def nonfinite_map(kind, dtype, shape=RANGE_SHAPE, seed=120):
    """kind: "-inf" / "+inf" / "nan" at 5 % of the positions, or "all-inf" (every value -inf)"""
    r = np.random.default_rng(seed)
    a = r.normal(0, 1.5, shape).astype(dtype)
    if kind == "all-inf":
        a[:] = -np.inf
    else:
        a[r.random(shape) < 0.05] = {"-inf": -np.inf, "+inf": np.inf, "nan": np.nan}[kind]
    return a


NONFINITE_KINDS = ["-inf", "+inf", "nan", "all-inf"]


# FINITE arguments whose x pass overflows: outside the domain (pbd_dt2d returns PBD_ERR_ARG after the run), and the y pass then meets +inf
# beside finite values in a DOUBLE line — s = -inf in a speculative stitch, the walk that did not end before its bound — or -inf
def overflow_case(kind):
    r = np.random.default_rng(5)
    a = r.normal(0, 1.5, RANGE_SHAPE)
    a[r.random(RANGE_SHAPE) < 0.05] = 1.79e308
    q = {"+inf": (-1e300, -1e306, -0.02, 0.0, 0, 0), "+inf_os": (-1e304, -1e306, -0.02, 0.0, 1, 0), "-inf": (-1e306, 0.0, -0.02, 0.0, 0, 0)}[kind]
    return _dt2d("overflow_" + kind, lambda: a, *q, [], fused=0, dtype=np.float64)


OVERFLOW_KINDS = ["+inf", "+inf_os", "-inf"]


def assert_same(got, ref, what):
    """(scores, Ix, Iy) bit for bit: scores compared as bytes"""
    assert got[0].dtype == ref[0].dtype, what
    np.testing.assert_array_equal(got[0].view(np.uint8), ref[0].view(np.uint8), err_msg=f"{what}: scores")
    np.testing.assert_array_equal(got[1], ref[1], err_msg=f"{what}: Ix")
    np.testing.assert_array_equal(got[2], ref[2], err_msg=f"{what}: Iy")


# ---- host replay --------------------------------------------------------------------------------------------------------
def build_replay(outdir):
    so = os.path.join(str(outdir), "dt_replay.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC,
                           os.path.join(ROOT, "tests", "tools", "dt_replay.cpp"), os.path.join(CSRC, "pbd_plan.cpp"), "-o", so])
    lib = C.CDLL(so)
    assert lib.dt_replay_ncounts() == len(HOST_COUNTERS)
    return lib


def replay(lib, case, want_rc=False, core=False):
    """(scores, ix, iy, counters) of pbd_dt2d on the case's input, replayed on the host; want_rc: only the return code (-1 where
    pbd_dt2d refuses the arguments, 1 where a pass left the finite range); core: without the domain check in front (host only)"""
    a = np.ascontiguousarray(case["make"](), case["dtype"])
    f64 = case["dtype"] == np.float64
    ct = C.c_double if f64 else C.c_float
    out = np.zeros_like(a)
    ix, iy = np.zeros(a.shape, np.int32), np.zeros(a.shape, np.int32)
    cnt = (C.c_longlong * len(HOST_COUNTERS))()
    ax, bx, ay, by, osx, osy = case["q"]
    fn = getattr(lib, ("dt_replay_core_dt2d" if core else "dt_replay_dt2d") + ("_f64" if f64 else ""))
    rc = fn(a.ctypes.data_as(C.POINTER(ct)), a.shape[0], a.shape[1], C.c_double(ax), C.c_double(bx), C.c_double(ay), C.c_double(by),
            osx, osy, out.ctypes.data_as(C.POINTER(ct)), ix.ctypes.data_as(C.POINTER(C.c_int32)), iy.ctypes.data_as(C.POINTER(C.c_int32)),
            cnt)
    if want_rc:
        return rc
    assert rc == 0, case["name"]
    return out, ix, iy, dict(zip(HOST_COUNTERS, list(cnt)))


# ---- GPU runs -----------------------------------------------------------------------------------------------------------
def run_case(case):
    """run the case through the library capi loaded (PBD_LIBRARY) and compare with the oracle: (mismatches: list of str)"""
    from oracle import orc
    from partsbaseddetector_amd import capi
    from partsbaseddetector_amd.model import make_tree_model
    bad = []
    if case["kind"] == "dt2d":
        a = case["make"]()
        h = capi.Handle(make_tree_model([-1, 0], 1, seed=1), conv_mode=capi.PBD_CONV_EXACT, dtype=case["dtype"])
        try:
            got = h.dt2d(a, *case["q"])
        finally:
            h.close()
        ref = orc.dt2d(a, *case["q"], dtype=case["dtype"])
        if not np.array_equal(got[0].view(np.uint8), ref[0].view(np.uint8)):
            bad.append(f"{case['name']}: scores differ at {int(np.count_nonzero(got[0] != ref[0]))} positions")
        for i, nm in ((1, "ix"), (2, "iy")):
            if not np.array_equal(got[i], ref[i]):
                bad.append(f"{case['name']}: {nm} differs at {int(np.count_nonzero(got[i] != ref[i]))} positions")
        return bad
    model = fold_model(case["K"], case["seed"])
    dt = case["dtype"]
    h = capi.Handle(model, conv_mode=capi.PBD_CONV_EXACT, dtype=dt)
    try:
        w, hh = case["wh"]
        h.begin_frame(w, hh, 3)
        g = h._geo
        rng = np.random.default_rng(case["seed"])
        nf = len(model.filtersw)
        resp = [(np.round(rng.normal(0, 1.5, (nf, g["cell_h"][l], g["cell_w"][l]))) * case.get("scale", 1.0)).astype(dt)
                for l in range(g["nlevels"])]
        for l in range(g["nlevels"]):
            for n in range(nf):
                h.set_level_response(l, n, resp[l][n])
        h.dp_min()
        desc = model.to_desc()
        for l in range(g["nlevels"]):
            Ix, Iy, Ik, rv, ri = orc.dp_min_level(desc, 0, resp[l], dtype=dt)
            grv, gri = h.root(l, 0)
            if not (np.array_equal(grv.view(np.uint8), rv.view(np.uint8)) and np.array_equal(gri, ri)):
                bad.append(f"{case['name']}: root scores / mixtures differ at level {l}")
            plane = 0
            for p in range(1, model.nparts(0)):
                for pm in range(len(model.filterid[0][model.parentid[0][p]])):
                    gx, gy, gk = h.dp_pointers(l, 0, p, pm)
                    if not (np.array_equal(gx, Ix[plane]) and np.array_equal(gy, Iy[plane]) and np.array_equal(gk, Ik[plane])):
                        bad.append(f"{case['name']}: pointers of part {p} mixture {pm} differ at level {l}")
                    plane += 1
    finally:
        h.close()
    return bad


def probe_counters():
    from partsbaseddetector_amd import capi
    out = (C.c_ulonglong * 8)()
    rc = capi.lib().pbd_debug_dt_counters(out)
    return rc, dict(zip(COUNTERS, [int(v) for v in out]))


def child_main(name):
    probe_counters()                      # reset
    bad = run_case(BY_NAME[name])
    rc, cnt = probe_counters()
    print(json.dumps(dict(case=name, rc=rc, counters=cnt, match=bad)))


def replay_child_main(so, kind, dtype, mode):
    """one map outside the domain through the host replay `so` (built by the parent): prints {"rc"} — a fresh process, so that a replay
    that did not return would cost its parent a time-out and nothing else.  mode "checked": as pbd_dt2d (non-finite maps are refused);
    "core": dt_core.hpp without the check in front.  kind: a NONFINITE_KINDS entry, or "overflow" + an OVERFLOW_KINDS entry."""
    lib = C.CDLL(so)
    if kind.startswith("overflow"):
        case = overflow_case(kind[len("overflow"):])
    else:
        a = nonfinite_map(kind, np.dtype(dtype))
        case = _dt2d("nonfinite", lambda: a, *_QA, 1, -2, [], fused=0, dtype=np.dtype(dtype))
    print(json.dumps(dict(kind=kind, dtype=dtype, mode=mode, rc=replay(lib, case, want_rc=True, core=mode == "core"))))


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    if sys.argv[1] == "--replay-child":
        replay_child_main(*sys.argv[2:6])
    else:
        child_main(sys.argv[1])
