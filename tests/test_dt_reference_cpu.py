"""The distance transform against the COMPILED reference, and over the whole finite float range — on the host (no GPU).

1. oracle/_ref/libref_dt.so — the reference's include/DistanceTransform.hpp compiled in place against a storage-only cv::Mat_
   (oracle/ref_dt/README.md) — equals the oracle's restatement (orc.dt2d) bit for bit on every dt2d case of tests/dt_path_cases.py, on
   the maps of test_reference_pins.py, and on non-finite maps (where both simply run the reference's loop).  Skips without the binary.
2. tests/golden/ref_dt_v1.npz, the compiled reference's recorded outputs, equals the binary (when present) and the oracle (always).
3. The host replay of k_dt_pass (tests/tools/dt_replay.cpp: the kernel's own dt_core.hpp) equals the oracle on every RANGE_CASES entry,
   and the float cases that must leave the float range do flag.
4. Outside the domain (DESIGN.md "Input domain of the distance transform"): the replay refuses non-finite maps as pbd_dt2d does; without
   that check dt_core.hpp still ends on every one of them; and a FINITE map whose x pass overflows — +inf beside finite values in the y
   pass's double lines, the walk that did not end before it was bounded — ends and is reported.  Every such replay runs in a fresh child
   process under a time limit, so that a regression costs a failure, not a hung suite.
5. Sensitivity: a Python model of computeRow reproduces the record, and stops doing so when it is perturbed where the output can see
   it (the read-out's comparison).  Three perturbations of the STACK — `<` for `<=` in the pop test,
   no `k > 0`, (T)os compared exactly — change the stack and not the output (the last two by argument, the first: no
   counter-example found); the tests say why and pin that they are real.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref_dt
from tests import dt_path_cases as dc

needs_binary = pytest.mark.skipif(not ref_dt.available(), reason="oracle/_ref/libref_dt.so not built (no reference checkout)")
DT2D_CASES = [c for c in dc.CASES + dc.RANGE_CASES if c["kind"] == "dt2d"]


_same = dc.assert_same


@pytest.fixture(scope="module")
def replay_lib(tmp_path_factory):
    return dc.build_replay(tmp_path_factory.mktemp("dt_replay"))


@pytest.fixture(scope="module")
def fixture_npz():
    return np.load(dc.REF_DT_FIXTURE)


# ---- 1. compiled reference == oracle ------------------------------------------------------------------------------------------
@needs_binary
@pytest.mark.parametrize("name", [c["name"] for c in DT2D_CASES])
def test_compiled_reference_equals_oracle(orc, name):
    case = dc.BY_NAME[name]
    a = case["make"]()
    _same(ref_dt.dt2d(a, *case["q"], dtype=case["dtype"]), orc.dt2d(a, *case["q"], dtype=case["dtype"]), name)


@needs_binary
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_compiled_reference_equals_oracle_on_the_pinned_maps(orc, dtype):
    """the six maps of test_reference_pins.py::test_distance_transform_matches_the_reference (1 x 7 and 9 x 1 among them)"""
    rng = np.random.default_rng(20260927)
    for i, (r, c) in enumerate([(7, 9), (23, 31), (40, 57), (118, 158), (1, 7), (9, 1)]):
        a = rng.normal(0, 1.5, (r, c)).astype(np.float32)
        if i == 2:
            a = np.round(a)
        q = (-0.01 - 0.01 * i, 0.002 * i, -0.02, -0.001 * i, i % 5 - 2, 2 - i % 5)
        _same(ref_dt.dt2d(a.astype(dtype), *q, dtype=dtype), orc.dt2d(a.astype(dtype), *q, dtype=dtype), f"map {i} {r}x{c}")


@needs_binary
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", dc.NONFINITE_KINDS)
def test_compiled_reference_equals_oracle_on_nonfinite_maps(orc, kind, dtype):
    """outside the product's domain, but the oracle is the reference's loop restated and must follow it there too (NaN compares equal
    as bytes: both run the same IEEE operations in the same order)"""
    a = dc.nonfinite_map(kind, np.dtype(dtype))
    q = (*dc._QA, 1, -2)
    _same(ref_dt.dt2d(a, *q, dtype=dtype), orc.dt2d(a, *q, dtype=dtype), f"{kind} {np.dtype(dtype).name}")


# ---- 2. the recorded fixture ------------------------------------------------------------------------------------------------------
def test_fixture_holds_exactly_the_recorded_cases(fixture_npz):
    assert sorted(fixture_npz.files) == sorted(c["name"] + s for c in dc.RECORDED_CASES for s in ("_out", "_ix", "_iy"))
    assert os.path.getsize(dc.REF_DT_FIXTURE) <= max(os.path.getsize(os.path.join(os.path.dirname(dc.REF_DT_FIXTURE), f))
                                                     for f in ("golden_v1.npz", "golden_f64_v1.npz", "ref_hog_v1.npz"))
    for c in dc.RECORDED_CASES:
        assert c["make"]().shape == dc.RECORDED_SHAPE and fixture_npz[c["name"] + "_out"].dtype == c["dtype"]


@needs_binary
@pytest.mark.parametrize("name", [c["name"] for c in dc.RECORDED_CASES])
def test_fixture_equals_compiled_reference(fixture_npz, name):
    case = next(c for c in dc.RECORDED_CASES if c["name"] == name)
    _same(dc.recorded(fixture_npz, name), ref_dt.dt2d(case["make"](), *case["q"], dtype=case["dtype"]), name)


@pytest.mark.parametrize("name", [c["name"] for c in dc.RECORDED_CASES])
def test_fixture_equals_oracle(orc, fixture_npz, name):
    case = next(c for c in dc.RECORDED_CASES if c["name"] == name)
    _same(orc.dt2d(case["make"](), *case["q"], dtype=case["dtype"]), dc.recorded(fixture_npz, name), name)


# ---- 3. the kernel's source on the host, over the range ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in dc.RANGE_CASES + dc.RECORDED_CASES])
def test_replay_equals_oracle_over_the_range(replay_lib, orc, name):
    case = dc.BY_NAME.get(name) or next(c for c in dc.RECORDED_CASES if c["name"] == name)
    a = case["make"]()
    assert np.isfinite(a).all() and a.dtype == case["dtype"]
    out, ix, iy, cnt = dc.replay(replay_lib, case)
    print(f"{name}: replay {cnt}")
    ref = orc.dt2d(a, *case["q"], dtype=case["dtype"])
    # inside the domain through BOTH passes (a finite map can leave it between them: test_finite_map_whose_x_pass_overflows_... is that boundary)
    assert np.isfinite(ref[0]).all() and dc.replay(replay_lib, case, want_rc=True) == 0
    _same((out, ix, iy), ref, name)
    missing = [p for p in case["paths"] if cnt[p] < 1]
    assert not missing, (name, missing, cnt)
    assert cnt["fused_groups"] == case["fused"], (name, cnt)
    assert cnt["seq_redos"] == cnt["scan_flags"] + cnt["stitch_flags"]
    if case["dtype"] == np.float64:
        assert cnt["scan_flags"] == 0            # IEEE divisions throughout: nothing to suspect


# ---- 4. outside the domain: refused in front, and dt_core.hpp ends on every bit pattern ------------------------------------------------
def _child(replay_lib, kind, dtype, mode):
    """a fresh child process under a time limit: a time-out is a failure (a loop of dt_core.hpp that does not end), never a hung suite"""
    try:
        r = subprocess.run([sys.executable, "-m", "tests.dt_path_cases", "--replay-child", replay_lib._name, kind, dtype, mode], cwd=dc.ROOT,
                           capture_output=True, text=True, timeout=30)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the replay ({mode}) of a {dtype} map with {kind} did not terminate within 30 s")
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert (res["kind"], res["dtype"], res["mode"]) == (kind, dtype, mode)
    return res["rc"]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kind", dc.NONFINITE_KINDS)
def test_nonfinite_replay_is_refused(replay_lib, kind, dtype):
    """the replay mirrors pbd_dt2d's argument checks (dt_replay.cpp: replay_dt2d): -1 at once"""
    assert _child(replay_lib, kind, dtype, "checked") == -1


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kind", dc.NONFINITE_KINDS)
def test_nonfinite_replay_terminates_in_dt_core(replay_lib, kind, dtype):
    """the same maps WITHOUT the check in front: scans, speculative stitches, rounds and redos of dt_core.hpp end whatever the line holds
    (a +inf in a double map did not, before the stitch walk protected every self-linked bottom).  What comes out is not the reference's."""
    assert _child(replay_lib, kind, dtype, "core") in (0, 1)


@pytest.mark.parametrize("kind", dc.OVERFLOW_KINDS)
def test_finite_map_whose_x_pass_overflows_terminates_and_is_reported(replay_lib, orc, kind):
    """finite scores, finite quadratics — nothing for the front check to refuse — and an x pass that overflows a double: the y pass runs on
    +inf beside finite values (s = -inf in the stitches) or on -inf.  It must end, and the call reports that a pass left the finite range
    (rc 1: pbd_dt2d's PBD_ERR_ARG after the run); the oracle agrees that the map is outside the domain."""
    case = dc.overflow_case(kind)
    a = case["make"]()
    assert np.isfinite(a).all() and all(np.isfinite(v) for v in case["q"])
    assert not np.isfinite(orc.dt2d(a, *case["q"], dtype=np.float64)[0]).all()
    assert _child(replay_lib, "overflow" + kind, "float64", "checked") == 1


def test_replay_refuses_nonfinite_quadratics(replay_lib):
    for i in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            q = [-0.01, 0.002, -0.02, -0.001]
            q[i] = bad
            case = dc._dt2d("badq", lambda: np.zeros((8, 16), np.float32), *q, 0, 0, [], fused=0)
            assert dc.replay(replay_lib, case, want_rc=True) == -1


# ---- 5. sensitivity -------------------------------------------------------------------------------------------------------------
def model_row(src, a, b, os_, T, strict_pop=False, guard=True, os_as_double=False, stack=False, readout_le=False):
    """DistanceTransform<T>::computeRow (:151-182) with Quadratic (:98-104), operation by operation: fp64 arithmetic on T values and ints,
    `T s = f(...)` narrowed, the pop test `s <= z[k] && k > 0`, the read-out's `z[k+1] < os` in T.  Python ints: no overflow anywhere.
    Perturbations: strict_pop (`<` for `<=`), guard = False (no `k > 0`: popping the bottom makes q the new bottom), os_as_double (the
    read-out compares z with the int offset exactly instead of with (T)os).  stack: return the final stack (v, z) instead of the read-out.
    A perturbation the output does see: readout_le (`z[k+1] <= os`)."""
    D = np.float64
    a, b = D(a), D(b)
    N = len(src)
    y = [D(v) for v in src]

    def isect(x0, x1):
        return T(((y[x1] - y[x0]) - b * D(x1 - x0) + a * D(x1 * x1 - x0 * x0)) / (D(2) * a * D(x1 - x0)))
    v, z = [0] * N, [T(0)] * (N + 1)
    k = 0
    z[0] = T(-np.inf)
    if N > 0:
        z[1] = T(np.inf)
    with np.errstate(all="ignore"):
        for q in range(1, N):
            s = isect(v[k], q)
            while ((s < z[k]) if strict_pop else (s <= z[k])) and (k > 0 or not guard):
                k -= 1
                if k < 0:
                    break
                s = isect(v[k], q)
            k += 1
            v[k] = q
            z[k] = s if k > 0 else T(-np.inf)
            z[k + 1] = T(np.inf)
        if stack:
            return v[:k + 1], z[:k + 1]
        k = 0
        dst, ptr = np.zeros(N, T), np.zeros(N, np.int32)
        for q in range(N):
            while (D(z[k + 1]) < D(os_)) if os_as_double else (z[k + 1] <= T(os_)) if readout_le else (z[k + 1] < T(os_)):
                k += 1
            x = os_ - v[k]
            dst[q] = T(a * D(x * x) + b * D(x) + y[v[k]])
            ptr[q] = v[k]
            os_ += 1
    return dst, ptr


def model_dt2d(a_, ax, bx, ay, by, osx, osy, **kw):
    """DistanceTransform<T>::compute (:203-245): rows, columns of the intermediate, pointers composed as Iy[m][Ix[m][n]]"""
    T = a_.dtype.type
    M, N = a_.shape
    tmp, Ix = np.zeros((M, N), T), np.zeros((M, N), np.int32)
    for m in range(M):
        tmp[m], Ix[m] = model_row(a_[m], ax, bx, osx, T, **kw)
    out, Iy = np.zeros((M, N), T), np.zeros((M, N), np.int32)
    for n in range(N):
        out[:, n], Iy[:, n] = model_row(tmp[:, n], ay, by, osy, T, **kw)
    return out, Ix, np.take_along_axis(Iy, Ix, axis=1)


def _differs(got, ref):
    return not all(np.array_equal(g.view(np.uint8), r.view(np.uint8)) for g, r in zip(got, ref))


@pytest.fixture(scope="module")
def model_results(fixture_npz):
    """which recorded cases each form of the model reproduces: computed once for the tests below"""
    forms = dict(exact={}, strict_pop=dict(strict_pop=True), no_guard=dict(guard=False), os_as_double=dict(os_as_double=True),
                 readout_le=dict(readout_le=True))
    res = {f: [] for f in forms}
    for c in dc.RECORDED_CASES:
        a = c["make"]()
        rec = dc.recorded(fixture_npz, c["name"])
        for f, kw in forms.items():
            if _differs(model_dt2d(a, *c["q"], **kw), rec):
                res[f].append(c["name"])
    return res


def test_model_reproduces_the_record(model_results):
    """the unperturbed model is the reference: every recorded case, bit for bit — so a difference below is the perturbation's"""
    assert model_results["exact"] == []


def test_record_catches_a_perturbed_read_out(model_results):
    """items 1-3 can fail: `z[k+1] <= os` for `<` in the read-out shows wherever an intersection falls on an integer (small integers,
    power-of-two curvature).  The comparison here is the one items 1-3 make (scores as bytes, Ix, Iy)."""
    print(f"readout_le: caught by {model_results['readout_le']}")
    assert "rec_ints_f32" in model_results["readout_le"] and "rec_ints_f64" in model_results["readout_le"]


def test_dropped_bottom_guard_is_invisible_in_the_output(model_results):
    """without `k > 0` the bottom is popped only by s = -inf (z[0] = -inf): a float quotient that overflowed.  The reference then pushes
    q with z = -inf ON the bottom, which hides the bottom from the read-out just as popping it does; the bottom could come back only
    through an element q' with s(q, q') = -inf and s(v[0], q') finite, and two jumps that each overflow the quotient sum to one that
    overflows it too (the threshold is proportional to the distance).  So no output depends on the guard; the record agrees."""
    print(f"no_guard: caught by {model_results['no_guard']}")
    assert model_results["no_guard"] == []
    case = next(c for c in dc.RECORDED_CASES if c["name"] == "rec_uniform_3e38_f32")
    popped = sum(model_row(row, case["q"][0], case["q"][1], 0, np.float32, guard=False, stack=True)[0][0] != 0 for row in case["make"]())
    assert popped > 0, "rec_uniform_3e38_f32 no longer reaches the bottom of a stack with s = -inf"


def test_strict_pop_test_is_invisible_in_the_output(model_results):
    """`s < z[k]` for `s <= z[k]` differs on exact ties — and then keeps an entry with z[k] == z[k+1], an EMPTY interval, which the
    read-out (`while (z[k+1] < os) k++`) can never stop on; a later element that pops its way down meets the kept entry at the tie point
    or left of it and pops it too (or ties again).  So the perturbation changes the stack and, as far as anyone has found, not the output (not proven: with a
    non-dyadic curvature the re-intersection after a pop may round an ulp away from the tie): no recorded case notices it, and none was found among 6 000 random lines of six kinds (integers, quarter steps, dyadic and non-dyadic curvature, offsets of
    40 000, values of 1e6 and 1e7) nor on integer maps under positive curvature.  What the record does pin is that the perturbation is
    real: on the integer map the stacks differ."""
    print(f"strict_pop: caught by {model_results['strict_pop']}")
    assert model_results["strict_pop"] == []
    case = next(c for c in dc.RECORDED_CASES if c["name"] == "rec_ints_f32")
    a = case["make"]()
    deeper = 0
    for row in a:
        (v0, z0), (v1, z1) = model_row(row, case["q"][0], case["q"][1], 0, np.float32, stack=True), \
            model_row(row, case["q"][0], case["q"][1], 0, np.float32, strict_pop=True, stack=True)
        assert set(v0) <= set(v1)                                     # the strict form only ever keeps more
        empty = [k for k in range(1, len(v1)) if v1[k] not in v0]
        assert all(z1[k] == (z1[k + 1] if k + 1 < len(z1) else None) or v1[k] in v0 for k in empty if k + 1 < len(z1))
        deeper += len(v1) > len(v0)
    assert deeper > 0, "rec_ints_f32 has no exact tie: the case no longer exercises `s <= z[k]` with equality"


def test_offset_comparison_perturbation(model_results):
    """`z[k+1] < os` compares in T: the int offset is converted, (float)os.  Comparing exactly instead can differ only where (float)os != os,
    i.e. |os| > 2^24 — and the reference squares the INT distance os - v[k] (Quadratic::square), which overflows from 46 341 on, so no
    input the reference defines reaches it: inside the domain the two forms are the same function and no recorded case may tell them
    apart.  The perturbation itself is real, and the comparison sees it where the model (Python ints) is still defined: one line at
    os = 2^24 + 1 whose only intersection rounds to 2^24."""
    assert model_results["os_as_double"] == []
    src = np.array([2.0 ** 24, 0.0], np.float32)
    exact = model_row(src, -0.5, 0.0, 2 ** 24 + 1, np.float32)
    pert = model_row(src, -0.5, 0.0, 2 ** 24 + 1, np.float32, os_as_double=True)
    assert list(exact[1]) == [0, 1] and list(pert[1]) == [1, 1]
    assert _differs(pert, exact)


# ---- the domain at the front door (no GPU needed: the model is refused before a device is looked for) -----------------------------------
def test_create_refuses_nonfinite_weights_on_the_host():
    from partsbaseddetector_amd import capi
    from partsbaseddetector_amd.model import make_tree_model
    for field in ("biasw", "defw", "filtersw"):
        for bad in (np.nan, np.inf, -np.inf):
            m = make_tree_model([-1, 0, 0], 2, seed=3)
            w = getattr(m, field)
            if isinstance(w, list):
                w = [np.array(x, np.float32) for x in w]
                w[-1].flat[0] = bad
            else:
                w = np.array(w, np.float32)
                w.flat[w.size - 1] = bad
            setattr(m, field, w)
            with pytest.raises(capi.PbdError) as e:
                capi.Handle(m, conv_mode=capi.PBD_CONV_EXACT)
            assert e.value.code == capi.PBD_ERR_ARG and "non-finite" in str(e.value), (field, bad, e.value)
