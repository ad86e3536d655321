"""The DP cases of tests/dp_range_cases.py on the host: every case stays inside the domain (finite, with the margin the tree gives), the
oracle's DP (orc.dp_min_level) equals the plain statement of tests/dp_ref.py (brute-force max-plus, the distance transform by definition,
the first maximum), and that statement with one slip differs from the oracle on the family aimed at the slip."""
import numpy as np
import pytest

from tests import dp_ref
from tests import dp_range_cases as R

PLAIN_LEVELS = (0, 7, 14, 20)        # 23 x 18, 14 x 10, 8 x 6 and 4 x 3 cells


@pytest.fixture(scope="module")
def geo(orc):
    g = orc.geometry(*R.FRAME, 4, 10)
    assert g["nlevels"] == 21 and (g["cell_w"][0], g["cell_h"][0], g["cell_w"][20], g["cell_h"][20]) == (23, 18, 4, 3)
    assert (int(g["cell_w"][0]), int(min(g["cell_w"]))) == R.LEVEL_W
    return g


@pytest.fixture(scope="module")
def cases(geo):
    return R.build_cases()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _zero_counts(v):
    z = v == 0
    return int((z & np.signbit(v)).sum()), int((z & ~np.signbit(v)).sum())


def test_case_list_covers_the_issue(cases, geo):
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for fam in "ZMQA":
        sel = [c for c in cases if c["family"] == fam]
        assert {c["dp_mode"] for c in sel} == {0, 1, 2}, fam
        assert any(np.float32 in c["dtypes"] for c in sel) and any(np.float64 in c["dtypes"] for c in sel)
    # Z: the tree shapes of TIE_CASES; A: all six anchor values on both axes, relative to the smallest and to the largest level
    assert {c["name"].split("_")[2] for c in cases if c["family"] == "Z"} == set(R.TREES)
    for c in cases:
        if "anchor_W" in c:
            assert c["anchor_W"] in (4, 23)
            for axis in range(2):
                assert set(R.anchor_values(c["anchor_W"])) == set(c["model"].anchors[:, axis].tolist()), c["name"]
            assert any(a[0] * a[1] < 0 for a in c["model"].anchors) and any(a[0] * a[1] > 0 for a in c["model"].anchors)
            K = [ids for ids in c["model"].defid[0] if len(ids) > 1]
            assert any(len({tuple(c["model"].anchors[d]) for d in ids}) > 1 for ids in K), c["name"]
    # a negative deformation weight (positive `a`) passes the model checks of the planner: the case exists (asserted against
    # pbd_create itself in tests/test_gpu_dp_range.py)
    assert sum(1 for c in cases if c.get("positive_a")) == 1


def test_every_case_is_finite_with_margin(orc, cases, geo):
    """Every value the oracle's DP exposes (rootv; the pointers are integers inside the map) is finite at every level, and so is every
    intermediate of the plain statement, because parts x (|response| + |bias| + deformation at the diagonal) <= max(T) / 2.  No case is
    excluded.  Family Z: the expected root scores hold BOTH zero patterns in every case — otherwise the case tests nothing."""
    for c in cases:
        desc = c["model"].to_desc()
        for dt in c["dtypes"]:
            neg = pos = 0
            for l in range(geo["nlevels"]):
                resp = R.responses(c, geo, l, dt)
                assert np.isfinite(resp).all()
                assert R.tree_bound(c["model"], resp) <= float(np.finfo(dt).max) / 2, (c["name"], dt, l)
                Ix, Iy, Ik, rv, ri = orc.dp_min_level(desc, 0, resp, dtype=dt)
                assert np.isfinite(rv).all(), (c["name"], dt, l)
                H, W = rv.shape
                assert Ix.min(initial=0) >= 0 and Iy.min(initial=0) >= 0 and Ix.max(initial=0) < W and Iy.max(initial=0) < H
                n, p = _zero_counts(rv)
                neg, pos = neg + n, pos + p
            if c["family"] == "Z":
                assert neg > 0 and pos > 0, (c["name"], dt, neg, pos)
    # the magnitudes reach what they claim: the top cases come within 2^-5 of max(T) / 2, the subnormal case is subnormal
    by = {c["name"]: c for c in cases}
    for dt in R.DTYPES:
        top = R.responses(by["M_top_K10"], geo, 0, dt)
        assert R.tree_bound(by["M_top_K10"]["model"], top) > float(np.finfo(dt).max) / 64
        sub = R.responses(by["M_subnormal_M4"], geo, 0, dt)
        assert 0 < np.abs(sub).max() < float(np.finfo(dt).tiny)


def _differs(a, b):
    return any(np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def test_oracle_equals_the_plain_statement(orc, cases, geo):
    """Ix, Iy, Ik, rooti equal and rootv equal BIT FOR BIT (the sign of zero included) in every case, exact sums or not: the plain
    statement evaluates the same quadratic a sq + b d + y in double and narrows once, as Quadratic::operator() does, so where the
    reference's stack algorithm finds the maximum the two do the same additions — no bound is needed, and none is used.
    The one exception is positive `a`: the stack algorithm is then no max-plus transform (the envelope it keeps is the wrong one), there
    is no plain statement of what it returns, and the DT of the statement is the oracle's own (orc.dt2d, pinned to the compiled reference
    by tests/test_dt_reference_cpu.py on that very family); the message passing around it is still the plain one."""
    for c in cases:
        desc = c["model"].to_desc()
        for dt in c["dtypes"]:
            for l in PLAIN_LEVELS:
                resp = R.responses(c, geo, l, dt)
                want = orc.dp_min_level(desc, 0, resp, dtype=dt)
                got = dp_ref.plain_level(c["model"], 0, resp, dt, orc=orc if c.get("positive_a") else None)
                for name, g, w in zip(("Ix", "Iy", "Ik", "rootv", "rooti"), got, want):
                    if name == "rootv":
                        g, w = _bits(g), _bits(w)
                    np.testing.assert_array_equal(g, w, err_msg=f"{name} {c['name']} {np.dtype(dt).name} level {l}")


def test_exact_cases_are_exact(cases, geo):
    """`exact` cases: the statement in double on the same (float-representable) planes gives the float statement's root scores — no
    sum of the float DP rounded."""
    for c in cases:
        if not c["exact"]:
            continue
        for l in PLAIN_LEVELS:
            resp = R.responses(c, geo, l, np.float32)
            a = dp_ref.plain_level(c["model"], 0, resp, np.float32)
            b = dp_ref.plain_level(c["model"], 0, resp.astype(np.float64), np.float64)
            assert np.array_equal(a[3].astype(np.float64), b[3]), c["name"]


# ---------------------------------------------------------------- sensitivity
AIMED = {"zero_order": "Z", "ge": "Z", "bias_after_max": "M", "anchor_clamp": "A", "child_count": "Q"}


def _caught(orc, cases, geo, slip):
    """names of the cases of the family the slip is aimed at on which the statement with that slip differs from the oracle"""
    hit = []
    for c in cases:
        if c["family"] != AIMED[slip]:
            continue
        desc = c["model"].to_desc()
        for dt in c["dtypes"]:
            for l in PLAIN_LEVELS:
                resp = R.responses(c, geo, l, dt)
                use_orc = orc if c.get("positive_a") else None
                if _differs(dp_ref.plain_level(c["model"], 0, resp, dt, orc=use_orc, slip=slip), orc.dp_min_level(desc, 0, resp, dtype=dt)):
                    hit.append(c["name"])
                    break
    return hit


def _proof(orc, cases, geo):
    return {slip: _caught(orc, cases, geo, slip) for slip in dp_ref.SLIPS}


def test_sensitivity(orc, cases, geo):
    """-0.0 ordered below +0.0 (a hardware max, integer keys), `>=` for `>`, the bias added after the max, the anchor clamped to the map
    before the read-out, the child's mixture count for the parent's: each differs from the oracle on its family, float and double."""
    proof = _proof(orc, cases, geo)
    assert all(proof.values()), proof
    # signed zeros: EVERY case of the family with a reduce in it (M = 1 has one mixture per part: reduceMax copies) tells the two orders
    # apart, and no case outside the family can (none holds a -0.0)
    assert set(proof["zero_order"]) == {c["name"] for c in cases if c["family"] == "Z" and max(map(len, c["model"].filterid[0])) > 1}
    for c in cases:
        if c["family"] == "Z":
            continue
        for dt in c["dtypes"]:
            resp = R.responses(c, geo, 0, dt)
            assert not _differs(dp_ref.plain_level(c["model"], 0, resp, dt, orc=orc, slip="zero_order"),
                                orc.dp_min_level(c["model"].to_desc(), 0, resp, dtype=dt)), c["name"]


def test_sensitivity_needs_every_family(orc, cases, geo):
    """the proof above is not vacuous: with the family a slip is aimed at removed, that slip goes unseen by the proof"""
    for fam in "ZMQA":
        proof = _proof(orc, [c for c in cases if c["family"] != fam], geo)
        for slip, aimed in AIMED.items():
            assert bool(proof[slip]) == (aimed != fam), (fam, slip)
