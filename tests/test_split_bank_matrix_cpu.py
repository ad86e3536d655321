"""What tests/test_gpu_split_bank_matrix.py reaches inside k_conv_split32 — no GPU: the census of tests/split_bank_census.py (the launchers'
choice of NT per launch and the kernel's choice of MV per wavefront, restated) over the matrix's banks and frames.  A guard against vacuous
coverage: a bank list or a frame that stops reaching a loop body, a ring parity or a remainder launch fails here."""
from tests import exact_bank_cases as X
from tests import split_bank_census as census
from tests.test_kernel_census import LAUNCHABLE

BANKS = [[(kh, kw)] * nf for nf, kh, kw in X.MATRIX_BANKS] + [X.matrix_mixed_sizes()]
NS = (3, 2)              # both split banks run every bank: PBD_CONV_SPLIT (three bfloat16 parts) and PBD_CONV_SPLIT_F16 (two binary16 parts)


def _levels(orc, frames):
    out = []
    for f in frames:
        g = orc.geometry(f[0], f[1], X.SBIN, X.INTERVAL)
        out += [(int(h), int(w)) for h, w in zip(g["cell_h"], g["cell_w"])]
    return out


def _bodies(orc):
    levels = _levels(orc, X.MATRIX_FRAMES)
    return set().union(*(census.reached(b, levels) for b in BANKS))


def test_launches_restated():
    """the launchers' arithmetic on counts whose launches the kernel's header states in words: 156 filters in one pass of five n-tiles,
    161 as five and one more, 208 as 5 + 2, 312 as two groups"""
    assert census.launches(16) == [(1, 0, 1)] and census.launches(33) == [(2, 0, 1)]
    assert census.launches(156) == [(5, 0, 1)] and census.launches(160) == [(5, 0, 1)]
    assert census.launches(161) == [(5, 0, 1), (1, 5, 1)]
    assert census.launches(208) == [(5, 0, 1), (2, 5, 1)]
    assert census.launches(312) == [(5, 0, 2)] and census.launches(321) == [(5, 0, 2), (1, 10, 1)]
    assert sorted(census.unit_mvs(16, 16)) == [4, 4, 4, 4] and census.unit_mvs(3, 3) == [1]
    assert sorted(census.unit_mvs(17, 17)) == [1, 1, 1, 4, 4, 4, 4]


def test_frames_hold_every_kind_of_level(orc):
    assert _levels(orc, [X.MATRIX_FRAMES[0]]) == [(17, 17), (13, 13), (10, 10), (8, 8), (6, 6), (4, 4)]
    assert _levels(orc, [X.MATRIX_FRAMES[1]]) == [(6, 6), (4, 5), (3, 3)]
    levels = _levels(orc, X.MATRIX_FRAMES)
    assert any(h >= 16 and w >= 16 for h, w in levels)               # a full unit
    assert any(w % 16 == 1 and w > 16 for h, w in levels)            # a one-cell-wide ragged unit
    assert any(h % 16 == 1 and h > 16 for h, w in levels)            # a one-row unit
    assert any(w < 16 and h * w >= 16 for h, w in levels)            # M-tiles straddle rows
    assert any(h * w < 16 for h, w in levels)                        # less than one M-tile
    assert {mv for h, w in levels for mv in census.unit_mvs(h, w)} == {1, 2, 3, 4}
    assert sum(h * w for h, w in levels) < 1000                      # (the GPU test reads every plane of every level)
    sweep = _levels(orc, [X.SWEEP_FRAME])
    assert sweep == [(11, 11), (8, 8), (6, 6), (5, 5), (3, 3)]       # all under a unit: a 9 x 9 filter's halo is wider than the level


def test_every_loop_body_is_reached(orc):
    bodies = _bodies(orc)
    loops = set().union(*(census.loop_bodies(bodies, ns) for ns in NS))
    assert loops == {(ns, mix, nt, mv) for ns in NS for mix in (False, True) for nt in range(1, 6) for mv in range(1, 5)}
    assert len(loops) == 80
    names = set().union(*(census.instantiations(bodies, ns) for ns in NS))
    assert names == {n for n in LAUNCHABLE if n.startswith("k_conv_split32<")} and len(names) == 20


def test_ring_parities_remainders_and_short_loops(orc):
    bodies = _bodies(orc)
    even = {b.nt for b in bodies if b.ntaps % 2 == 0}
    odd = {b.nt for b in bodies if b.ntaps % 2 == 1}
    assert {1, 3, 5} <= even                                         # odd NT: a two-tap body left through the loop's condition
    assert {1, 3, 5} <= odd                                          # ... and through the break in its middle
    assert {2, 4} <= even and {2, 4} <= odd
    assert {b.nt for b in bodies if b.ntile0 == 5} >= {1, 2, 3, 4}   # every remainder behind one full group
    assert any(b.ngroup == 1 for b in bodies)                        # a second full group: ntb = ntile0 + ngroup * NT
    assert any(b.ntile0 == 10 for b in bodies)                       # ... and the remainder behind it
    assert {b.nt for b in bodies if b.mix} == {1, 2, 3, 4, 5}
    assert any(b.mix and b.ntile0 > 0 for b in bodies)               # a size group with a remainder launch
    for ntaps in (1, 2):
        assert any(b.ntaps == ntaps and b.nt % 2 == 1 and not b.mix for b in bodies)
        assert any(b.ntaps == ntaps and b.nt % 2 == 0 for b in bodies)
    for nt in range(1, 6):                                           # every MV of every NT at either parity it was asked at above
        assert {b.mv for b in bodies if b.nt == nt and b.ntaps % 2 == 0} == {1, 2, 3, 4}
