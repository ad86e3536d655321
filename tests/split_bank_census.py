"""Which loop bodies of k_conv_split32 a bank reaches on a list of levels — plain Python, no GPU, no library.

The kernel (partsbaseddetector_amd/csrc/k_conv_split32.hpp) is instantiated per (NT n-tiles per workgroup, NS parts, MIX) and holds one
separately scheduled K loop per MV = M-tiles of the wavefront; the launcher picks NT from the filter count, the kernel MV from the unit's
valid cells.  Both choices are restated here, each beside the line it restates, so that a test can say which (NT, MV) bodies, ring parities
and remainder launches its banks and frames run.  A guard against vacuous coverage — not a reference: nothing on the GPU is compared with it."""
import collections

G = 5                    # k_conv_split32.hpp, launch_conv_split_groups: `int G = 5` n-tiles per full group (what the product launches)
NW = 4                   # k_conv_split.hip, launch_conv_split / launch_conv_split16: launch_conv_split_groups<4, 2, NS, MIX>
UNIT = 16                # pbd_plan.cpp, hog_conv_tiles: `for (int y = 0; y < L.ch; y += 16) for (int x = 0; x < L.cw; x += 16)`

# one K loop as a wavefront runs it: mix, nt, mv = the instantiation's MIX, NT and the switch's MV; ntile0, ngroups = the launch's arguments;
# ngroup = the workgroup's group (ntb = ntile0 + ngroup * NT); ntaps = kh * kw, the loop's trip count in taps
Body = collections.namedtuple("Body", "mix nt ntile0 ngroups ngroup mv ntaps")


def launches(nf):
    """[(NT, ntile0, ngroups)] of a uniform bank (or one size group) of nf filters.
    k_conv_split32.hpp, launch_conv_split_groups: `ntl = conv_split_ntiles(nf), full = ntl / G, rest = ntl - G * full;
    if (full) go(G, 0, full); if (rest) go(rest, G * full, 1);` with k_conv_split.hip `conv_split_ntiles(nf) = (nf + 31) / 32`"""
    ntl = (nf + 31) // 32
    full = ntl // G
    rest = ntl - G * full
    return ([(G, 0, full)] if full else []) + ([(rest, G * full, 1)] if rest else [])


def unit_mvs(ch, cw):
    """the MV of every wavefront that runs a K loop on a level of ch x cw cells, unit by unit.
    k_conv_split32.hpp, the kernel: `vw = min(16, W - tx0), vh = min(ROWS, H - ty0), ncell = vw * vh; nmt = (ncell + 15) >> 4;
    mvalid = max(0, min(4, (nmt - wave + NW - 1) / NW))` (ROWS = 4 NW = 16); `default: return` for mvalid = 0"""
    out = []
    for y0 in range(0, ch, UNIT):
        for x0 in range(0, cw, UNIT):
            vw, vh = min(UNIT, cw - x0), min(UNIT, ch - y0)
            nmt = (vw * vh + 15) >> 4
            out += [mv for mv in (max(0, min(4, (nmt - wave + NW - 1) // NW)) for wave in range(NW)) if mv]
    return out


def size_groups(sizes):
    """{(kh, kw): filters} — pbd_plan.cpp, plan_model: the size groups of a mixed bank are the runs of one kh x kw in the size-sorted
    filter order, so one group per distinct size whatever the caller's order"""
    return collections.Counter(map(tuple, sizes))


def reached(sizes, levels):
    """the set of Body a bank (sizes[n] = (kh, kw)) runs on levels [(ch, cw)].  A bank of one size is uniform (capi.Handle: pbd_create);
    pbd_api.cpp, run_pdf: a mixed bank launches every size group over every tile of the frame"""
    groups = size_groups(sizes)
    mix = len(groups) > 1
    mvs = {mv for ch, cw in levels for mv in unit_mvs(ch, cw)}
    return {Body(mix, nt, ntile0, ngroups, g, mv, kh * kw)
            for (kh, kw), nf in groups.items() for nt, ntile0, ngroups in launches(nf) for g in range(ngroups) for mv in mvs}


def instantiations(bodies, ns):
    """the kernels' names as tests/test_kernel_census.py spells them"""
    return {f"k_conv_split32<{b.nt},{NW},2,{ns},{'true' if b.mix else 'false'}>" for b in bodies}


def loop_bodies(bodies, ns):
    """(NS, MIX, NT, MV): the separately register-allocated, hand-scheduled K loops"""
    return {(ns, b.mix, b.nt, b.mv) for b in bodies}
