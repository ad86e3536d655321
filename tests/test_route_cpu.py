"""The frame route (partsbaseddetector_amd/csrc/pbd_route.hpp) on the host, no GPU: tests/tools/route_check.cpp evaluates
route_frame for every combination of frame kind, candidate filter mode x NMS kind, the four post-stage settings, the compact plan,
RCCL-gathering membership and the zero-copy build flag (3840 rows).  The route is what decides which buffer each kernel behind the
back-tracking reads and writes and what the collect is told about the frame, so the properties that used to hold through comments
are stated here outright, for every row; ten rows are then spelled out by hand, field by field."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from partsbaseddetector_amd.capi import PBD_CAND_RAW, PBD_CAND_SORT, PBD_CAND_SORT_NMS, PBD_NMS_PAINTED, PBD_NMS_PARTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partsbaseddetector_amd", "csrc")

STAGE_FIELDS = ("on", "in", "in_count", "out", "out_count")
ROUTE_FIELDS = (("latent", "gt", "bt_out", "bt_count", "bt_host_count")
                + tuple(f"{s}_{f}" for s in ("zf", "filter", "parts") for f in STAGE_FIELDS)
                + ("filter_mode", "count_d2h", "first_d2h", "pack_count", "final_buf", "final_count",
                   "active", "on_host", "filtered", "pending_gt", "b3", "cl3", "b3_has", "ps", "ps_compact", "dp_timed"))
HAS = 0b101   # the depth frames of a row's job


class Enums:
    pass


@pytest.fixture(scope="module")
def router(tmp_path_factory):
    so = tmp_path_factory.mktemp("route") / "route_check.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC,
                           os.path.join(ROOT, "tests", "tools", "route_check.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    e = Enums()
    for name in ("FRAME_PLAIN FRAME_DEPTH FRAME_LATENT FRAME_GTBOX FRAME_STAGE BUF_NONE HOST_OUT DEV_OUT DEV_RAW DEV_ZF DEV_CP_STAGE "
                 "CNT_NONE CNT_DEV CNT_DEV_ZF CNT_HOST_CF CNT_DEV_CF CNT_DEV_CP").split():
        v = lib.route_enum(name.encode())
        assert v >= 0, name
        setattr(e, name, v)
    assert len({e.BUF_NONE, e.HOST_OUT, e.DEV_OUT, e.DEV_RAW, e.DEV_ZF, e.DEV_CP_STAGE}) == 6
    assert len({e.CNT_NONE, e.CNT_DEV, e.CNT_DEV_ZF, e.CNT_HOST_CF, e.CNT_DEV_CF, e.CNT_DEV_CP}) == 6

    def route(kind, mode=PBD_CAND_RAW, nms=PBD_NMS_PAINTED, zf_on=0, b3_on=0, cl3_on=0, ps_on=0, compact=0, member=0, zero_copy=1,
              ps_compact_was=0, dp_timed=0):
        """the route as a dict, or None for a refused combination"""
        args = (C.c_int * 13)(kind, mode, nms, zf_on, b3_on, cl3_on, ps_on, compact, member, zero_copy, ps_compact_was, dp_timed, HAS)
        out = (C.c_int * len(ROUTE_FIELDS))(*([-7] * len(ROUTE_FIELDS)))
        if not lib.route_row(args, out):
            return None
        assert -7 not in list(out)
        return dict(zip(ROUTE_FIELDS, out))
    return e, route


def stages(r):
    """the record-writing stages of a route in launch order: (name, in, in_count, out, out_count); the back-tracking reads no records"""
    st = [("bt", None, None, r["bt_out"], r["bt_count"])]
    for s in ("zf", "filter", "parts"):
        if r[f"{s}_on"]:
            st.append((s,) + tuple(r[f"{s}_{f}"] for f in STAGE_FIELDS[1:]))
    return st


def refused(e, kind, mode, zf_on, b3_on, cl3_on, ps_on, member):
    """what the entries refuse: the gt-box entries every post-stage (pbd_i_gt_check); a pbd_group member everything but plain frames
    and the candidate filter (the latent and gt-box checks, the setters of the depth filter, 3-D boxes and part scores)"""
    if kind == e.FRAME_GTBOX and (mode != PBD_CAND_RAW or zf_on or b3_on or cl3_on or ps_on):
        return True
    return bool(member and (kind in (e.FRAME_DEPTH, e.FRAME_LATENT, e.FRAME_GTBOX) or b3_on or ps_on))


def test_every_combination(router):
    e, route = router
    kinds = (e.FRAME_PLAIN, e.FRAME_DEPTH, e.FRAME_LATENT, e.FRAME_GTBOX, e.FRAME_STAGE)
    modes = (PBD_CAND_RAW, PBD_CAND_SORT, PBD_CAND_SORT_NMS)
    host_bufs, dev_counts = {e.HOST_OUT}, {e.CNT_DEV, e.CNT_DEV_ZF, e.CNT_DEV_CF, e.CNT_DEV_CP}
    rows = reachable = 0
    for kind, mode, nms, zf_on, b3_on, cl3_on, ps_on, compact, member, zc in itertools.product(
            kinds, modes, (PBD_NMS_PAINTED, PBD_NMS_PARTS), *([(0, 1)] * 7)):
        rows += 1
        row = dict(kind=kind, mode=mode, nms=nms, zf_on=zf_on, b3_on=b3_on, cl3_on=cl3_on, ps_on=ps_on, compact=compact, member=member, zero_copy=zc)
        r = route(**row)
        # every row the entries refuse comes back as an error, and no reachable row does
        assert (r is None) == refused(e, kind, mode, zf_on, b3_on, cl3_on, ps_on, member), row
        if r is None:
            continue
        reachable += 1
        ctx = (row, r)
        stage = kind == e.FRAME_STAGE
        cm = PBD_CAND_RAW if stage else mode
        # which stages run is the settings' and the kind's alone
        assert r["zf_on"] == (kind == e.FRAME_DEPTH and zf_on), ctx
        assert r["filter_on"] == (cm != PBD_CAND_RAW) == r["filtered"], ctx
        parts = cm == PBD_CAND_SORT_NMS and nms == PBD_NMS_PARTS
        assert r["parts_on"] == parts, ctx
        assert r["filter_mode"] == (PBD_CAND_SORT if parts else cm), ctx
        assert r["latent"] == (kind == e.FRAME_LATENT) and r["gt"] == (kind == e.FRAME_GTBOX) == r["pending_gt"], ctx
        assert r["active"] == 1, ctx
        st = stages(r)
        # each stage's input is the output (records and count) of the stage before it, starting at the back-tracking
        for prev, cur in zip(st, st[1:]):
            assert cur[1] == prev[3] and cur[2] == prev[4], ctx
        # no stage reads the buffer, or the count, it writes; every stage names both
        for _, bi, ci, bo, co in st:
            assert bo != e.BUF_NONE and co != e.CNT_NONE and bi != bo and ci != co, ctx
        # the final records are the output and count of the last record-writing stage
        assert (r["final_buf"], r["final_count"]) == st[-1][3:], ctx
        if kind == e.FRAME_GTBOX:
            # the one route whose records stay on the device: the selection reads the back-tracking's list there and only its winners
            # (pinned slots of their own) and the list's count come home, so the collect has nothing to fetch
            assert r["final_buf"] == e.DEV_OUT and r["on_host"] == 1, ctx
            assert r["count_d2h"] == e.CNT_DEV and not r["first_d2h"] and r["pack_count"] == e.CNT_NONE and len(st) == 1, ctx
        else:
            # on_host holds exactly when that buffer is HOST_OUT
            assert r["on_host"] == (r["final_buf"] == e.HOST_OUT), ctx
        bufs = {s[3] for s in st}
        if member:
            # a member's route names no host buffer and no host count, and ends in exactly one send-block pack, of the final records
            assert not (bufs & host_bufs) and {s[4] for s in st} <= dev_counts and not r["bt_host_count"], ctx
            assert r["count_d2h"] == e.CNT_NONE and not r["first_d2h"], ctx
            assert r["pack_count"] == r["final_count"] and r["final_buf"] == e.DEV_OUT, ctx
        else:
            # a non-member's route never packs; its count and records reach the host one way exactly
            assert r["pack_count"] == e.CNT_NONE, ctx
            if kind != e.FRAME_GTBOX:
                assert r["first_d2h"] == (not r["on_host"]), ctx
                if r["first_d2h"]:      # the fetch of a first block reads DEV_OUT and the back-tracking's count
                    assert r["final_buf"] == e.DEV_OUT and r["final_count"] == e.CNT_DEV == r["count_d2h"], ctx
                ways = [bool(r["bt_host_count"]), r["count_d2h"] != e.CNT_NONE, r["final_count"] == e.CNT_HOST_CF]
                assert sum(ways) == 1, ctx
                if r["count_d2h"] != e.CNT_NONE:
                    assert r["count_d2h"] == r["final_count"], ctx
                assert r["bt_host_count"] <= (r["bt_out"] == e.HOST_OUT and len(st) == 1), ctx
        if stage:   # a stage entry runs no post-stage, selection or mask, and computes nothing per record
            assert len(st) == 1 and not (r["ps"] or r["b3"] or r["cl3"] or r["latent"] or r["gt"] or r["filtered"]), ctx
        # b3 implies DEPTH, cl3 implies b3, ps implies !compact
        assert r["b3"] == (kind == e.FRAME_DEPTH and b3_on) and r["cl3"] == (r["b3"] and cl3_on), ctx
        assert r["b3_has"] == (HAS if r["b3"] else 0), ctx
        assert r["ps"] == (ps_on and not compact and not stage), ctx
        if not stage:
            assert r["ps_compact"] == (ps_on and compact), ctx
    assert rows == 3840 and 0 < reachable < rows


def test_stage_rows_keep_what_the_last_frame_left(router):
    """pbd_get_part_scores tests ps_compact before ps_ready: a stage entry keeps the previous frame's; dp_timed is the caller's"""
    e, route = router
    for was, timed in itertools.product((0, 1), (0, 1)):
        r = route(e.FRAME_STAGE, ps_on=1, compact=1 - was, ps_compact_was=was, dp_timed=timed)
        assert r["ps_compact"] == was and r["dp_timed"] == timed and not r["ps"]
        assert route(e.FRAME_PLAIN, ps_on=1, compact=1 - was, ps_compact_was=was, dp_timed=timed)["ps_compact"] == 1 - was


def expect(e, **kw):
    """a route with nothing on but the back-tracking into DEV_OUT, overridden by kw"""
    r = dict.fromkeys(ROUTE_FIELDS, 0)
    for s in ("zf", "filter", "parts"):
        r.update({f"{s}_in": e.BUF_NONE, f"{s}_out": e.BUF_NONE, f"{s}_in_count": e.CNT_NONE, f"{s}_out_count": e.CNT_NONE})
    r.update(bt_out=e.DEV_OUT, bt_count=e.CNT_DEV, filter_mode=PBD_CAND_RAW, count_d2h=e.CNT_NONE, pack_count=e.CNT_NONE,
             final_buf=e.DEV_OUT, final_count=e.CNT_DEV, active=1)
    r.update(kw)
    return r


def stage_kw(name, bi, ci, bo, co):
    return {f"{name}_on": 1, f"{name}_in": bi, f"{name}_in_count": ci, f"{name}_out": bo, f"{name}_out_count": co}


def test_rows_by_hand(router):
    e, route = router
    H, D, RAW, ZF, CP = e.HOST_OUT, e.DEV_OUT, e.DEV_RAW, e.DEV_ZF, e.DEV_CP_STAGE
    cD, cZ, cHF, cDF, cCP = e.CNT_DEV, e.CNT_DEV_ZF, e.CNT_HOST_CF, e.CNT_DEV_CF, e.CNT_DEV_CP
    cases = {
        # the back-tracking writes records and count into the pinned buffers itself
        "plain zero-copy": (dict(kind=e.FRAME_PLAIN),
                            expect(e, bt_out=H, bt_host_count=1, final_buf=H, on_host=1)),
        # ... into d_cand_out; count and a first block follow by copies
        "plain, zero-copy compiled off": (dict(kind=e.FRAME_PLAIN, zero_copy=0),
                                          expect(e, count_d2h=cD, first_d2h=1)),
        "member raw": (dict(kind=e.FRAME_PLAIN, member=1),
                       expect(e, pack_count=cD)),
        # the filter writes the device buffer the send block is packed from, so the back-tracking goes to d_cand_raw
        "member filtered": (dict(kind=e.FRAME_PLAIN, member=1, mode=PBD_CAND_SORT_NMS),
                            expect(e, bt_out=RAW, filter_mode=PBD_CAND_SORT_NMS, **stage_kw("filter", RAW, cD, D, cDF),
                                   pack_count=cDF, final_count=cDF, filtered=1)),
        # k_zfilter writes the kept records to the host; its count follows by a copy
        "depth + pruning, raw": (dict(kind=e.FRAME_DEPTH, zf_on=1),
                                 expect(e, bt_out=RAW, **stage_kw("zf", RAW, cD, H, cZ), count_d2h=cZ, final_buf=H, final_count=cZ,
                                        on_host=1)),
        "depth + pruning + sort-NMS": (dict(kind=e.FRAME_DEPTH, zf_on=1, mode=PBD_CAND_SORT_NMS),
                                       expect(e, bt_out=RAW, **stage_kw("zf", RAW, cD, ZF, cZ), filter_mode=PBD_CAND_SORT_NMS,
                                              **stage_kw("filter", ZF, cZ, H, cHF), final_buf=H, final_count=cHF, on_host=1,
                                              filtered=1)),
        # no record-writing post-stage: the boxes read the zero-copy records where the back-tracking put them
        "depth without pruning + box3d": (dict(kind=e.FRAME_DEPTH, b3_on=1, cl3_on=1),
                                          expect(e, bt_out=H, bt_host_count=1, final_buf=H, on_host=1, b3=1, cl3=1, b3_has=HAS)),
        # the filter only sorts, into the staging buffer; k_cand_parts writes what it would have written
        "part-wise NMS": (dict(kind=e.FRAME_PLAIN, mode=PBD_CAND_SORT_NMS, nms=PBD_NMS_PARTS, ps_on=1),
                          expect(e, filter_mode=PBD_CAND_SORT, **stage_kw("filter", D, cD, CP, cCP), **stage_kw("parts", CP, cCP, H, cHF),
                                 final_buf=H, final_count=cHF, on_host=1, filtered=1, ps=1)),
        # a device list; only the count (and the winners, in slots of their own) come home
        "gt-box": (dict(kind=e.FRAME_GTBOX),
                   expect(e, gt=1, pending_gt=1, count_d2h=cD, on_host=1)),
        "latent + filter": (dict(kind=e.FRAME_LATENT, mode=PBD_CAND_SORT, zf_on=1, b3_on=1),
                            expect(e, latent=1, filter_mode=PBD_CAND_SORT, **stage_kw("filter", D, cD, H, cHF), final_buf=H,
                                   final_count=cHF, on_host=1, filtered=1)),
    }
    for name, (row, want) in cases.items():
        got = route(**row)
        assert got is not None, name
        assert {k: (got[k], want[k]) for k in ROUTE_FIELDS if got[k] != want[k]} == {}, name
