// route_check.cpp — the frame route (partsbaseddetector_amd/csrc/pbd_route.hpp) on the host: tests/test_route_cpu.py builds this with
// g++ and calls route_row through ctypes, one call per combination of settings and frame kind.  Plain data in, plain data out: the
// invariants are stated in the test.
#include <cstring>
#include <initializer_list>
#include "pbd_route.hpp"

extern "C" {

// the value of an enumerator of pbd_route.hpp by name; -1: unknown
int route_enum(const char* name) {
#define E(x) if (!strcmp(name, #x)) return (int)x;
  E(FRAME_PLAIN) E(FRAME_DEPTH) E(FRAME_LATENT) E(FRAME_GTBOX) E(FRAME_STAGE)
  E(BUF_NONE) E(HOST_OUT) E(DEV_OUT) E(DEV_RAW) E(DEV_ZF) E(DEV_CP_STAGE)
  E(CNT_NONE) E(CNT_DEV) E(CNT_DEV_ZF) E(CNT_HOST_CF) E(CNT_DEV_CF) E(CNT_DEV_CP)
#undef E
  return -1;
}

// in:  kind, cand_mode, cand_nms, zf_on, b3_on, cl3_on, ps_on, compact, member, zero_copy, ps_compact_was, dp_timed, has
// out: the route, field by field (ROUTE_FIELDS of the test, in this order); returns 1, or 0 for a refused combination
int route_row(const int* in, int* out) {
  RouteSettings s;
  FrameJob job;
  job.kind = (FrameKind)in[0];
  s.cand_mode = in[1]; s.cand_nms = in[2];
  s.zf_on = in[3]; s.b3_on = in[4]; s.cl3_on = in[5]; s.ps_on = in[6];
  s.compact = in[7]; s.member = in[8]; s.zero_copy = in[9];
  s.ps_compact_was = in[10]; s.dp_timed = in[11];
  job.z.has = (unsigned long long)in[12];
  FrameRoute r;
  if (!route_frame(s, job, &r)) return 0;
  int n = 0;
  out[n++] = r.latent; out[n++] = r.gt;
  out[n++] = r.bt.out; out[n++] = r.bt.out_count; out[n++] = r.bt_host_count;
  for (const RouteStage* st : {&r.zf, &r.filter, &r.parts}) {
    out[n++] = st->on; out[n++] = st->in; out[n++] = st->in_count; out[n++] = st->out; out[n++] = st->out_count;
  }
  out[n++] = r.filter_mode;
  out[n++] = r.count_d2h; out[n++] = r.first_d2h; out[n++] = r.pack_count;
  out[n++] = r.final_buf; out[n++] = r.final_count;
  const PendingFrame& p = r.pending;
  out[n++] = p.active; out[n++] = p.on_host; out[n++] = p.filtered; out[n++] = p.gt;
  out[n++] = p.b3; out[n++] = p.cl3; out[n++] = (int)p.b3_has;
  out[n++] = p.ps; out[n++] = p.ps_compact; out[n++] = p.dp_timed;
  return 1;
}

}  // extern "C"
