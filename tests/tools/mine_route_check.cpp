// mine_route_check.cpp — the route of a mining frame (FRAME_MINE, partsbaseddetector_amd/csrc/pbd_route.hpp) on the host: a stand-alone
// program, built and run by tests/test_mine_cpu.py.  It prints one line per property that does not hold and returns their number.
#include <cstdio>
#include "pbd_route.hpp"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static bool on_device(RouteBuf b) { return b == DEV_OUT || b == DEV_RAW || b == DEV_ZF || b == DEV_CP_STAGE; }

int main() {
  const FrameJob job{FRAME_MINE};
  struct Mode { const char* name; int mode, nms; bool filter, parts; };
  const Mode modes[] = {{"RAW", PBD_CAND_RAW, PBD_NMS_PAINTED, false, false}, {"SORT", PBD_CAND_SORT, PBD_NMS_PAINTED, true, false},
                        {"SORT_NMS", PBD_CAND_SORT_NMS, PBD_NMS_PAINTED, true, false}, {"NMS_PARTS", PBD_CAND_SORT_NMS, PBD_NMS_PARTS, true, true}};
  for (const Mode& m : modes)
    for (int zc = 0; zc < 2; ++zc) {
      RouteSettings s;
      s.cand_mode = m.mode; s.cand_nms = m.nms; s.zero_copy = zc != 0;
      FrameRoute r;
      const bool ok = route_frame(s, job, &r);
      CHECK(ok, "%s zero_copy %d: no route", m.name, zc);
      if (!ok) continue;
      // no stage writes the pinned host buffer or a host count; every buffer named is a device buffer
      const RouteStage* st[] = {&r.bt, &r.zf, &r.filter, &r.parts};
      for (const RouteStage* t : st) {
        if (!t->on) continue;
        CHECK(t->out != HOST_OUT && on_device(t->out), "%s: a stage writes buffer %d", m.name, (int)t->out);
        CHECK(!route_on_host(t->out_count) && t->out_count != CNT_NONE, "%s: a stage writes count %d", m.name, (int)t->out_count);
        CHECK(t == &r.bt || (t->in != t->out && t->in_count != t->out_count), "%s: a stage reads what it writes", m.name);
      }
      CHECK(!r.bt_host_count, "%s: the back-tracking writes the host count", m.name);
      CHECK(!r.zf.on && r.filter.on == m.filter && r.parts.on == m.parts, "%s: stages %d %d %d", m.name, r.zf.on, r.filter.on, r.parts.on);
      CHECK(r.filter_mode == (m.parts ? PBD_CAND_SORT : m.mode), "%s: filter mode %d", m.name, r.filter_mode);
      // the final records: DEV_OUT, counted on the device (the filter's count block when one runs)
      CHECK(r.final_buf == DEV_OUT, "%s: final_buf %d", m.name, (int)r.final_buf);
      CHECK(r.final_count == (m.filter ? CNT_DEV_CF : CNT_DEV), "%s: final_count %d", m.name, (int)r.final_count);
      const RouteStage& last = m.parts ? r.parts : m.filter ? r.filter : r.bt;
      CHECK(last.out == r.final_buf && last.out_count == r.final_count, "%s: the last stage does not write the final records", m.name);
      if (m.filter) CHECK(r.filter.in == r.bt.out && r.filter.in_count == r.bt.out_count, "%s: the filter does not read the back-tracking", m.name);
      if (m.parts) CHECK(r.parts.in == r.filter.out && r.parts.in_count == r.filter.out_count, "%s: the parts NMS does not read the filter", m.name);
      // only a count is copied back: no first block of records, no send block
      CHECK(r.count_d2h == CNT_DEV && !r.first_d2h && r.pack_count == CNT_NONE, "%s: d2h %d %d %d", m.name, (int)r.count_d2h, r.first_d2h, (int)r.pack_count);
      CHECK(!r.latent && !r.gt, "%s: latent / gt", m.name);
      const PendingFrame& p = r.pending;
      CHECK(p.active && p.on_host && p.filtered == m.filter && !p.gt && !p.b3 && !p.cl3 && !p.ps && !p.ps_compact, "%s: pending", m.name);
      // the refused combinations
      struct Off { const char* name; bool RouteSettings::*flag; };
      const Off offs[] = {{"member", &RouteSettings::member}, {"compact", &RouteSettings::compact}, {"depth pruning", &RouteSettings::zf_on},
                          {"3-D boxes", &RouteSettings::b3_on}, {"object clusters", &RouteSettings::cl3_on}, {"part scores", &RouteSettings::ps_on}};
      for (const Off& o : offs) {
        RouteSettings t = s;
        t.*(o.flag) = true;
        FrameRoute q;
        CHECK(!route_frame(t, job, &q), "%s with %s: routed", m.name, o.name);
      }
    }
  // FRAME_MINE is appended: the kinds before it keep their values
  CHECK(FRAME_PLAIN == 0 && FRAME_DEPTH == 1 && FRAME_LATENT == 2 && FRAME_GTBOX == 3 && FRAME_STAGE == 4 && FRAME_MINE == 5, "FrameKind values");
  printf("%d failures\n", failures);
  return failures;
}
