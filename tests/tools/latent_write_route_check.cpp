// latent_write_route_check.cpp — the route of a latent-positive frame (FRAME_LATENT_WRITE, partsbaseddetector_amd/csrc/pbd_route.hpp)
// on the host: a stand-alone program, built and run by tests/test_latent_write_cpu.py.  It prints one line per property that does not
// hold and returns their number.
#include <cstdio>
#include "pbd_route.hpp"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
  const FrameJob job{FRAME_LATENT_WRITE}, lat{FRAME_LATENT}, mine{FRAME_MINE};
  struct Mode { const char* name; int mode, nms; bool filter, parts; };
  const Mode modes[] = {{"RAW", PBD_CAND_RAW, PBD_NMS_PAINTED, false, false}, {"SORT", PBD_CAND_SORT, PBD_NMS_PAINTED, true, false},
                        {"SORT_NMS", PBD_CAND_SORT_NMS, PBD_NMS_PAINTED, true, false}, {"NMS_PARTS", PBD_CAND_SORT_NMS, PBD_NMS_PARTS, true, true}};
  for (const Mode& m : modes)
    for (int zc = 0; zc < 2; ++zc) {
      RouteSettings s;
      s.cand_mode = m.mode; s.cand_nms = m.nms; s.zero_copy = zc != 0;
      FrameRoute r, l, n;
      const bool ok = route_frame(s, job, &r) && route_frame(s, lat, &l) && route_frame(s, mine, &n);
      CHECK(ok, "%s zero_copy %d: no route", m.name, zc);
      if (!ok) continue;
      // a latent frame (the mask stage, k_latent_best's record) whose records go where a mining frame's go
      CHECK(r.latent && l.latent && !n.latent && !r.gt, "%s: latent flags", m.name);
      const RouteStage* a[] = {&r.bt, &r.zf, &r.filter, &r.parts};
      const RouteStage* b[] = {&n.bt, &n.zf, &n.filter, &n.parts};
      for (int i = 0; i < 4; ++i)
        CHECK(a[i]->on == b[i]->on && a[i]->in == b[i]->in && a[i]->in_count == b[i]->in_count && a[i]->out == b[i]->out &&
              a[i]->out_count == b[i]->out_count, "%s: stage %d differs from the mining frame's", m.name, i);
      CHECK(!r.bt_host_count && r.filter_mode == n.filter_mode, "%s: host count / filter mode", m.name);
      CHECK(r.final_buf == DEV_OUT && r.final_count == (m.filter ? CNT_DEV_CF : CNT_DEV), "%s: final %d %d", m.name, (int)r.final_buf, (int)r.final_count);
      CHECK(r.count_d2h == CNT_DEV && !r.first_d2h && r.pack_count == CNT_NONE, "%s: d2h", m.name);
      const PendingFrame& p = r.pending;
      CHECK(p.active && p.on_host && p.filtered == m.filter && !p.gt && !p.b3 && !p.cl3 && !p.ps && !p.ps_compact, "%s: pending", m.name);
      // the plain latent frame's route is what it was: its final records reach the host
      CHECK(route_on_host(l.final_buf) || l.first_d2h, "%s: the latent frame's records stay on the device", m.name);
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
  // FRAME_LATENT_WRITE is appended: the kinds before it keep their values
  CHECK(FRAME_PLAIN == 0 && FRAME_DEPTH == 1 && FRAME_LATENT == 2 && FRAME_GTBOX == 3 && FRAME_STAGE == 4 && FRAME_MINE == 5 && FRAME_LATENT_WRITE == 6,
        "FrameKind values");
  printf("%d failures\n", failures);
  return failures;
}
