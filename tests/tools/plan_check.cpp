// plan_check.cpp — the frame planner (partsbaseddetector_amd/csrc/pbd_plan.cpp) on the host, with fake buffer addresses: plans a
// model and a frame, then checks the tables the kernels would read (tests/test_plan_cpu.py builds this with the planner and calls
// plan_check through ctypes).  Nothing behind the fake addresses is ever read.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include "pbd_lds.hpp"
#include "pbd_plan.hpp"

namespace {

const char* const kBufName[FB_COUNT] = {"img", "pyr", "feat", "resp", "pk", "rootv", "rooti", "nms_mask", "dt_tmpT", "dt_sdt",
                                        "dt_ixT", "dt_iy", "acc", "feat_split"};

struct Checker {
  const HostModel& hm;
  const FrameLayout& lay;
  const FrameBases& b;
  std::string msg;
  int nerr = 0;
  void bad(const std::string& s) {
    if (nerr++ < 20) msg += s + "\n";
  }
  bool within(int i, const void* p, size_t bytes) const {
    const char* c = (const char*)p;
    return b.p[i] && c >= b.p[i] && c + bytes <= b.p[i] + lay.buf[i].bytes;
  }
  // the buffer p points into, with `bytes` from p inside it; -1: none
  int owner(const void* p, size_t bytes) const {
    for (int i = 0; i < FB_COUNT; ++i)
      if (within(i, p, bytes)) return i;
    return -1;
  }
  void in(const char* what, const void* p, size_t bytes, std::initializer_list<int> allowed) {
    for (int a : allowed)
      if (within(a, p, bytes)) return;
    const int o = owner(p, bytes);
    char s[256];
    snprintf(s, sizeof(s), "%s: %p + %zu B lies in %s", what, p, bytes, o < 0 ? "no buffer (or crosses its end)" : kBufName[o]);
    bad(s);
  }
};

template <typename T>
size_t table_bytes(const std::vector<T>& v) { return (v.empty() ? 1 : v.size()) * sizeof(T); }

// the tables' bytes with the structs' trailing padding cleared (it carries no data)
std::string canonical(const FrameTables& t) {
  std::string s;
  auto add = [&](const void* p, size_t n) { s.append((const char*)p, n); };
  add(t.pyrjobs.data(), t.pyrjobs.size() * sizeof(PyrJob));
  add(t.pyr_launches.data(), t.pyr_launches.size() * sizeof(PyrLaunch));
  add(t.levels.data(), t.levels.size() * sizeof(LevelDev));
  add(t.hog_tiles.data(), t.hog_tiles.size() * sizeof(HogTile));
  add(t.conv_tiles.data(), t.conv_tiles.size() * sizeof(ConvTile));
  add(t.conv_tiles_mix.data(), t.conv_tiles_mix.size() * sizeof(ConvTile));
  add(t.maps.data(), t.maps.size() * sizeof(DtMap));
  add(t.tasks.data(), t.tasks.size() * sizeof(DtTask));
  add(t.folds.data(), t.folds.size() * sizeof(FoldJob));
  add(t.foldx.data(), t.foldx.size() * sizeof(unsigned long long));
  add(t.red.data(), t.red.size() * sizeof(ReduceJob));
  add(t.redblk.data(), t.redblk.size() * sizeof(ReduceBlock));
  add(t.rootblk.data(), t.rootblk.size() * sizeof(ReduceBlock));
  add(t.scr_base.data(), t.scr_base.size() * sizeof(unsigned long long));
  for (RootJob J : t.rootjobs) { memset((char*)&J + offsetof(RootJob, pad) + 4, 0, sizeof(J) - offsetof(RootJob, pad) - 4); add(&J, sizeof(J)); }
  for (BackLevel B : t.back) { memset((char*)&B + offsetof(BackLevel, scale) + 4, 0, sizeof(B) - offsetof(BackLevel, scale) - 4); add(&B, sizeof(B)); }
  for (const RoundLaunch& R : t.rl) {
    const long long v[8] = {R.xtask0, R.nxtasks, R.ytask0, R.nytasks, (long long)R.lds_x, (long long)R.lds_y, R.fold_x, (long long)R.foldx0};
    add(v, sizeof(v));
    add(R.waves.data(), R.waves.size() * sizeof(ReduceWave));
  }
  const long long v[6] = {t.hog_tc, t.dt_nt, (long long)t.dt_lds, t.root_cells, t.root_maxcells, 0};
  add(v, sizeof(v));
  return s;
}

void check_layout(Checker& C) {
  const FrameLayout& lay = C.lay;
  for (int i = 0; i < FB_COUNT; ++i) {
    const BufPlace& p = lay.buf[i];
    if (p.region < 0) continue;
    if (p.region >= (int)lay.regions.size() || p.offset + p.bytes > lay.regions[p.region]) C.bad(std::string(kBufName[i]) + ": outside its region");
  }
  auto allowed = [&](int i, int j) {
    if (!lay.compact) return false;
    auto is = [&](int a, int c) { return (i == a && j == c) || (i == c && j == a); };
    return is(FB_PYR, FB_PK) || is(FB_PYR, FB_DT_TMPT) || is(FB_FEAT, FB_PK) || is(FB_FEAT, FB_DT_TMPT) || is(FB_FEAT_SPLIT, FB_DT_IXT);
  };
  for (int i = 0; i < FB_COUNT; ++i)
    for (int j = i + 1; j < FB_COUNT; ++j) {
      if (!C.b.p[i] || !C.b.p[j]) continue;
      const bool ov = C.b.p[i] < C.b.p[j] + lay.buf[j].bytes && C.b.p[j] < C.b.p[i] + lay.buf[i].bytes;
      if (ov && !allowed(i, j)) C.bad(std::string("overlap: ") + kBufName[i] + " / " + kBufName[j]);
    }
}

void check_dt(Checker& C, const FrameTables& t) {
  const HostModel& hm = C.hm;
  const size_t ts = hm.ts;
  const std::initializer_list<int> scores = {FB_RESP, FB_ACC};
  for (const RoundLaunch& R : t.rl) {
    if (R.lds_x > 160 * 1024 || R.lds_y > 160 * 1024) C.bad("launch LDS over 160 KB");
    for (int pass = 0; pass < 2; ++pass) {
      const int t0 = pass ? R.ytask0 : R.xtask0, nt = pass ? R.nytasks : R.nxtasks;
      const size_t lds = pass ? R.lds_y : R.lds_x;
      std::map<std::pair<int, int>, int> cover;   // (map, line) -> tasks covering it
      std::map<int, std::pair<int, int>> group_maps;   // map0 -> (nmaps, nlines)
      for (int i = t0; i < t0 + nt; ++i) {
        const DtTask& T = t.tasks[i];
        const DtGroup& g = T.g;
        if (dt_lds_bytes(g.stride, g.lpb, hm.ts, t.dt_nt) > lds) C.bad("task needs more LDS than its launch");
        if (((g.fused & DT_G_NATURAL) != 0) != (pass == 0)) C.bad("DT_G_NATURAL not exactly on the x pass");
        group_maps[g.map0] = {g.nmaps, g.nlines};
        if (g.fold >= 0) {
          if (pass || !R.fold_x) C.bad("fold group outside a fold x launch");
          for (int r = T.g0; r < T.g0 + T.nl / g.nmaps; ++r)
            for (int k = 0; k < g.nmaps; ++k) cover[{g.map0 + k, r}]++;
          if (T.nl % g.nmaps) C.bad("fold task: lines not whole rows");
        } else {
          for (int gi = T.g0; gi < T.g0 + T.nl; ++gi) cover[{g.map0 + gi / g.nlines, gi % g.nlines}]++;
          if (T.src0) {
            const DtMap& M = t.maps[(size_t)g.map0 + T.m0];
            if ((const char*)T.src0 != (const char*)M.src + (size_t)T.l0 * g.len * ts) C.bad("DtTask::src0 is not its first line");
            C.in("DtTask::src0", T.src0, (size_t)T.nl * g.len * ts, pass ? std::initializer_list<int>{FB_DT_TMPT} : scores);
          }
        }
      }
      for (const auto& gm : group_maps) {
        for (int k = 0; k < gm.second.first; ++k) {
          const int mi = gm.first + k;
          const DtMap& M = t.maps[mi];
          for (int l = 0; l < gm.second.second; ++l) {
            auto it = cover.find({mi, l});
            if (it == cover.end() || it->second != 1) { C.bad("(map, line) not covered exactly once"); break; }
          }
          // the group's geometry: nlines lines of len elements
          const DtTask* any = nullptr;
          for (int i = t0; i < t0 + nt && !any; ++i) if (t.tasks[i].g.map0 == gm.first) any = &t.tasks[i];
          const size_t n = (size_t)any->g.nlines * any->g.len;
          if (pass == 0) {
            C.in("x DtMap::src", M.src, n * ts, scores);
            C.in("x DtMap::dst", M.dst, n * ts, {FB_DT_TMPT});
            C.in("x DtMap::ptr", M.ptr, n * 2, {FB_DT_IXT});
          } else {
            C.in("y DtMap::src", M.src, n * ts, {FB_DT_TMPT});
            C.in("y DtMap::dst", M.dst, n * ts, {C.lay.compact ? FB_RESP : FB_DT_SDT});
            C.in("y DtMap::ptr", M.ptr, n * 2, {FB_DT_IY});
            const DtMap& X = t.maps[mi - gm.second.first];   // the level's x maps precede its y maps, in the same order
            if (X.dst != M.src) C.bad("y map does not read its x map's output");
            if (C.lay.compact && M.dst != X.src) C.bad("compact: transformed scores outside their mixture's response plane");
          }
        }
      }
      if ((int)cover.size() != [&] { int s = 0; for (auto& gm : group_maps) s += gm.second.first * gm.second.second; return s; }())
        C.bad("tasks cover lines outside their groups");
    }
    // fold x tasks: their loader records
    if (R.fold_x) {
      for (int i = 0; i < R.nxtasks; ++i) {
        const DtTask& T = t.tasks[R.xtask0 + i];
        const unsigned long long* q = &t.foldx[R.foldx0 + (size_t)i * PBD_FOLDX_QW];
        const FoldJob& J = t.folds[T.g.fold];
        bool ok = q[17] == (unsigned long long)J.nch;
        for (int m = 0; m < 8; ++m) ok = ok && q[m] == (unsigned long long)(uintptr_t)t.maps[T.g.map0 + std::min(m, T.g.nmaps - 1)].src;
        for (int k = 0; k < 8; ++k) ok = ok && q[8 + k] == (unsigned long long)(uintptr_t)J.ch[0].sdt[k];
        ok = ok && q[16] == (unsigned long long)(uintptr_t)J.ch[0].ok;
        if (!ok) C.bad("foldx record differs from its task's maps / fold job");
      }
    }
  }
}

void check_fold(Checker& C, const FoldJob& J, size_t HW, int L) {
  for (int c = 0; c < J.nch; ++c) {
    const FoldChild& F = J.ch[c];
    for (int k = 0; k < PBD_FOLD_MAXMIX; ++k) C.in("FoldChild::sdt", F.sdt[k], HW * C.hm.ts, {C.lay.compact ? FB_RESP : FB_DT_SDT});
    C.in("FoldChild::ok", F.ok, HW * L, {FB_PK});
  }
}

void check_tables(Checker& C, const FrameTables& t) {
  const HostModel& hm = C.hm;
  const size_t ts = hm.ts;
  check_dt(C, t);
  for (const RoundLaunch& R : t.rl)
    for (int i = 0; R.fold_x && i < R.nxtasks; ++i) {
      const DtGroup& g = t.tasks[R.xtask0 + i].g;
      check_fold(C, t.folds[g.fold], (size_t)g.nlines * g.len, g.nmaps);
    }
  for (const ReduceJob& J : t.red) {
    const size_t HW = (size_t)J.H * J.W;
    for (int m = 0; m < J.L; ++m) {
      C.in("ReduceJob::par_in", J.par_in[m], HW * ts, {FB_RESP, FB_ACC});
      C.in("ReduceJob::par_out", J.par_out[m], HW * ts, {FB_ACC});
    }
    for (int c = 0; c < J.nch; ++c) {
      C.in("ReduceChild::sdt", J.ch[c].sdt, HW * ts * J.ch[c].K, {FB_DT_SDT});
      C.in("ReduceChild::ok", J.ch[c].ok, HW * J.L, {FB_PK});
    }
  }
  unsigned maxc = 0;
  for (const RootJob& J : t.rootjobs) {
    const size_t HW = (size_t)J.H * J.W;
    maxc = std::max(maxc, (unsigned)HW);
    for (int k = 0; k < PBD_MAX_MIX; ++k) C.in("RootJob::score", J.score[k], HW * ts, {FB_RESP, FB_ACC});
    C.in("RootJob::rootv", J.rootv, HW * ts, {FB_ROOTV});
    C.in("RootJob::rooti", J.rooti, HW * 4, {FB_ROOTI});
    if (J.fold >= 0) check_fold(C, t.folds[J.fold], HW, J.K);
    if ((J.fold >= 0) != hm.fold) C.bad("RootJob::fold does not follow the DP structure");
  }
  if (maxc != t.root_maxcells) C.bad("root_maxcells");
  const int nc = hm.md.ncomponents;
  for (int l = 0; l < C.lay.nvl; ++l)
    for (int c = 0; c < nc; ++c) {
      const BackLevel& B = t.back[(size_t)l * nc + c];
      const size_t HW = (size_t)B.H * B.W;
      if (!HW) continue;
      C.in("BackLevel::pk", B.pk, HW * std::max(1, hm.comp_plane0[c + 1] - hm.comp_plane0[c]), {FB_PK});
      C.in("BackLevel::rootv", B.rootv, HW * ts, {FB_ROOTV});
      C.in("BackLevel::rooti", B.rooti, HW * 4, {FB_ROOTI});
    }
  // scr_base: the DT pointer planes of (level, part) inside dt_ixT / dt_iy
  for (int l = 0; l < C.lay.nvl; ++l)
    for (size_t fp = 0; fp < hm.parts.size(); ++fp)
      if (hm.parts[fp].p > 0 && C.lay.lv[l].active) {
        const size_t e = t.scr_base[(size_t)l * hm.parts.size() + fp] + (size_t)hm.parts[fp].K * C.lay.lv[l].cw * C.lay.lv[l].ch;
        if (e > C.lay.dt_cap_elems) C.bad("scr_base beyond the DT pointer planes");
      }
}

}  // namespace

extern "C" int plan_check(const pbd_model_desc* md, const int32_t* fsize, int sized, const pbd_options* opt, int w, int h, int cn,
                          int batch, int depth, const int32_t* levels, int nlevels, int ncu, unsigned long long* frame_bytes, char* report,
                          int report_len) {
  auto say = [&](const std::string& s) { if (report && report_len > 0) snprintf(report, report_len, "%s", s.c_str()); };
  HostModel hm;
  std::string err;
  int rc = plan_model(hm, md, fsize, sized != 0, opt, &err);
  if (rc) { say("plan_model: " + err); return rc; }
  FrameSpec f;
  f.w = w; f.h = h; f.cn = cn; f.batch = batch; f.depth = depth;
  for (int i = 0; i < nlevels; ++i) {
    if ((int)f.level_set.size() <= levels[i]) f.level_set.resize(levels[i] + 1, 0);
    f.level_set[levels[i]] = 1;
  }
  FrameLayout lay;
  if ((rc = plan_layout(hm, f, lay, &err))) { say("plan_layout: " + err); return rc; }
  // fake, disjoint, aligned regions 1 TiB apart
  std::vector<char*> regions;
  for (size_t i = 0; i < lay.regions.size(); ++i) regions.push_back((char*)(uintptr_t)((1ull << 44) + (i << 40)));
  const FrameBases b = frame_bases(lay, regions.data());
  FrameTables t, t2;
  const PlanKnobs kn;
  if ((rc = plan_tables(hm, f, lay, b, ncu, 0, kn, t, &err))) { say("plan_tables: " + err); return rc; }
  // the device memory the plan holds: one allocation per region, one per uploaded table (pbd_api.cpp: plan_frame)
  unsigned long long total = 0;
  for (size_t r : lay.regions) total += r;
  total += table_bytes(t.pyrjobs) + table_bytes(t.levels) + table_bytes(t.hog_tiles) + table_bytes(t.conv_tiles) +
           (hm.mixed ? table_bytes(t.conv_tiles_mix) : 0) + table_bytes(t.maps) + table_bytes(t.tasks) + table_bytes(t.folds) +
           table_bytes(t.foldx) + table_bytes(t.red) + table_bytes(t.redblk) + table_bytes(t.rootjobs) + table_bytes(t.rootblk) +
           table_bytes(t.back) + table_bytes(t.scr_base);
  if (frame_bytes) *frame_bytes = total;
  Checker C{hm, lay, b, "", 0};
  check_layout(C);
  check_tables(C, t);
  if (plan_tables(hm, f, lay, b, ncu, 0, kn, t2, &err) || canonical(t) != canonical(t2)) C.bad("planning twice gives different tables");
  char head[160];
  snprintf(head, sizeof(head), "%s plan, %d virtual levels, %zu regions, %zu tasks, %zu folds, %zu reduce jobs, %zu root jobs\n",
           lay.compact ? "compact" : "default", lay.nvl, lay.regions.size(), t.tasks.size(), t.folds.size(), t.red.size(), t.rootjobs.size());
  say(std::string(head) + C.msg);
  return C.nerr ? 100 : PBD_OK;
}
